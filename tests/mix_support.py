"""The mixer's definition (include/adsb_hip.h, "Frequency shift") restated in numpy with an int64 accumulator, and
composed with the restated decimator and resampler (tests/decim_support.py, tests/resamp_support.py): the definition is
compositional, so the device must equal restated FIR o restated mixer bit for bit.  No GPU, no library.

    t   = m mod N
    re' = clamp((x.re c[t] - x.im s[t] + 8192) >> 14, -32768, 32767)
    im' = clamp((x.re s[t] + x.im c[t] + 8192) >> 14, -32768, 32767)          >> arithmetic, a half rounds up
"""
import numpy as np

from tests import decim_support as ds
from tests import resamp_support as rs

MAX_PERIOD = 256


def mix(x, w, P: int = 0) -> np.ndarray:
    """x ((n, 2) int16 [re, im]), the stream's samples P .. P + n - 1, through the table w ((N, 2) int16 {c, s}; None: no
    mixer) -> (n, 2) int16."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    if w is None:
        return x.astype(np.int16)
    w = np.asarray(w, dtype=np.int64).reshape(-1, 2)
    assert 1 <= len(w) <= MAX_PERIOD and np.abs(w).max() <= 32767
    t = (int(P) + np.arange(len(x))) % len(w)
    c, s = w[t, 0], w[t, 1]
    re = (x[:, 0] * c - x[:, 1] * s + 8192) >> 14
    im = (x[:, 0] * s + x[:, 1] * c + 8192) >> 14
    return np.clip(np.stack([re, im], axis=1), -32768, 32767).astype(np.int16)


def table(k: int, N: int) -> np.ndarray:
    """What adsb_mix_table describes, from numpy: round(16384 cos / sin (2 pi k t / N))."""
    a = 2 * np.pi * ((int(k) * np.arange(N)) % N) / N
    return np.stack([np.rint(16384 * np.cos(a)), np.rint(16384 * np.sin(a))], axis=1).astype(np.int16)


def rotation(k: int) -> np.ndarray:
    """The exact table of a rotation by k quarter turns per sample (N = 4)."""
    quarter = [(16384, 0), (0, 16384), (-16384, 0), (0, -16384)]
    return np.array([quarter[(k * t) % 4] for t in range(4)], np.int16)


def random_table(rng, N: int) -> np.ndarray:
    """N random entries in -32767 .. 32767 with both bounds and a zero among them (where N has the room)."""
    w = rng.integers(-32767, 32768, size=(N, 2), dtype=np.int64)
    for i, v in enumerate([(32767, -32767), (-32767, 32767), (32767, 32767), (-32767, -32767), (0, 0)][:N]):
        w[N - 1 - i] = v   # (N - 1 first: the entry in front of the wrap)
    return w.astype(np.int16)


def shift_spectrum(x, k: int, N: int) -> np.ndarray:
    """x moved by k / N cycles per sample in double precision, rounded to int16: how an offset-tuned radio would have
    delivered the stream (clipped at the rails)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    a = 2 * np.pi * ((int(k) * np.arange(len(x))) % N) / N
    z = (x[:, 0] + 1j * x[:, 1]) * np.exp(1j * a)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)), -32768, 32767).astype(np.int16)


class _Mixed:
    """A streaming restatement with a mixer in front of it: the table is applied by the absolute index P."""

    def __init__(self, inner):
        self.inner, self.w = inner, None

    @property
    def P(self) -> int:
        return self.inner.P

    def set_mixer(self, w) -> None:
        self.w = None if w is None else np.asarray(w, dtype=np.int16).reshape(-1, 2)

    def reset(self) -> None:
        self.inner.reset()

    def out_count(self, n_in: int) -> int:
        return self.inner.out_count(n_in)

    def run(self, x) -> np.ndarray:
        return self.inner.run(mix(x, self.w, self.inner.P))


class DecimStream(_Mixed):
    def __init__(self, h, D: int, s: int, w=None):
        super().__init__(ds.Stream(h, D, s))
        self.set_mixer(w)


class ResampStream(_Mixed):
    def __init__(self, h, L: int, M: int, s: int, w=None):
        super().__init__(rs.Stream(h, L, M, s))
        self.set_mixer(w)


def decimate(x, h, D: int, s: int, w) -> np.ndarray:
    return ds.decimate(mix(x, w, 0), h, D, s)


def resample(x, h, L: int, M: int, s: int, w) -> np.ndarray:
    return rs.resample(mix(x, w, 0), h, L, M, s)

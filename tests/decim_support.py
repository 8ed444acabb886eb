"""The decimator's definition (include/adsb_hip.h, "Decimation") restated in numpy with an int64 accumulator: a direct
transcription of the formulas, one call and streaming, which the device is held to bit for bit.  No GPU, no library.

    acc  = sum_k h[k] x[n D - k]          x[m] = 0 for m < 0
    y[n] = clamp((acc + r) >> s, -32768, 32767),  r = 1 << (s - 1) or 0 when s == 0,  >> arithmetic
    a call of n_in inputs behind P consumed ones produces the y[n] with P <= n D < P + n_in
"""
import numpy as np

CHUNK = 131072


def _finish(acc: np.ndarray, s: int) -> np.ndarray:
    r = (1 << (s - 1)) if s else 0
    return np.clip((acc + r) >> s, -32768, 32767).astype(np.int16)


def decimate(x, h, D: int, s: int) -> np.ndarray:
    """The whole stream x ((N, 2) int16 [re, im]) in one call -> y ((ceil(N / D), 2) int16)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    h = np.asarray(h, dtype=np.int64)
    T, N = len(h), len(x)
    n = np.arange(-(-N // D))
    xp = np.concatenate([np.zeros((T - 1, 2), np.int64), x])   # xp[m + T - 1] = x[m]
    acc = np.zeros((len(n), 2), np.int64)
    for k in range(T):
        acc += h[k] * xp[n * D - k + T - 1]
    return _finish(acc, s)


class Stream:
    """The streaming form: P and the last T - 1 inputs, as the decimator keeps them."""

    def __init__(self, h, D: int, s: int):
        self.h, self.D, self.s = np.asarray(h, dtype=np.int64), int(D), int(s)
        self.reset()

    def reset(self) -> None:
        self.P = 0
        self.hist = np.zeros((len(self.h) - 1, 2), np.int64)

    def out_count(self, n_in: int) -> int:
        D, P = self.D, self.P
        return -(-(P + n_in) // D) - -(-P // D)

    def run(self, x) -> np.ndarray:
        x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
        T, D, P = len(self.h), self.D, self.P
        n = np.arange(-(-P // D), -(-(P + len(x)) // D))   # P <= n D < P + n_in
        full = np.concatenate([self.hist, x])              # full[i + T - 1] = input i of this call
        acc = np.zeros((len(n), 2), np.int64)
        for k in range(T):
            acc += self.h[k] * full[n * D - P - k + T - 1]
        self.hist = full[len(full) - (T - 1):]
        self.P = P + len(x)
        return _finish(acc, self.s)


def cut_plan(rng, total: int, lengths, D: int):
    """Call lengths that cut a stream of `total` inputs: D calls of one input first (so that every residue of P mod D
    stands at a cut), then every length of `lengths` once in a random order, then draws from them until the stream is
    used up (the last call takes what is left)."""
    plan = [1] * D + [int(n) for n in rng.permutation(lengths)]
    while sum(plan) < total:
        plan.append(int(rng.choice(lengths)))
    out, left = [], total
    for n in plan:
        n = min(n, left)
        out.append(n)
        left -= n
        if left == 0 and n:
            break
    return out


def random_taps(rng, T: int, total: int = 65534) -> np.ndarray:
    """T random signed int16 taps with sum |h| = total (or T * 32767 where that is less: T = 1)."""
    total = min(total, T * 32767)
    mag = rng.multinomial(total, rng.dirichlet(np.ones(T))).astype(np.int64)
    while mag.max() > 32767:   # (few taps: hand a tap's excess to the smallest)
        i, j = int(mag.argmax()), int(mag.argmin())
        mag[j] += mag[i] - 32767
        mag[i] = 32767
    assert mag.sum() == total
    return (mag * rng.choice([-1, 1], size=T)).astype(np.int16)


def random_iq(rng, n: int, run: int = 0) -> np.ndarray:
    """Full-range random (n, 2) int16 with runs of both rails (-32768 and 32767) of length `run` in it."""
    x = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int64).astype(np.int16)
    for rail in (-32768, 32767, -32768):
        if run and n > run:
            at = int(rng.integers(0, n - run))
            x[at:at + run, int(rng.integers(0, 2))] = rail
            x[at:at + run // 2 + 1] = rail
    return x


def hamming_sinc_taps(D: int) -> np.ndarray:
    """What adsb_decim_default_taps describes -- 8 D + 1 taps of a Hamming-windowed sinc with its cutoff at 1.2 MHz,
    round(h * 32768) -- from numpy, so that an expectation built on it does not hang on the library's libm."""
    M = 8 * D
    i = np.arange(M + 1)
    w = np.sinc((i - M // 2) / D) * (0.54 - 0.46 * np.cos(2 * np.pi * i / M))
    return np.rint(w / w.sum() * 32768).astype(np.int16)

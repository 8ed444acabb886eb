"""The resampler's definition (include/adsb_hip.h, "Resampling") restated in numpy with an int64 accumulator: a direct
transcription of the formulas, one call and streaming, which the device is held to bit for bit.  No GPU, no library.

    p = (n M) mod L,  q = floor(n M / L)
    acc  = sum over j >= 0 with p + j L < T of h[p + j L] x[q - j]          x[m] = 0 for m < 0
    y[n] = clamp((acc + r) >> s, -32768, 32767),  r = 1 << (s - 1) or 0 when s == 0,  >> arithmetic
    a call of n_in inputs behind P consumed ones produces the y[n] with ceil(P L / M) <= n < ceil((P + n_in) L / M)
"""
import numpy as np

from tests.decim_support import _finish, cut_plan, rail_u8_table, random_iq  # noqa: F401  (shared with the decimator's tests)

CHUNK = 131072

# the ratios of the radios the header names: rate in Hz -> (L, M)
RADIO_RATES = {2_500_000: (24, 25), 10_000_000: (6, 25), 3_000_000: (4, 5), 6_000_000: (2, 5), 8_000_000: (3, 10),
               20_000_000: (3, 25), 2_000_000: (6, 5), 2_560_000: (15, 16), 3_200_000: (3, 4), 12_500_000: (24, 125)}
TABLE_RATIOS = sorted(set(RADIO_RATES.values()))   # ten, each once


# tests/test_gpu_resamp_edges.py: the ratios whose tile geometry (resamp_rows) the radios' ratios do not reach
EDGE_RATIOS = [(16, 15),                                # 128 rows with L a multiple of four
               (2, 1),                                  # L = 2 M: every input feeds two outputs
               (4, 3), (31, 128),                       # 512 rows with L = 4; 64 rows, a tile below 2048, uneven units
               (5, 56), (7, 54),                        # the largest LDS requests (65 440 and 65 360 bytes at K = 512)
               (33, 17), (33, 128), (48, 49),           # 64 rows, tiles of 2112 and 3072 outputs
               (96, 95), (64, 127), (128, 65),          # 64 rows, tiles of 6144, 4096 and 8192
               (128, 127), (127, 128), (117, 128)]      # 32 rows: half of every wave has no member
# ... and the ratios tests/test_gpu_resamp.py and tests/test_gpu_mix.py launch on the device
FIRST_FILES_RATIOS = [(1, 1), (1, 2), (1, 5), (1, 16), (2, 5), (3, 4), (3, 10), (3, 25), (4, 5), (6, 5), (6, 25), (15, 16),
                      (24, 25), (24, 125)]
MAX_RATIO = 128


def accepted_ratios():
    """Every (L, M) adsb_resamp_create accepts (include/adsb_hip.h): coprime, both 1..128, L <= 2 M, M <= 16 L."""
    from math import gcd
    return [(L, M) for L in range(1, MAX_RATIO + 1) for M in range(1, MAX_RATIO + 1)
            if gcd(L, M) == 1 and L <= 2 * M and M <= 16 * L]


def tile_class(L: int, tile: int):
    """What decides the paths k_resamp takes at a ratio: the rows of a class (below 64: a wave is partly idle), whether
    the staged tile is larger than 2048 outputs, and whether L is no multiple of four (at 64 rows and fewer the tile has
    L units, which then do not divide evenly among the four waves)."""
    return tile // L, tile > 2048, L % 4 != 0


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def phase_taps(L: int, T: int) -> int:
    """K = ceil(T / L): the most taps one output uses."""
    return ceil_div(T, L)


def out_range(L: int, M: int, P: int, n_in: int):
    """(first output, number of outputs) of a call of n_in inputs behind P consumed ones.  Python integers."""
    first = ceil_div(P * L, M)
    return first, ceil_div((P + n_in) * L, M) - first


def out_count(L: int, M: int, P: int, n_in: int) -> int:
    return out_range(L, M, P, n_in)[1]


def _outputs(n, full, origin: int, h, L: int, M: int, s: int) -> np.ndarray:
    """y[n] for the output indices n, from full[m + origin] = x[m] (zeros or history in front of the call included)."""
    T = len(h)
    K = phase_taps(L, T)
    p, q = (n * M) % L, (n * M) // L
    hp = np.concatenate([h, np.zeros(K * L - T, np.int64)])   # h[k] = 0 for k >= T
    acc = np.zeros((len(n), 2), np.int64)
    for j in range(K):
        acc += hp[p + j * L][:, None] * full[q - j + origin]
    return _finish(acc, s)


def resample(x, h, L: int, M: int, s: int) -> np.ndarray:
    """The whole stream x ((N, 2) int16 [re, im]) in one call -> y ((ceil(N L / M), 2) int16)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    h = np.asarray(h, dtype=np.int64)
    K = phase_taps(L, len(h))
    n = np.arange(ceil_div(len(x) * L, M))
    full = np.concatenate([np.zeros((K - 1, 2), np.int64), x])   # full[m + K - 1] = x[m]
    return _outputs(n, full, K - 1, h, L, M, s)


class Stream:
    """The streaming form: P and the last K - 1 inputs, as the resampler keeps them."""

    def __init__(self, h, L: int, M: int, s: int):
        self.h, self.L, self.M, self.s = np.asarray(h, dtype=np.int64), int(L), int(M), int(s)
        self.K = phase_taps(self.L, len(self.h))
        self.reset()

    def reset(self) -> None:
        self.P = 0
        self.hist = np.zeros((self.K - 1, 2), np.int64)

    def out_count(self, n_in: int) -> int:
        return out_count(self.L, self.M, self.P, n_in)

    def run(self, x) -> np.ndarray:
        x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
        first, count = out_range(self.L, self.M, self.P, len(x))
        n = np.arange(first, first + count)
        full = np.concatenate([self.hist, x])   # full[i + K - 1] = input i of this call = x[P + i]
        y = _outputs(n, full, self.K - 1 - self.P, self.h, self.L, self.M, self.s)
        self.hist = full[len(full) - (self.K - 1):]
        self.P += len(x)
        return y


def random_phase_taps(rng, T: int, L: int, total: int = 65534) -> np.ndarray:
    """T random signed int16 taps whose every phase p has sum_j |h[p + j L]| = total (or 32767 times the phase's tap
    count where that is less)."""
    from tests.decim_support import random_taps
    h = np.zeros(T, np.int16)
    for p in range(min(L, T)):
        h[p::L] = random_taps(rng, len(h[p::L]), total)
    return h


def phase_abs_sums(h, L: int) -> np.ndarray:
    h = np.abs(np.asarray(h, dtype=np.int64))
    return np.array([h[p::L].sum() for p in range(L)])


def max_taps(L: int) -> int:
    """The largest T with K = 512 (and T <= 4096)."""
    return min(512 * L, 4096)


def hamming_sinc_taps(L: int, M: int) -> np.ndarray:
    """What adsb_resamp_default_taps describes -- 8 max(L, M) + 1 taps of a Hamming-windowed sinc over the zero-stuffed
    rate with its cutoff at half the lower of the two rates, scaled to sum L 2^14 and rounded -- from numpy's sinc, so that
    an expectation built on it does not hang on the library's libm.  Shift 14."""
    big = max(L, M)
    N = 8 * big
    i = np.arange(N + 1)
    w = np.sinc((i - N // 2) / big) * (0.54 - 0.46 * np.cos(2 * np.pi * i / N))
    return np.rint(w / w.sum() * L * 16384).astype(np.int16)


def hold_input(y, L: int, M: int, rng) -> np.ndarray:
    """An input x with x[floor(n M / L)] = y[n] (L <= M: every output has an input of its own) and random samples
    elsewhere: with h = [1] * L and s = 0 it resamples to y exactly."""
    assert L <= M
    y = np.asarray(y, dtype=np.int16).reshape(-1, 2)
    n = np.arange(len(y))
    q = (n * M) // L
    x = rng.integers(-32768, 32768, size=(int(q[-1]) + 1, 2), dtype=np.int64).astype(np.int16)
    x[q] = y
    return x


def inputs_for(L: int, M: int, P: int, count: int) -> int:
    """The fewest inputs behind P consumed ones that give at least `count` outputs: up to the newest input of the last."""
    if count == 0:
        return 0
    last = ceil_div(P * L, M) + count - 1
    return (last * M) // L - P + 1


def window_inputs(first_output: int, count: int, T: int, L: int, M: int):
    """[lo, hi): the inputs resample_window needs for outputs first_output .. first_output + count - 1."""
    K = phase_taps(L, T)
    return max((first_output * M) // L - (K - 1), 0), ((first_output + count - 1) * M) // L + 1


def resample_window(x_window, first_output: int, count: int, h, L: int, M: int, s: int) -> np.ndarray:
    """Outputs first_output .. first_output + count - 1 of a stream from a window of its inputs: x_window[0] is input
    window_inputs(...)[0] of the stream and the window reaches the newest input of the last output."""
    x = np.asarray(x_window, dtype=np.int64).reshape(-1, 2)
    h = np.asarray(h, dtype=np.int64)
    K = phase_taps(L, len(h))
    lo, hi = window_inputs(first_output, count, len(h), L, M)
    assert count == 0 or len(x) >= hi - lo
    n = np.arange(first_output, first_output + count)
    full = np.concatenate([np.zeros((K - 1, 2), np.int64), x])   # full[m - lo + K - 1] = x[m]
    # (behind a window that starts inside the stream no output reaches the padding: lo is the oldest input of the first)
    assert count == 0 or lo == 0 or (first_output * M) // L - (K - 1) == lo
    return _outputs(n, full, K - 1 - lo, h, L, M, s)


def tile_base(blk: int, q0: int, L: int, M: int, K: int, tile: int) -> int:
    """The input index (0 = the call's first input) k_resamp's tile `blk` puts its buffer resource at: the 8-sample
    boundary below (the first input the tile needs) - 8, or 0.  The first input the tile needs is its first output's
    newest input, q0 + blk R M, less the K - 1 in front of it (R = tile / L; q0: the call's first output's newest input)."""
    i0 = q0 + blk * (tile // L) * M - (K - 1)
    return max((i0 - 8) & ~7, 0)


def rail_window(x, h, L: int, M: int, n0: int, polarity: int):
    """Puts the rail of each tap's sign (times the polarity) behind output n0 in x, on both components, and returns
    (the accumulator these inputs give output n0, sum |h| of its phase).  Python integers."""
    h = [int(v) for v in np.asarray(h)]
    p, q = (n0 * M) % L, (n0 * M) // L
    taps = h[p::L]
    assert q >= len(taps) - 1
    from tests.decim_support import rail_for
    acc = 0
    for j, hj in enumerate(taps):
        x[q - j] = rail_for(hj, polarity)
        acc += hj * int(x[q - j, 0])
    return acc, sum(abs(v) for v in taps)

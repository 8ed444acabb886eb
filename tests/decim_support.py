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


def grid_taps(D: int):
    """The tap counts every factor is run at (tests/test_gpu_decim_edges.py, "every factor")."""
    return sorted({1, D + 1, 8 * D + 1, 505, 511, 512} | ({D - 1} if D > 1 else set()))


def row_ceiling(D: int, T: int, tile: int) -> int:
    """ceil((tile D + T + 15) / D): a row of the kernel's polyphase store before it is made odd (decim_row_len)."""
    return -(-(tile * D + T + 15) // D)


def rail_for(hk: int, polarity: int, lo: int = -32768, hi: int = 32767) -> int:
    """The rail that gives h[k] x the sign of `polarity`."""
    return hi if polarity * int(hk) > 0 else lo


def worst_case_iq(h, D: int, n0: int, n: int, polarity: int, seed: int = 0, lo: int = -32768, hi: int = 32767,
                  dtype=np.int16) -> np.ndarray:
    """Full-range random (n, 2) samples in which x[n0 D - k] = polarity sign(h[k]) rail (lo or hi) on both components
    for every k with n0 D - k >= 0: output n0's accumulator is the extreme these taps allow, positive for polarity 1
    and negative for -1.  (A zero tap's sample stays random.)  lo, hi, dtype: bytes 0 and 255 for the 8-bit format."""
    rng = np.random.default_rng([seed, D, n0, n, polarity % 3, len(h)])
    x = rng.integers(lo, hi + 1, size=(n, 2), dtype=np.int64).astype(dtype)
    assert 0 <= n0 * D < n
    for k, hk in enumerate(np.asarray(h, dtype=np.int64)):
        m = n0 * D - k
        if m >= 0 and hk:
            x[m] = rail_for(hk, polarity, lo, hi)
    return x


def worst_case_acc(h, D: int, n0: int, polarity: int, lo: int = -32768, hi: int = 32767) -> int:
    """The bound the taps and the rails give output n0's accumulator: sum of h[k] (its rail) over the taps whose sample
    lies in the stream (n0 D - k >= 0).  Python integers."""
    return sum(int(hk) * rail_for(hk, polarity, lo, hi) for k, hk in enumerate(np.asarray(h, dtype=np.int64))
               if n0 * D - k >= 0)


WORST_D = (2, 7, 16)   # the factors of the accumulator leg


def worst_case_sets(seed: int = 4000):
    """(name, taps, shifts) of the accumulator leg: random taps of full weight, all positive, all negative, and the
    sets that hold the tap -32768."""
    rng = np.random.default_rng(seed)
    sets =[("random %d" % T, random_taps(rng, T), (0, 15, 16)) for T in (2, 17, 512)]
    sets.append(("positive", np.full(62, 65534 // 62, np.int16), (0, 15, 16)))       # 62 x 1057
    sets.append(("negative", np.full(434, -(65534 // 434), np.int16), (0, 15, 16)))  # 434 x -151
    sets.append(("-32768 32766", np.array([-32768, 32766], np.int16), (0, 15, 16)))
    sets.append(("-32768", np.array([-32768], np.int16), (0,)))
    sets.append(("32767 -32767", np.array([32767, -32767], np.int16), (0,)))
    return sets


def rail_u8_table() -> np.ndarray:
    """An 8-bit table that reaches both int16 rails, linear in between: T8[b] = 257 b - 32768."""
    t = (257 * np.arange(256, dtype=np.int64) - 32768).astype(np.int16)
    assert t[0] == -32768 and t[255] == 32767
    return t


def worst_case_outputs(D: int, tile: int):
    """(n0 of the accumulator leg, inputs of its streams): lane 0 and the last lane of the first tile, lane 0 of the
    second, and a lane of the ragged third of a stream of 2 tile + 37 outputs (its length no multiple of D)."""
    return (0, tile - 1, tile, 2 * tile + 20), (2 * tile + 36) * D + (1 if D == 2 else 2)


def decimate_window(x_window, first_output: int, count: int, h, D: int, s: int) -> np.ndarray:
    """Outputs first_output .. first_output + count - 1 of a stream from a window of its inputs: x_window[0] is input
    max(first_output D - (T - 1), 0) of the stream and the window reaches input (first_output + count - 1) D."""
    x = np.asarray(x_window, dtype=np.int64).reshape(-1, 2)
    h = np.asarray(h, dtype=np.int64)
    T = len(h)
    lo = max(first_output * D - (T - 1), 0)
    n = np.arange(first_output, first_output + count)
    assert count == 0 or lo + len(x) > n[-1] * D
    xp = np.concatenate([np.zeros((T - 1, 2), np.int64), x])   # xp[m - lo + T - 1] = x[m]
    acc = np.zeros((count, 2), np.int64)
    for k in range(T):
        idx = n * D - k - lo + T - 1
        assert (idx >= (T - 1 if lo > 0 else 0)).all()   # (behind a window that starts inside the stream: no padding)
        acc += h[k] * xp[idx]
    return _finish(acc, s)


def window_inputs(first_output: int, count: int, T: int, D: int):
    """[lo, hi): the inputs decimate_window needs for these outputs."""
    return max(first_output * D - (T - 1), 0), (first_output + count - 1) * D + 1


def tile_base(blk: int, first: int, D: int, T: int, tile: int) -> int:
    """The input index k_decim's tile `blk` puts its buffer resource at: the 8-sample boundary below (the first input the
    tile needs) - 8, or 0."""
    i0 = first + blk * tile * D - (T - 1)
    return max((i0 - 8) & ~7, 0)


def hamming_sinc_taps(D: int) -> np.ndarray:
    """What adsb_decim_default_taps describes -- 8 D + 1 taps of a Hamming-windowed sinc with its cutoff at 1.2 MHz,
    round(h * 32768) -- from numpy, so that an expectation built on it does not hang on the library's libm."""
    M = 8 * D
    i = np.arange(M + 1)
    w = np.sinc((i - M // 2) / D) * (0.54 - 0.46 * np.cos(2 * np.pi * i / M))
    return np.rint(w / w.sum() * 32768).astype(np.int16)

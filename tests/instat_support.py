"""The input statistics of a decimator, a resampler or a bank (include/adsb_hip.h, "Input statistics"), restated in
numpy from the definition: the record of a set of raw input samples in one of the four formats.  The conversion is
tests/formats_in_support.to_cs16; nothing here is taken from the library.  No GPU, no library.

    c[m] = (re, im)   the converted CS16 sample, before the mixer
    clipped           CS16 / REAL16: a component in {-32768, 32767}; 8-bit: a byte in {0, 255}; CF32: a component that is
                      not NaN and has q(x) in {-32768, 32767}
    NaN               CF32: a sample with a NaN component (its converted value 0 enters the sums and bin 0)
    hist              hist[bin(v)]++ for v = re and v = im (REAL16: re only); bin(0) = 0, else 1 + floor(log2 |v|)
"""
import numpy as np

from tests import formats_in_support as fi

CS16, U8, CF32, REAL16 = fi.CS16, fi.U8, fi.CF32, fi.REAL16
FORMATS = (CS16, U8, CF32, REAL16)
BINS = 17
# adsb_input_stats, field by field as the header spells it (208 bytes)
DTYPE = np.dtype([("n_samples", "<u8"), ("sum_re", "<i8"), ("sum_im", "<i8"), ("sum_re2", "<u8"), ("sum_im2", "<u8"),
                  ("sum_re_im", "<i8"), ("n_clipped", "<u8"), ("n_nan", "<u8"), ("hist", "<u8", (BINS,)), ("peak", "<u4"),
                  ("reserved", "<u4")])
assert DTYPE.itemsize == 208
RAILS = (-32768, 32767)


def input_bin(v) -> np.ndarray:
    """0 for v == 0, else 1 + floor(log2 |v|): 0 .. 16, -32768 in bin 16.  (log2 of an integer up to 2^15 in binary64:
    exact at the powers of two, and 2^k - 1 lies 4e-5 below k at the least.)"""
    a = np.abs(np.asarray(v).astype(np.int64))
    return np.where(a == 0, 0, 1 + np.floor(np.log2(np.maximum(a, 1)))).astype(np.int64)


def record(x, fmt: int, g: float = fi.DEFAULT_SCALE, table=None) -> np.ndarray:
    """The record of the samples x of one call (or of any set of samples) in `fmt`, as a 0-d array of DTYPE."""
    c = fi.to_cs16(x, fmt, g, table).astype(np.int64).reshape(-1, 2)
    n = len(c)
    re, im = c[:, 0], c[:, 1]
    out = np.zeros((), dtype=DTYPE)
    out["n_samples"] = n
    out["sum_re"], out["sum_im"] = int(re.sum()), int(im.sum())
    out["sum_re2"], out["sum_im2"] = int((re * re).sum()), int((im * im).sum())
    out["sum_re_im"] = int((re * im).sum())
    nan = np.zeros(n, dtype=bool)
    if fmt == U8:
        b = np.asarray(x).reshape(-1, 2)
        clipped = ((b == 0) | (b == 255)).any(axis=1)   # the bytes decide, not the table
    elif fmt == CF32:
        f = np.asarray(x).reshape(-1, 2)
        is_nan = np.isnan(f)
        clipped = (~is_nan & np.isin(c, RAILS)).any(axis=1)
        nan = is_nan.any(axis=1)
    elif fmt == REAL16:
        clipped = np.isin(re, RAILS)
    else:
        clipped = np.isin(c, RAILS).any(axis=1)
    out["n_clipped"], out["n_nan"] = int(clipped.sum()), int(nan.sum())
    comps = re if fmt == REAL16 else c.reshape(-1)
    out["hist"] = np.bincount(input_bin(comps), minlength=BINS)
    out["peak"] = int(np.abs(c).max()) if n else 0
    return out


def add(a, b) -> np.ndarray:
    """The record of the union of two disjoint sets of samples."""
    out = np.zeros((), dtype=DTYPE)
    for name in DTYPE.names:
        out[name] = np.maximum(a[name], b[name]) if name == "peak" else a[name] + b[name]
    return out


def empty() -> np.ndarray:
    return np.zeros((), dtype=DTYPE)


def same(got, want) -> bool:
    return np.asarray(got, dtype=DTYPE).tobytes() == np.asarray(want, dtype=DTYPE).tobytes()


def explain(got, want) -> str:
    return "; ".join(f"{n}: got {got[n].tolist()} want {want[n].tolist()}" for n in DTYPE.names if np.any(got[n] != want[n]))


def sprinkled(rng, fmt: int, n: int, g: float = fi.DEFAULT_SCALE):
    """n random samples in `fmt` with rails and zeros sprinkled in (CF32: NaN and the infinities too)."""
    k = max(1, n // 16)
    if n == 0:
        return rail_fill(fmt, 0)
    if fmt == CS16:
        x = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int64).astype(np.int16)
        x.reshape(-1)[rng.integers(0, 2 * n, size=k)] = rng.choice(np.array([-32768, 32767, 0, 1, -1], np.int16), size=k)
    elif fmt == U8:
        x = rng.integers(0, 256, size=(n, 2), dtype=np.int64).astype(np.uint8)
        x.reshape(-1)[rng.integers(0, 2 * n, size=k)] = rng.choice(np.array([0, 255, 127, 128], np.uint8), size=k)
    elif fmt == REAL16:
        x = rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
        x[rng.integers(0, n, size=k)] = rng.choice(np.array([-32768, 32767, 0, 1, -1], np.int16), size=k)
    else:
        x = (rng.standard_normal((n, 2)) * (12000.0 / g)).astype(np.float32)
        x.reshape(-1)[rng.integers(0, 2 * n, size=k)] = rng.choice(
            np.array([np.nan, np.inf, -np.inf, 0.0, 1e30, -1e30, 32767.0 / g, -32768.0 / g], np.float32), size=k)
    return x


def rail_fill(fmt: int, n: int):
    """n samples of what must never be counted: rail values (CF32: NaN)."""
    if fmt == CS16:
        return np.full((n, 2), -32768, np.int16)
    if fmt == U8:
        return np.full((n, 2), 255, np.uint8)
    if fmt == REAL16:
        return np.full(n, 32767, np.int16)
    return np.full((n, 2), np.nan, np.float32)

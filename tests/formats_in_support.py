"""The two sample formats a decimator or resampler converts on its way in (include/adsb_hip.h, "Sample formats"),
restated in numpy: q for CF32, the widening for REAL16.  The expected output of every test is this conversion followed
by the existing restatements (tests/decim_support.py, tests/resamp_support.py, tests/mix_support.py) -- never anything
taken from the library.  No GPU, no library.

    CF32    t = x * g in binary32;  q(x) = 0 where t is a NaN, else clamp(rint(t), -32768, 32767), ties to even
    REAL16  x[m] = (r[m], 0)
"""
import numpy as np

CS16, U8, CF32, REAL16 = 0, 1, 2, 3
DEFAULT_SCALE = 32768.0
G2 = float(np.float32(1000.1))   # a scale that is no power of two: 0x1.f40cccp+9


def q(x, g: float = DEFAULT_SCALE) -> np.ndarray:
    """float32 components of any shape -> int16, as the header's numpy line says."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    with np.errstate(all="ignore"):
        t = x * np.float32(g)
    assert t.dtype == np.float32
    r = np.where(np.isnan(t), np.float32(0), np.rint(t))
    return np.clip(r, -32768, 32767).astype(np.int16)


def q_exact(x: float, g: float) -> int:
    """q of one component by another road: the product of two binary32 numbers is exact in binary64, so one rounding
    to binary32 gives t; Python's round() is ties-to-even."""
    x, g = float(np.float32(x)), float(np.float32(g))
    if x != x:
        return 0
    if x in (float("inf"), float("-inf")):
        return 32767 if x > 0 else -32768
    with np.errstate(all="ignore"):
        t = float(np.float32(np.float64(x) * np.float64(g)))
    if t in (float("inf"), float("-inf")):
        return 32767 if t > 0 else -32768
    return int(min(max(round(t), -32768), 32767))


def real_to_cs16(r) -> np.ndarray:
    """(n,) int16 real samples -> (n, 2) int16 [r, 0]."""
    r = np.asarray(r)
    assert r.dtype == np.int16 and r.ndim == 1
    return np.ascontiguousarray(np.stack([r, np.zeros_like(r)], axis=1))


def to_cs16(x, fmt: int, g: float = DEFAULT_SCALE, table=None) -> np.ndarray:
    """A call's input in `fmt` -> the (n, 2) int16 samples that replace x[m] in the filters' definitions."""
    if fmt == CS16:
        return np.asarray(x, dtype=np.int16).reshape(-1, 2)
    if fmt == U8:
        return np.ascontiguousarray(np.asarray(table)[np.asarray(x).reshape(-1, 2)])
    if fmt == CF32:
        return q(np.asarray(x).reshape(-1, 2), g)
    assert fmt == REAL16
    return real_to_cs16(x)


def cs16_as_cf32(x, g: float = DEFAULT_SCALE) -> np.ndarray:
    """(n, 2) int16 -> (n, 2) float32 x / g, for a g that is a power of two: exact, and q brings x back."""
    f = (np.asarray(x, dtype=np.float32).reshape(-1, 2) / np.float32(g)).astype(np.float32)
    assert np.array_equal(q(f, g), np.asarray(x).reshape(-1, 2))
    return f


def real_carrier(x) -> np.ndarray:
    """The real stream r[4 n] = re x[n], r[4 n - 1] = im x[n], zeros elsewhere (4 len(x) - 3 samples, the last at
    4 (len(x) - 1)): through the exact table of -1/4 turn per sample (adsb_mix_table(3, 4)), D = 4, taps [1, 1] and
    shift 0 it decimates to x, except that im of sample 0 has no carrier."""
    x = np.asarray(x, dtype=np.int16).reshape(-1, 2)
    r = np.zeros(4 * len(x) - 3, np.int16)
    r[0::4] = x[:, 0]
    r[3::4] = x[1:, 1]
    return r


F32_MAX_SUBNORMAL = float.fromhex("0x1.fffffcp-127")
# (x, q at g = 32768, q at g = G2), spelled out.  Ties at 0.5, 1.5, 2.5 and 32767.5 LSB of both signs, for g = 32768 as
# k / 32768 and for G2 as the binary32 x whose product with G2 rounds to exactly k; then 1.0, NaN, the infinities, the
# zeros, the largest subnormal and 1e30.
Q_EDGES = [
    (0.5 / 32768, 0, 0), (-0.5 / 32768, 0, 0), (1.5 / 32768, 2, 0), (-1.5 / 32768, -2, 0),
    (2.5 / 32768, 2, 0), (-2.5 / 32768, -2, 0), (32767.5 / 32768, 32767, 1000), (-32767.5 / 32768, -32768, -1000),
    (float.fromhex("0x1.061e28p-11"), 16, 0), (float.fromhex("-0x1.061e28p-11"), -16, 0),           # x G2 = +-0.5
    (float.fromhex("0x1.892d3cp-10"), 49, 2), (float.fromhex("-0x1.892d3cp-10"), -49, -2),           # x G2 = +-1.5
    (float.fromhex("0x1.47a5b2p-9"), 82, 2), (float.fromhex("-0x1.47a5b2p-9"), -82, -2),             # x G2 = +-2.5
    (float.fromhex("0x1.061d22p+5"), 32767, 32767), (float.fromhex("-0x1.061d22p+5"), -32768, -32768),   # x G2 = +-32767.5
    (1.0, 32767, 1000), (-1.0, -32768, -1000),
    (float("nan"), 0, 0), (float("inf"), 32767, 32767), (float("-inf"), -32768, -32768),
    (0.0, 0, 0), (-0.0, 0, 0), (F32_MAX_SUBNORMAL, 0, 0), (-F32_MAX_SUBNORMAL, 0, 0), (1e30, 32767, 32767), (-1e30, -32768, -32768),
]


def edge_values() -> np.ndarray:
    return np.array([e[0] for e in Q_EDGES], dtype=np.float32)

"""What the signal-statistics tests share (include/adsb_hip.h, "Signal statistics"): the plain restatement of a
record, over the ORACLE's magnitudes and the raw input -- never the library's own adsb_to_mag."""
import numpy as np

CHUNK = 131072
FULL = 65535


def bin_of(m: int) -> int:
    """adsb_signal_bin as the header states it."""
    if m < 8:
        return m
    e = m.bit_length() - 1
    return 8 + 4 * (e - 3) + ((m >> (e - 2)) & 3)


BIN = np.array([bin_of(m) for m in range(65536)], dtype=np.int64)


def bin_edge(b: int) -> int:
    """The smallest magnitude of bin b."""
    return int(np.argmax(BIN == b))


def restated(orc, cs16: np.ndarray, raw: np.ndarray, dtype) -> np.ndarray:
    """One record per 131072-sample buffer of a call.  cs16: the (N, 2) int16 samples the call MEANS (CU8 widened);
    raw: what it was handed, (N, 2) int16 or uint8 -- the rails are counted on that."""
    n = len(cs16)
    out = np.zeros((n + CHUNK - 1) // CHUNK, dtype=dtype)
    lo, hi = (0, 255) if raw.dtype == np.uint8 else (-32768, 32767)
    for c in range(len(out)):
        seg, rseg = cs16[c * CHUNK:(c + 1) * CHUNK], raw[c * CHUNK:(c + 1) * CHUNK]
        data, length = orc.to_mag(seg)
        assert length == len(seg)
        m = data[326:326 + length].astype(np.uint64)
        r = out[c]
        r["chunk"], r["n_samples"] = c, length
        r["sum_power"] = int((m * m).sum())
        r["peak"] = int(m.max()) if length else 0
        r["n_strong"] = int((2 * m * m >= FULL * FULL).sum())
        r["n_clipped"] = int(((rseg == lo) | (rseg == hi)).any(axis=1).sum())
        r["hist"] = np.bincount(BIN[m.astype(np.int64)], minlength=60)
    return out


def summary_of(rec: np.ndarray) -> dict:
    """adsb_signal_summary's formulas in numpy float64."""
    n = int(rec["n_samples"].astype(np.uint64).sum())
    power = int(rec["sum_power"].astype(np.uint64).sum())
    peak = int(rec["peak"].max()) if len(rec) else 0
    hist = rec["hist"].astype(np.uint64).sum(axis=0) if len(rec) else np.zeros(60, np.uint64)
    edge = 0
    if n:
        b = int(np.searchsorted(np.cumsum(hist), (n + 1) // 2))
        edge = bin_edge(b)
    ninf = -np.inf
    return {
        "n_buffers": len(rec), "n_samples": n,
        "mean_power_dbfs": 10.0 * np.log10(np.float64(power) / np.float64(n) / (65535.0 * 65535.0)) if n and power else ninf,
        "peak_dbfs": 20.0 * np.log10(np.float64(peak) / 65535.0) if peak else ninf,
        "median_dbfs": 20.0 * np.log10(np.float64(edge) / 65535.0) if edge else ninf,
        "clipped_fraction": float(rec["n_clipped"].astype(np.uint64).sum()) / n if n else 0.0,
        "strong_fraction": float(rec["n_strong"].astype(np.uint64).sum()) / n if n else 0.0,
    }


def feed_line(s: dict, buffers: int) -> str:
    """adsb_feed --stats: the line it prints for a summary."""
    return ("buffers %d, floor %.3f dBFS, mean %.3f dBFS, peak %.3f dBFS, clipped %.6f %%, strong %.6f %%"
            % (buffers, s["median_dbfs"], s["mean_power_dbfs"], s["peak_dbfs"], 100.0 * s["clipped_fraction"],
               100.0 * s["strong_fraction"]))

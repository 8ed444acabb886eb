"""Streams and frames that sit exactly on the demodulator's integer decisions (src/demod_2400.rs:127-146, 215-321,
72-83), and a numpy model of those decisions written from the reference lines -- a second reading beside the oracle
that also counts how often each edge is reached.

  mag_inverse()      an (re, im) pair for every u16 magnitude the magnitude function can produce (all but 1 and 5)
  debruijn_stream()  a magnitude walk whose adjacent comparisons (<, =, >) are a de Bruijn sequence of order 13:
                     every comparison pattern of p0..p13 occurs
  alphabet_stream()  i.i.d. magnitudes from a small set: ties, 2*sig == 3*noise and loud == high in bulk
  catalogue()        clean DF17 bursts with p0..p18 or one slicer sample rewritten onto an edge, each with a twin one
                     unit away whose verdict is the opposite
  gates()/counters() the model: check_preamble's branch, the 3.5 dB and quiet gates, the fast scan's "<=" superset
                     branch and its tied pairs, and the slicer values of the sliced positions

Magnitudes are handled as the demodulator sees them: data[0:326] is the buffer's lead-in, sample k is data[326 + k],
a position j reads data[j .. j + 18] for its gates and data[j + 19 ..] for its bits."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from dump1090_rs_amd import synth

CHUNK = 131072
LEAD = 326
ORDER = 13
QUIET = (5, 6, 7, 8, 14, 15, 16, 17, 18)
SLICE_COEF = np.array([[5, -3, -2, 0], [4, -1, -3, 0], [3, 1, -4, 0], [2, 3, -5, 0], [1, 5, -5, -1]], dtype=np.int64)
# the five branches of check_preamble (:227, :242, :262, :280, :300) as (a, b) pairs meaning p[a] > p[b]
BRANCH_GT = [
    [(1, 2), (3, 2), (3, 4), (9, 8), (9, 10), (11, 10)],
    [(1, 2), (3, 2), (3, 4), (9, 8), (9, 10), (12, 11)],
    [(1, 2), (3, 2), (4, 5), (9, 8), (10, 11), (12, 11)],
    [(1, 2), (4, 3), (4, 5), (10, 9), (10, 11), (12, 11)],
    [(2, 3), (4, 3), (4, 5), (10, 9), (10, 11), (12, 11)],
]
# which of each branch's pairs are the reference's "<" (the fast scan's pattern stage has only ">" and takes "<="
# for these), as (low, high) sample indices: p0 < p1 (:221) and the branch's own three -- gate_eval's p1-p0, dx, dy, dz
LT_PAIRS = [
    [(0, 1), (2, 3), (8, 9), (10, 11)],
    [(0, 1), (2, 3), (8, 9), (11, 12)],
    [(0, 1), (2, 3), (8, 9), (11, 12)],
    [(0, 1), (3, 4), (9, 10), (11, 12)],
    [(0, 1), (3, 4), (9, 10), (11, 12)],
]
# high = sum(HIGH) / 4, base_signal = sum(SIG), base_noise = sum(NOISE)
HIGH = [(1, 3, 9, 11, 12), (1, 3, 9, 12), (1, 3, 4, 9, 10, 12), (1, 4, 10, 12), (1, 2, 4, 10, 12)]
SIG = [(1, 3, 9), (1, 3, 9, 12), (1, 12), (1, 4, 10, 12), (4, 10, 12)]
NOISE = [(5, 6, 7), (5, 6, 7, 8), (6, 7), (5, 6, 7, 8), (6, 7, 8)]


# ------------------------------------------------------------------------------------------- magnitude inverse
_INV: Optional[np.ndarray] = None


def _mags_of(pairs: np.ndarray) -> np.ndarray:
    """oracle to_mag of (N, 2) [re, im] pairs, in buffers."""
    from oracle import binding
    orc = binding.Oracle()
    out = []
    for a in range(0, len(pairs), CHUNK):
        part = np.ascontiguousarray(pairs[a:a + CHUNK], dtype=np.int16)
        data, n = orc.to_mag(part)
        out.append(data[LEAD:LEAD + n])
    return np.concatenate(out).astype(np.int64)


def mag_inverse() -> np.ndarray:
    """(65536, 2) int16 [re, im] with to_mag(re, im) == index; (-32768, -32768) marks the values no pair reaches.  On the axis (k, 0) gives 2k; the odd values come from off-axis pairs near radius
    m * 32768 / 65535."""
    global _INV
    if _INV is not None:
        return _INV
    inv = np.full((65536, 2), -32768, dtype=np.int16)
    found = np.zeros(65536, dtype=bool)

    def take(pairs):
        pairs = np.asarray(pairs, dtype=np.int64)
        ok = (pairs[:, 0] >= -32768) & (pairs[:, 0] <= 32767) & (pairs[:, 1] >= -32768) & (pairs[:, 1] <= 32767)
        pairs = pairs[ok]
        m = _mags_of(pairs)
        new = ~found[m]
        m, pairs = m[new], pairs[new]
        first = np.unique(m, return_index=True)[1]
        inv[m[first]] = pairs[first]
        found[m[first]] = True

    axis = np.concatenate([np.arange(0, 32768), np.arange(-32768, 0)])     # (k, 0) first: 2k
    take(np.stack([axis, np.zeros(65536, dtype=np.int64)], axis=1))
    g = np.arange(0, 48)
    take(np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2))
    want = np.nonzero(~found)[0]
    r = want.astype(np.float64) * 32768.0 / 65535.0
    for im in range(1, 256):
        re = np.sqrt(np.maximum(r * r - im * im, 0.0))
        base = np.floor(re).astype(np.int64)
        cand = np.concatenate([np.stack([base + d, np.full_like(base, im)], axis=1) for d in (-1, 0, 1, 2)])
        take(cand)
        if found.sum() >= 65534:
            break
    inv[~found] = -32768
    _INV = inv
    return inv


def reachable() -> np.ndarray:
    inv = mag_inverse()
    return ~((inv[:, 0] == -32768) & (inv[:, 1] == -32768))


def to_iq(mags: np.ndarray) -> np.ndarray:
    """(N, 2) int16 IQ whose magnitudes are `mags`; refuses a value no IQ pair reaches."""
    m = np.asarray(mags, dtype=np.int64)
    ok = reachable()
    if not ok[m].all():
        bad = np.unique(m[~ok[m]])
        raise ValueError(f"magnitudes no (re, im) pair reaches: {bad[:8].tolist()}")
    return np.ascontiguousarray(mag_inverse()[m])


# ------------------------------------------------------------------------------------------- streams
def debruijn(k: int, n: int) -> np.ndarray:
    """The lexicographically least cyclic de Bruijn sequence over 0..k-1 of order n (FKM algorithm)."""
    a = [0] * (k * n)
    seq: List[int] = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10 * n + 100))
    try:
        db(1, 1)
    finally:
        sys.setrecursionlimit(old)
    return np.array(seq, dtype=np.int8)


def comparison_sequence() -> np.ndarray:
    """The linear de Bruijn sequence over {0: "<", 1: "=", 2: ">"} of order 13: 3^13 + 12 symbols, every window of
    13 a different pattern."""
    s = debruijn(3, ORDER)
    return np.concatenate([s, s[:ORDER - 1]])


def walk(symbols: np.ndarray, seed: int = 13, centre: int = 16600) -> np.ndarray:
    """Magnitudes m with sign(m[i+1] - m[i]) given by symbols[i] ("<": up, "=": equal, ">": down).  Steps toward the
    centre are big, steps away from it 2, so the walk stays in range: the sequence's longest stretch without a "<" is
    8204 symbols, without a ">" 26.  All levels are even (on-axis IQ)."""
    r = np.random.default_rng(seed)
    small = np.full(len(symbols), 2)
    big = 2 * r.integers(2, 120, len(symbols))
    m = np.empty(len(symbols) + 1, dtype=np.int64)
    v = centre
    m[0] = v
    for i, s in enumerate(symbols.tolist()):
        if s == 0:
            v += big[i] if v < centre else small[i]
        elif s == 2:
            v -= big[i] if v > centre else small[i]
        m[i + 1] = v
    return m


def split_overlapping(m: np.ndarray, overlap: int = ORDER + 6) -> List[np.ndarray]:
    """Buffers of at most CHUNK samples, each repeating the last `overlap` samples of the one before, so that every
    window of p0..p18 lies whole inside one buffer."""
    out, a = [], 0
    while True:
        out.append(m[a:a + CHUNK])
        if a + CHUNK >= len(m):
            return out
        a += CHUNK - overlap


def debruijn_stream() -> Tuple[np.ndarray, np.ndarray]:
    """(magnitudes per buffer, concatenated (n_buffers * CHUNK) with the last buffer zero-padded; the comparison
    sequence)."""
    seq = comparison_sequence()
    parts = split_overlapping(walk(seq))
    m = np.zeros(len(parts) * CHUNK, dtype=np.int64)
    for k, p in enumerate(parts):
        m[k * CHUNK:k * CHUNK + len(p)] = p
    return m, seq


ALPHABETS = {
    "low": (0, 2, 4, 6),
    "wide": (0, 100, 150, 200, 300),
    "odd": (0, 3, 4, 7, 9, 10),                # odd magnitudes: off-axis IQ pairs
    "full": (0, 65530, 65533, 65534, 65535),   # full scale: 65533 / 65534 off-axis, 65535 = (-32768, 0)
    "caller": (0, 1, 5, 6),                    # no IQ pair reaches 1 or 5: caller magnitudes only
    "caller_full": (0, 1, 5, 65531, 65534, 65535),
}


def alphabet_stream(name: str, n_buffers: int, seed: int) -> np.ndarray:
    a = np.array(ALPHABETS[name], dtype=np.int64)
    return a[np.random.default_rng(seed).integers(0, len(a), n_buffers * CHUNK)]


STREAM_BUFFERS = {"low": 2, "wide": 2, "odd": 2, "full": 2}


def iq_stream(name: str) -> np.ndarray:
    """An IQ-domain stream by name: "debruijn", "catalogue" or "planted" (one buffer each; "planted" has the clean
    templates in front of the catalogue) or one of the IQ-reachable alphabets above."""
    if name == "debruijn":
        return to_iq(debruijn_stream()[0])
    if name == "catalogue":
        return to_iq(catalogue_mags(catalogue(), CHUNK)[0])
    if name == "planted":   # the clean templates first, so that a repair mode knows the aircraft, then the catalogue
        clean = [Case("clean", "clean", m, j0, f, tp, True) for m, f, j0, tp in templates()]
        return to_iq(catalogue_mags(clean + catalogue(), CHUNK)[0])
    return to_iq(alphabet_stream(name, STREAM_BUFFERS[name], seed=sorted(ALPHABETS).index(name) + 90))


def data_of(mags: np.ndarray, lead: Optional[np.ndarray] = None) -> np.ndarray:
    """The reference's MagnitudeBuffer.data (326 lead-in + up to 131072 samples + zeros) of one buffer."""
    from oracle.binding import MAG_DATA_LEN
    d = np.zeros(MAG_DATA_LEN, dtype=np.uint16)
    if lead is not None:
        d[:LEAD] = lead
    d[LEAD:LEAD + len(mags)] = mags
    return d


# ------------------------------------------------------------------------------------------- the model
def gates(d: np.ndarray, n: int) -> Dict[str, np.ndarray]:
    """The reference's decisions at positions 0..n-1 of data d, and the fast scan's "<=" superset branch:
      branch   first matching branch of check_preamble (0..4), -1 when it returns None (:215-321)
      snr, cand  ... passes 2*sig >= 3*noise (:129); ... and the quiet samples stay below high (:135-146)
      sup      the branch the pattern stage takes with "<=" for the reference's "<" (adsb_scan_fast_body.inc P3)
      tie      (n, 4) bool: which of sup's four "<" pairs are equal
      sup_pass the gates of branch sup computed as if its pairs were strict (gate_eval without its fallback)
    and high / sig / noise / hsum / loud of `branch` (of `sup` in the sup_* entries)."""
    p = [d[k:k + n].astype(np.int64) for k in range(19)]
    quick = (p[0] < p[1]) & (p[12] > p[13])
    sup_ok = (p[0] <= p[1]) & (p[12] > p[13])

    def conds(strict):
        out = []
        for b in range(5):
            c = np.ones(n, dtype=bool)
            lt = set(LT_PAIRS[b][1:])
            for hi, lo in BRANCH_GT[b]:
                if (lo, hi) in lt and not strict:
                    c &= p[hi] >= p[lo]
                else:
                    c &= p[hi] > p[lo]
            out.append(c)
        return out

    def first(cs, ok):
        br = np.full(n, -1, dtype=np.int64)
        for b in range(4, -1, -1):
            br[ok & cs[b]] = b
        return br

    branch = first(conds(True), quick)
    sup = first(conds(False), sup_ok)

    def values(br):
        hsum = np.zeros(n, dtype=np.int64)
        sig = np.zeros(n, dtype=np.int64)
        noise = np.zeros(n, dtype=np.int64)
        for b in range(5):
            w = br == b
            hsum[w] = sum(p[k][w] for k in HIGH[b])
            sig[w] = sum(p[k][w] for k in SIG[b])
            noise[w] = sum(p[k][w] for k in NOISE[b])
        return hsum, sig, noise

    loud = np.max(np.stack([p[k] for k in QUIET]), axis=0)
    hsum, sig, noise = values(branch)
    high = hsum // 4
    snr = (branch >= 0) & (2 * sig >= 3 * noise)
    cand = snr & (loud < high)
    shsum, ssig, snoise = values(sup)
    sup_pass = (sup >= 0) & (2 * ssig >= 3 * snoise) & (loud < shsum // 4)
    tie = np.zeros((n, 4), dtype=bool)
    for b in range(5):
        w = sup == b
        for i, (lo, hi) in enumerate(LT_PAIRS[b]):
            tie[w, i] = p[lo][w] == p[hi][w]
    return {"branch": branch, "snr": snr, "cand": cand, "high": high, "hsum": hsum, "sig": sig, "noise": noise,
            "loud": loud, "sup": sup, "tie": tie, "sup_pass": sup_pass, "sup_sig": ssig, "sup_noise": snoise,
            "sup_hsum": shsum}


def slice_values(d: np.ndarray, js: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(D, phase) of every bit of the five trials at each j: shape (len(js), 5, 112); bit = D > 0 (:72-83)."""
    js = np.asarray(js, dtype=np.int64)
    tp = np.arange(4, 9)[None, :, None]
    nb = np.arange(112)[None, None, :]
    pos = 5 * (js[:, None, None] + 19) + tp + 12 * nb
    s, ph = pos // 5, pos % 5
    c = SLICE_COEF[ph]
    dd = d.astype(np.int64)
    D = sum(c[..., k] * dd[s + k] for k in range(4))
    return D, ph


def bits_of(D: np.ndarray) -> bytes:
    """The 14 message bytes of one trial's 112 slicer values."""
    return np.packbits(D > 0).tobytes()


def stage_lists(d: np.ndarray, n: int, buf: int = 0) -> Dict[str, List[int]]:
    g = gates(d, n)
    f = lambda m: [buf << 32 | int(j) for j in np.nonzero(m)[0]]
    return {"preamble": f(g["branch"] >= 0), "snr": f(g["snr"]), "cand": f(g["cand"])}


COUNTER_KEYS = (["tie_flip_b%d_p%d" % (b, i) for b in range(5) for i in range(4)] +
                ["snr_eq_sliced", "snr_short1", "loud_eq_r0", "loud_eq_r1", "loud_eq_r2", "loud_eq_r3", "loud_m1"] +
                ["d0_ph%d" % ph for ph in range(5)] + ["d0_cand"])


def counters(d: np.ndarray, n: int) -> Dict[str, int]:
    """How often one buffer reaches each edge:
      tie_flip_b*_p*  the pattern stage's branch b with its "<" pair i tied, where that changes the verdict (the
                      positions gate_eval must hand to preamble_gates)
      snr_eq_sliced   2*sig == 3*noise at a position that is sliced;  snr_short1: 3*noise - 2*sig == 1 where the quiet
                      samples would pass
      loud_eq_r*      the loudest quiet sample == high (rejected) with the branch's sum % 4 == r;  loud_m1: == high - 1
      d0_ph*          slicer values D == 0 (bit 0, by "> 0") of the sliced positions' trials, per slicer phase;
                      d0_cand: sliced positions with at least one"""
    g = gates(d, n)
    out = {k: 0 for k in COUNTER_KEYS}
    flip = g["sup_pass"] != g["cand"]
    for b in range(5):
        for i in range(4):
            out["tie_flip_b%d_p%d" % (b, i)] = int((flip & (g["sup"] == b) & g["tie"][:, i]).sum())
    q = g["loud"] < g["high"]
    out["snr_eq_sliced"] = int((g["cand"] & (2 * g["sig"] == 3 * g["noise"])).sum())
    out["snr_short1"] = int(((g["branch"] >= 0) & q & (3 * g["noise"] - 2 * g["sig"] == 1)).sum())
    for r in range(4):
        out["loud_eq_r%d" % r] = int((g["snr"] & (g["loud"] == g["high"]) & (g["hsum"] % 4 == r)).sum())
    out["loud_m1"] = int((g["snr"] & (g["loud"] == g["high"] - 1)).sum())
    js = np.nonzero(g["cand"])[0]
    if len(js):
        D, ph = slice_values(d, js)
        z = D == 0
        for k in range(5):
            out["d0_ph%d" % k] = int((z & (ph == k)).sum())
        out["d0_cand"] = int(z.any(axis=(1, 2)).sum())
    return out


def add_counters(a: Dict[str, int], b: Dict[str, int]) -> Dict[str, int]:
    return {k: a.get(k, 0) + b.get(k, 0) for k in COUNTER_KEYS}


# ------------------------------------------------------------------------------------------- edge-frame catalogue
ICAO = 0x4CA2D6
SPACING = 420            # samples per catalogue slot: the burst (~300) and a quiet stretch
FIRST = 600


@dataclass
class Case:
    name: str
    kind: str             # "tie", "snr_eq", "snr_short1", "loud", "p12_p13", "slice"
    mags: np.ndarray      # the slot's magnitudes (SPACING samples)
    j0: int               # the edge position (sample index of p0 inside the slot)
    frame: bytes          # the DF17 the slot carries
    tp: int               # its trial phase
    passes: bool          # the model's verdict: the gates let j0 through and (slicer cases) the frame decodes
    twin: int = -1        # index of the twin in the catalogue


def _template(me: int, tick: int) -> Tuple[np.ndarray, bytes, int, int]:
    """A zero-noise DF17 in a slot: (magnitudes, frame, j0, try_phase) with j0 the preamble position the oracle
    finds (one frame, from the sample index j0 of the slot)."""
    from oracle import binding
    frame = synth.df17_frame(ICAO, me)
    iq = np.zeros((SPACING, 2), dtype=np.int16)
    synth.add_bursts(iq, [synth.Burst(tick=tick, amplitude=14000, angle=0, frame=frame)])
    orc = binding.Oracle()
    orc.icao_flush()
    data, n = orc.to_mag(iq)
    got, _ = orc.demodulate2400(data, n)
    hits = [w for w in got if w["buffer"] == frame]
    assert len(hits) == 1, (me, tick, [w["j"] for w in got])
    return data[LEAD:LEAD + SPACING].astype(np.int64), frame, hits[0]["j"] - LEAD, hits[0]["try_phase"]


def _verdict(P: np.ndarray) -> Dict[str, np.ndarray]:
    """gates() of rows of p0..p18 (one position per row)."""
    P = np.atleast_2d(P)
    # one position per row: lay the rows out with 19 zeros between them so that they do not interact
    flat = np.zeros(P.shape[0] * 40, dtype=np.int64)
    idx = np.arange(P.shape[0]) * 40
    for k in range(19):
        flat[idx + k] = P[:, k]
    g = gates(flat.astype(np.uint16), len(flat) - 19)
    return {k: v[idx] for k, v in g.items()}


def _random_rows(r, b: int, n: int, hi=(24000, 34000), lo=(500, 6000)) -> np.ndarray:
    """n random p0..p18 with branch b's peaks high and everything else low (even values)."""
    peaks = set(SIG[b]) | set(HIGH[b])
    P = 2 * r.integers(lo[0] // 2, lo[1] // 2, (n, 19))
    for k in peaks:
        P[:, k] = 2 * r.integers(hi[0] // 2, hi[1] // 2, n)
    return P


def _pick(r, b: int, make, accept, tries: int = 4000):
    """Random rows of branch b, transformed by make(P) -> (case rows, twin rows), the first pair accept()s."""
    for _ in range(20):
        P = _random_rows(r, b, tries)
        A, B = make(P.copy())
        ga, gb = _verdict(A), _verdict(B)
        ok = accept(A, B, ga, gb) & (A >= 0).all(1) & (B >= 0).all(1) & (A <= 65535).all(1) & (B <= 65535).all(1)
        ok &= ~np.isin(A, (1, 5)).any(1) & ~np.isin(B, (1, 5)).any(1)
        w = np.nonzero(ok)[0]
        if len(w):
            return A[w[0]], B[w[0]]
    raise AssertionError("no row found")


def _preamble_pairs(seed: int) -> List[Tuple[str, str, np.ndarray, np.ndarray]]:
    """(name, kind, rows that pass, twin rows that do not -- or the reverse for the rejected edge cases)."""
    r = np.random.default_rng(seed)
    out = []
    for b in range(5):
        for i, (lo, hi) in enumerate(LT_PAIRS[b]):
            def make(P, lo=lo, hi=hi):
                A = P.copy()
                up = np.arange(len(A)) % 2 == 0  # move the low end up or the high end down
                A[up, lo] = A[up, hi] - 1        # strict by one unit
                A[~up, hi] = A[~up, lo] + 1
                B = A.copy()
                B[up, lo] = B[up, hi]            # tied
                B[~up, hi] = B[~up, lo]
                return A, B

            def accept(A, B, ga, gb, b=b, i=i):
                # A: branch b, sliced; B: the pattern stage still takes b, its gates alone would pass, the
                # reference rejects
                return ((ga["branch"] == b) & ga["cand"] & (gb["sup"] == b) & gb["tie"][:, i] & gb["sup_pass"]
                        & ~gb["cand"])
            A, B = _pick(r, b, make, accept)
            out.append(("b%d_tie%d" % (b, i), "tie", A, B))
        # 2*sig == 3*noise (sliced) and noise + 1 (rejected)
        def make_eq(P, b=b, short=0):
            adj = SIG[b][-1]
            for _ in range(3):                   # 2*sig + short divisible by 3
                s = sum(P[:, k] for k in SIG[b])
                bad = (2 * s + short) % 3 != 0
                P[bad, adj] += 1
            s = sum(P[:, k] for k in SIG[b])
            t = (2 * s + short) // 3             # the noise wanted, spread over the branch's noise samples
            nz = NOISE[b]
            for i, k in enumerate(nz):
                P[:, k] = t // len(nz) + (i < t % len(nz))
            A = P.copy()
            B = P.copy()
            if short:
                B[:, adj] += 1                   # sig + 1: passes
            else:
                B[:, 7] += 1                     # noise + 1: fails
            return A, B

        def acc_eq(A, B, ga, gb, b=b):
            return ((ga["branch"] == b) & ga["cand"] & (2 * ga["sig"] == 3 * ga["noise"]) & (gb["branch"] == b)
                    & ~gb["snr"] & (gb["loud"] < gb["high"]))
        A, B = _pick(r, b, make_eq, acc_eq)
        out.append(("b%d_snr_eq" % b, "snr_eq", A, B))

        def acc_short(A, B, ga, gb, b=b):
            return ((ga["branch"] == b) & ~ga["snr"] & (3 * ga["noise"] - 2 * ga["sig"] == 1) & (ga["loud"] < ga["high"])
                    & (gb["branch"] == b) & gb["cand"])
        A, B = _pick(r, b, lambda P, b=b: make_eq(P, b, short=1), acc_short)
        out.append(("b%d_snr_short1" % b, "snr_short1", A, B))
        # loud == high (rejected) with sum % 4 == res, twin loud == high - 1 (sliced); the loud sample cycles
        for res in range(4):
            q = (14, 15, 16, 17, 18, 8, 5)[(4 * b + res) % 7]

            def make_loud(P, b=b, res=res, q=q):
                for _ in range(4):
                    s = sum(P[:, k] for k in HIGH[b])
                    P[s % 4 != res, 12] += 1
                high = sum(P[:, k] for k in HIGH[b]) // 4
                A = P.copy()
                A[:, q] = high
                B = A.copy()
                B[:, q] = high - 1
                return A, B

            def acc_loud(A, B, ga, gb, b=b, res=res, q=q):
                return ((ga["branch"] == b) & ga["snr"] & (ga["loud"] == ga["high"]) & (ga["hsum"] % 4 == res)
                        & (gb["branch"] == b) & gb["cand"] & (gb["loud"] == gb["high"] - 1))
            A, B = _pick(r, b, make_loud, acc_loud)
            out.append(("b%d_loud_r%d" % (b, res), "loud", A, B))
        # p12 == p13 fails the quick test (:221); p13 = p12 - 1 passes
        def make_q(P):
            A = P.copy()
            A[:, 13] = A[:, 12]
            B = A.copy()
            B[:, 13] -= 1
            return A, B
        A, B = _pick(r, b, make_q, lambda A, B, ga, gb, b=b: (ga["branch"] < 0) & (gb["branch"] == b) & gb["cand"])
        out.append(("b%d_p12_p13" % b, "p12_p13", A, B))
    return out


def _slicer_pairs(tmpl: np.ndarray, frame: bytes, j0: int, tp: int):
    """For each slicer phase and each wanted bit value: a copy of the template with one sample moved so that one bit
    of the winning trial has D == 0 (sliced as 0) and every other bit of that trial keeps its value, and the twin
    with that sample one unit further (D != 0, sliced as 1).  The frame decodes in the copy iff its bit is 0."""
    d = np.zeros(LEAD + SPACING + 8, dtype=np.int64)
    d[LEAD:LEAD + SPACING] = tmpl
    j = LEAD + j0
    want_bits = np.unpackbits(np.frombuffer(frame, dtype=np.uint8))
    out = []
    for ph in range(5):
        for bit in (0, 1):
            done = False
            for n in range(8, 112):            # (bits 0..4 are the DF: leave them alone)
                pos = 5 * (j + 19) + tp + 12 * n
                s, p = pos // 5, pos % 5
                if p != ph or want_bits[n] != bit:
                    continue
                c = SLICE_COEF[ph]
                for k in range(4 if ph == 4 else 3):
                    D = int(sum(c[i] * d[s + i] for i in range(4)))
                    rest = D - c[k] * d[s + k]
                    if rest % c[k]:
                        continue
                    v = -rest // c[k]
                    for twin_v in (v + 1, v - 1):
                        if not (0 <= v <= 65535 and 0 <= twin_v <= 65535) or v in (1, 5) or twin_v in (1, 5):
                            continue
                        e, f = d.copy(), d.copy()
                        e[s + k], f[s + k] = v, twin_v
                        Ae = slice_values(e.astype(np.uint16), np.array([j]))[0][0]
                        Af = slice_values(f.astype(np.uint16), np.array([j]))[0][0]
                        De, Df = Ae[tp - 4], Af[tp - 4]
                        be, bf = (De > 0).astype(np.uint8), (Df > 0).astype(np.uint8)
                        others = np.arange(112) != n
                        if De[n] != 0 or bf[n] != 1 or not (np.array_equal(be[others], want_bits[others])
                                                             and np.array_equal(bf[others], want_bits[others])):
                            continue
                        # no other trial phase may carry the frame past the edge
                        dec_e = any(bits_of(Ae[t]) == frame for t in range(5))
                        dec_f = any(bits_of(Af[t]) == frame for t in range(5))
                        if dec_e != (bit == 0) or dec_f != (bit == 1):
                            continue
                        # the preamble gates must be untouched by the moved sample
                        ge, gf = gates(e.astype(np.uint16), j + 1), gates(f.astype(np.uint16), j + 1)
                        if not (ge["cand"][j] and gf["cand"][j]):
                            continue
                        out.append(("ph%d_bit%d_n%d" % (ph, bit, n), e[LEAD:LEAD + SPACING], f[LEAD:LEAD + SPACING],
                                    bit == 0))
                        done = True
                        break
                    if done:
                        break
                if done:
                    break
    return out


_CAT: Optional[List[Case]] = None
_TMPL = None


def templates():
    """The five clean DF17 slots the catalogue starts from (one per tick offset), as (mags, frame, j0, try_phase)."""
    global _TMPL
    if _TMPL is None:
        r = np.random.default_rng(4711)
        _TMPL = [_template(int(r.integers(0, 1 << 56)), 5 * 40 + t) for t in range(5)]
    return _TMPL


def catalogue() -> List[Case]:
    """Every edge case and its twin, one slot each (twins adjacent, twin = index ^ 1)."""
    global _CAT
    if _CAT is not None:
        return _CAT
    cases: List[Case] = []
    tmpls = templates()
    for k, (name, kind, A, B) in enumerate(_preamble_pairs(2024)):
        m, frame, j0, tp = tmpls[k % 5]
        for tag, P in (("", A), ("/twin", B)):
            mm = m.copy()
            mm[j0:j0 + 19] = P
            passes = bool(_verdict(P)["cand"][0])
            cases.append(Case(name + tag, kind, mm, j0, frame, tp, passes))
    # one or two slicer pairs per (phase, bit), from the templates where the edge decides the frame at every trial phase
    per: Dict[str, int] = {}
    for m, frame, j0, tp in tmpls:
        for name, e, f, dec in _slicer_pairs(m, frame, j0, tp):
            key = name.rsplit("_n", 1)[0]
            if per.get(key, 0) == 2:
                continue
            per[key] = per.get(key, 0) + 1
            cases.append(Case("tp%d_%s" % (tp, name), "slice", e, j0, frame, tp, dec))
            cases.append(Case("tp%d_%s/twin" % (tp, name), "slice", f, j0, frame, tp, not dec))
    assert sorted(per) == ["ph%d_bit%d" % (ph, b) for ph in range(5) for b in (0, 1)], per
    for i, c in enumerate(cases):
        c.twin = i ^ 1
    _CAT = cases
    return cases


def catalogue_mags(cases: List[Case], n_samples: int, first: int = FIRST, starts: Optional[List[int]] = None):
    """Magnitudes of a stream of n_samples with the cases' slots laid out from `first` (or at `starts`), and the
    sample index of each case's p0."""
    m = np.zeros(n_samples, dtype=np.int64)
    at = []
    for i, c in enumerate(cases):
        a = starts[i] if starts is not None else first + i * SPACING
        assert a + SPACING <= n_samples
        m[a:a + SPACING] = c.mags
        at.append(a + c.j0)
    return m, at

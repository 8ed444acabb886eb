"""Shared by the tests of every Mode S downlink format and score class (tests/test_formats_cpu.py,
tests/test_gpu_formats.py, tests/fuzz_gpu.py --formats): frame builders for every DF, a stream that puts every score
branch of the reference (src/mode_s/mod.rs:33-139) into every buffer, and a small Python model of
score_modes_message with the reference filter (src/icao_filter.rs), written from the reference and nothing else --
a second reading of the score table, independent of the oracle's and the library's."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from dump1090_rs_amd import synth

CHUNK = 131072
TILE = 7712                    # positions per tile of the scan (csrc/adsb_scan_geometry.h)
LEAD = 326                     # the magnitude buffer's lead-in: a burst starting at sample s has its preamble at j = s + 325..326
SPAN = 290                     # samples a 112-bit burst covers (8 + 112 us at 2.4 MHz), rounded up
AP_SHORT = (0, 4, 5)
AP_LONG = (16, 20, 21)
COMM_D = tuple(range(24, 32))
UNDEFINED = (1, 2, 3, 6, 7, 8, 9, 10, 12, 13, 14, 15, 19, 22, 23)
ADSB_NT = 1 << 25


# ----------------------------------------------------------------------------------------------- frame builders
def with_parity(body: bytes, residual: int) -> bytes:
    """`body` (4 or 11 bytes) and a parity field that leaves `residual` as its CRC residual."""
    return body + (synth.crc24(body) ^ residual).to_bytes(3, "big")


def ap_frame(df: int, addr: int, payload: int = 0) -> bytes:
    """An address/parity reply (DF 0/4/5/16/20/21/24-31, or any other DF): parity = CRC xor `addr`.  DF >= 16 is
    112 bits.  `payload` fills the three spare bits of the first byte and the body."""
    n = 11 if df & 0x10 else 4
    rest = (payload & ((1 << (8 * (n - 1))) - 1)).to_bytes(n - 1, "big")
    return with_parity(bytes([(df << 3) | ((payload >> 61) & 7)]) + rest, addr)


def df11_frame(addr: int, iid: int = 0, ca: int = 5, bad_pi: int = 0) -> bytes:
    """An all-call reply with interrogator id `iid` (the residual's low 7 bits); `bad_pi` (a multiple of 0x80, non-zero)
    corrupts the PI above the IID bits."""
    assert 0 <= iid < 128 and bad_pi & 0x7F == 0
    return with_parity(bytes([(11 << 3) | (ca & 7)]) + addr.to_bytes(3, "big"), iid | bad_pi)


def es_frame(df: int, addr: int, me: int, ca: int = 5) -> bytes:
    """A clean extended squitter, DF17 or DF18, with CA / CF `ca`."""
    assert df in (17, 18)
    return with_parity(bytes([(df << 3) | (ca & 7)]) + addr.to_bytes(3, "big") + (me & ((1 << 56) - 1)).to_bytes(7, "big"), 0)


def undefined_frame(df: int, addr: int, payload: int = 0) -> bytes:
    """A DF the reference scores -2 whatever its parity (mod.rs:136), with parity that would match `addr`."""
    assert df in UNDEFINED
    return ap_frame(df, addr, payload)


ZERO14 = bytes(14)                                    # all 14 sliced bytes zero: None (mod.rs:51)
ZERO7_TAIL = bytes(7) + bytes([0xA5, 0x5A, 0x3C, 0xC3, 0x0F, 0xF0, 0x99])   # DF0, residual 0, not all zero: 1000


def flip(frame: bytes, *bits: int) -> bytes:
    f = bytearray(frame)
    for b in bits:
        f[b >> 3] ^= 0x80 >> (b & 7)
    return bytes(f)


def fold(a: int) -> int:
    """The folded superset's index of a 24-bit value (contexts of <= 16 buffers, csrc/adsb_device.h)."""
    return (a ^ (a >> 19)) & ((1 << 19) - 1)


def folds_onto(k: int, d: int) -> int:
    """A value other than `k` that folds onto `k`'s bit (0 < d < 32)."""
    assert 0 < d < 32
    v = k ^ (d << 19) ^ d
    assert v != k and fold(v) == fold(k)
    return v


# ----------------------------------------------------------------------------------------------- the Python model
def crc_residual(msg: bytes, nbits: int) -> int:
    """src/crc.rs:263-282 over the first nbits / 8 bytes (bitwise, not the table)."""
    n = nbits // 8
    rem = 0
    for byte in msg[: n - 3]:
        rem ^= byte << 16
        for _ in range(8):
            rem = ((rem << 1) ^ 0xFFF409) & 0xFFFFFF if rem & 0x800000 else (rem << 1) & 0xFFFFFF
    return rem ^ int.from_bytes(msg[n - 3:n], "big")


def icao_hash(a: int) -> int:
    """src/icao_filter.rs:19-43"""
    h = 0
    for k in range(3):
        h += (a >> (8 * k)) & 0xFF
        h += h << 10
        h &= (1 << 64) - 1
        h ^= h >> 6
    h += h << 3
    h &= (1 << 64) - 1
    h ^= h >> 11
    h += h << 15
    h &= (1 << 64) - 1
    return h & 4095


class PyFilter:
    """src/icao_filter.rs: table A of 4096 slots, linear probing; table B is only ever flushed (all zero)."""

    def __init__(self):
        self.a = [0] * 4096

    def add(self, addr: int) -> None:          # :46-62
        h0 = h = icao_hash(addr)
        while self.a[h] != 0 and self.a[h] != addr:
            h = (h + 1) & 4095
            if h == h0:
                return                         # "icao24 hash table full"
        if self.a[h] == 0:
            self.a[h] = addr

    @staticmethod
    def _probe(t, addr: int) -> bool:
        h0 = h = icao_hash(addr)
        while t[h] != 0 and t[h] != addr:
            h = (h + 1) & 4095
            if h == h0:
                break
        return t[h] == addr

    def test(self, addr: int) -> bool:         # :65-97 (table B: an empty slot equals 0)
        return self._probe(self.a, addr) or addr == 0


def getbits(msg: bytes, first: int, last: int) -> int:
    """src/mode_s/mod.rs:14-30, bits numbered from 1"""
    v = 0
    for b in range(first - 1, last):
        v = (v << 1) | ((msg[b >> 3] >> (7 - (b & 7))) & 1)
    return v


def score_modes_message(f: PyFilter, msg: bytes) -> Optional[Tuple[int, int]]:
    """src/mode_s/mod.rs:33-139 on a 14-byte slice: None, or (length in bytes, score); mutates `f` like the reference."""
    if len(msg) < 7:
        return None
    df = getbits(msg, 1, 5)
    nbits = 112 if df & 0x10 else 56
    if len(msg) * 8 < nbits or not any(msg):
        return None
    if df in (0, 4, 5):
        res = 1000 if f.test(crc_residual(msg, nbits)) else -1
    elif df == 11:
        crc = crc_residual(msg, nbits)
        iid, crc = crc & 0x7F, crc & 0xFFFF80
        addr = getbits(msg, 9, 32)
        known = f.test(addr)
        if crc != 0:
            res = -2
        elif iid == 0 and known:
            res = 1600
        elif iid == 0:
            f.add(addr)
            res = 750
        else:
            res = 1000 if known else -1
    elif df in (17, 18):
        addr = getbits(msg, 9, 32)
        crc = crc_residual(msg, nbits)
        if crc != 0:
            res = -2
        elif f.test(addr):
            res = 1800
        else:
            f.add(addr if df == 17 else addr | ADSB_NT)
            res = 1400
    elif df in AP_LONG or df >= 24:
        res = 1000 if f.test(crc_residual(msg, 112)) else -2
    else:
        res = -2
    return nbits // 8, res


def model_demod(trials: np.ndarray, f: Optional[PyFilter] = None) -> List[tuple]:
    """src/demod_2400.rs:149-207 over the oracle's trials (oracle.binding.all_trials records of consecutive buffers,
    (chunk, j, try_phase) order), scored by the model: strictly greater wins from -2, emitted when >= 0.
    [(chunk, j, try_phase, score, bytes)]."""
    f = f if f is not None else PyFilter()
    out = []
    i, n = 0, len(trials)
    while i < n:
        pos = (int(trials[i]["chunk"]), int(trials[i]["j_tp"]) & 0xFFFFFF)
        best = None
        best_score = -2
        while i < n and (int(trials[i]["chunk"]), int(trials[i]["j_tp"]) & 0xFFFFFF) == pos:
            msg = bytes(trials[i]["msg"])
            tp = int(trials[i]["j_tp"]) >> 24
            i += 1
            s = score_modes_message(f, msg)
            if s is not None and s[1] > best_score:
                best, best_score = (tp, msg[: s[0]]), s[1]
        if best is not None and best_score >= 0:
            out.append((pos[0], pos[1], best[0], best_score, best[1]))
    return out


# ----------------------------------------------------------------------------------------------- the formats stream
@dataclass
class Event:
    buffer: int          # the buffer the burst starts in
    sample: int          # first sample of the burst (absolute)
    tick: int
    amplitude: int
    frame: bytes         # what is transmitted
    emits: bytes         # what an emission of it carries (buffer(): 7 or 14 bytes; a repaired copy: the clean frame)
    cls: str             # the class (CLASSES)
    addr: int            # the aircraft (or the residual an AP frame carries)
    whole: bool = True   # the burst lies inside its buffer (a reference-semantics pass can decode it)
    expect: Tuple[int, ...] = ()   # scores its first emission may have (model, plan order); () = never emitted


# class -> (DF set or None, minimum per buffer).  The plan puts at least that many of each into every buffer.
CLASSES: Dict[str, int] = {
    "df17_new": 4, "df17_known": 4, "df18_only": 8, "df18_known": 8, "df18_before_df17": 3, "df17_after_df18": 3,
    "df18_after_df17": 3, "df11_iid0_new": 3, "df11_iid0_known": 3, "df11_iid_known": 6, "df11_iid_unknown": 4,
    "df11_bad_pi": 3, "ap_short_known": 6, "ap_long_known": 6, "comm_d_known": 6, "ap_short_unknown": 3,
    "ap_long_unknown": 3, "comm_d_unknown": 3, "ap_of_df18_only": 6, "undefined": len(UNDEFINED), "residual0_short": 3,
    "residual0_long": 3, "zero14": 1, "zero7_tail": 1, "folded": 6,
}
# ... and in fix mode
FIX_CLASSES: Dict[str, int] = {"damaged_df18_known": 6, "damaged_df17_known": 3, "damaged_df18_only": 4,
                               "damaged_before_clean": 3, "damaged_two_bits": 3}
AMPLITUDES = (20000, 23000, 26000, 28500, 31000)


class _Draw:
    def __init__(self, seed: int):
        self.r = np.random.default_rng([0xF0E1, seed])

    def addr(self, used: set) -> int:
        while True:
            a = int(self.r.integers(1, 1 << 24))
            # (and nothing that folds onto an address already drawn: the folded values below are the only such)
            if a not in used and fold(a) not in {fold(u) for u in used}:
                used.add(a)
                return a

    def u(self, bits: int) -> int:
        return int(self.r.integers(0, 1 << 62)) >> (62 - bits) if bits <= 62 else \
            (int(self.r.integers(0, 1 << 62)) << (bits - 62)) | int(self.r.integers(0, 1 << (bits - 62)))

    def pick(self, seq):
        return seq[int(self.r.integers(0, len(seq)))]


def _buffer_plan(d: _Draw, used: set, fix: bool, extra=()) -> List[Tuple[str, int, bytes, bytes, int]]:
    """One buffer's events in transmission order (aircraft of its own, so every buffer holds every class whatever
    came before): (class, aircraft, frame, emitted bytes, group)."""
    seqs: List[List[Tuple[str, int, bytes, bytes]]] = []   # per aircraft, in order

    def es(df, a):
        f = es_frame(df, a, d.u(56), ca=d.pick(range(8)))
        return f

    def ap(df, a):
        f = ap_frame(df, a, d.u(64))
        return f[:7] if len(f) == 7 else f

    # heard by DF17
    for k in range(4):
        a = d.addr(used)
        s = [("df17_new", a, es(17, a)), ("df17_known", a, es(17, a)), ("df18_known", a, es(18, a)),
             ("df11_iid0_known", a, df11_frame(a, 0, ca=d.pick(range(8))))]
        s += [("df11_iid_known", a, df11_frame(a, 1 + int(d.r.integers(0, 127)))),
              ("ap_short_known", a, ap(d.pick(AP_SHORT), a)), ("ap_long_known", a, ap(d.pick(AP_LONG), a)),
              ("comm_d_known", a, ap(d.pick(COMM_D), a)), ("comm_d_known", a, ap(d.pick(COMM_D), a))]
        if k < 2:
            s += [("folded", folds_onto(a, 1 + int(d.r.integers(0, 31))), None)]
        if fix:
            bit = 5 + int(d.r.integers(0, 107))
            s.insert(0, ("damaged_before_clean", a, flip(es(18, a), bit)))
            s += [("damaged_df18_known", a, None), ("damaged_df17_known", a, None)]
        seqs.append(s)
    # heard by DF11 with IID 0 only
    for k in range(3):
        a = d.addr(used)
        s = [("df11_iid0_new", a, df11_frame(a, 0)), ("df11_iid0_known", a, df11_frame(a, 0)), ("df18_known", a, es(18, a)),
             ("df18_known", a, es(18, a)), ("df11_iid_known", a, df11_frame(a, 1 + int(d.r.integers(0, 127)))),
             ("df11_bad_pi", a, df11_frame(a, int(d.r.integers(0, 128)), bad_pi=0x80 << int(d.r.integers(0, 17)))),
             ("ap_short_known", a, ap(d.pick(AP_SHORT), a)), ("ap_long_known", a, ap(d.pick(AP_LONG), a)),
             ("comm_d_known", a, ap(d.pick(COMM_D), a))]
        if k < 2:
            s += [("folded", folds_onto(a, 1 + int(d.r.integers(0, 31))), None)]
        if fix:
            s += [("damaged_df18_known", a, None), ("damaged_two_bits", a, None)]
        seqs.append(s)
    # heard only by DF18 (and their address/parity replies, which must never score)
    for k in range(4):
        a = d.addr(used)
        s = [("df18_only", a, es(18, a)), ("df18_only", a, es(18, a)), ("ap_of_df18_only", a, ap(d.pick(AP_SHORT), a)),
             ("ap_of_df18_only", a, ap(d.pick(AP_LONG + COMM_D), a)), ("df11_iid_unknown", a, df11_frame(a, 1 + k))]
        if k < 2:
            s += [("folded", folds_onto(a, 1 + int(d.r.integers(0, 31))), None)]
        if fix:
            s += [("damaged_df18_only", a, None)]
        seqs.append(s)
    # DF18 before and after the DF17 of the same aircraft
    for k in range(3):
        a = d.addr(used)
        seqs.append([("df18_before_df17", a, es(18, a)), ("df17_after_df18", a, es(17, a)), ("df18_after_df17", a, es(18, a)),
                     ("ap_short_known", a, ap(d.pick(AP_SHORT), a))])
    # never heard cleanly
    for k in range(3):
        a = d.addr(used)
        s = [("ap_short_unknown", a, ap(d.pick(AP_SHORT), a)), ("ap_long_unknown", a, ap(d.pick(AP_LONG), a)),
             ("comm_d_unknown", a, ap(d.pick(COMM_D), a)), ("df11_iid_unknown", a, df11_frame(a, 100 + k))]
        if fix:
            s.insert(0, ("damaged_before_clean", a, flip(es(17, a), 5 + int(d.r.integers(0, 107)))))
        seqs.append(s)
    # undefined DFs (parity that would match an address heard by DF17), residual 0, the two zero edges
    anyone = seqs[0][0][1]
    for df in UNDEFINED:
        seqs.append([("undefined", anyone, undefined_frame(df, anyone, d.u(64)))])
    for df in (0, 4, 5):
        seqs.append([("residual0_short", 0, ap(df, 0))])
    for df in (16, 20, d.pick(COMM_D)):
        seqs.append([("residual0_long", 0, ap(df, 0))])
    seqs.append([("zero14", 0, ZERO14)])
    seqs.append([("zero7_tail", 0, ZERO7_TAIL)])
    seqs += [list(x) for x in extra]

    # the folded values and damaged copies are built now that the aircraft's clean frames exist
    out_seqs = []
    for s in seqs:
        clean18 = [f for c, _, f in s if f is not None and f[0] >> 3 == 18 and c != "damaged_before_clean"]
        clean17 = [f for c, _, f in s if f is not None and f[0] >> 3 == 17 and c != "damaged_before_clean"]
        o = []
        for c, a, f in s:
            if c == "folded":
                f = ap(d.pick(AP_SHORT + AP_LONG + COMM_D), a)
            elif c in ("damaged_df18_known", "damaged_df18_only"):
                good = clean18[0] if clean18 else es(18, a)
                f = (flip(good, 5 + int(d.r.integers(0, 107))), good)
            elif c == "damaged_df17_known":
                good = clean17[0]
                f = (flip(good, 5 + int(d.r.integers(0, 107))), good)
            elif c == "damaged_two_bits":
                good = clean18[0]
                b1 = 5 + int(d.r.integers(0, 106))
                f = (flip(good, b1, b1 + 1 + int(d.r.integers(0, 111 - b1))), good)
            o.append((c, a, f))
        out_seqs.append(o)
    # interleave the aircraft at random, each one's frames in its own order
    keys = [sorted(d.r.random(len(s)).tolist()) for s in out_seqs]
    for g, s in enumerate(out_seqs):
        if s[0][0] == "damaged_before_clean":   # ... right in front of the first clean frame: same tile, same pass
            keys[g][1] = keys[g][0] + 1e-12
    flat = [(keys[g][i], g, i) for g, s in enumerate(out_seqs) for i in range(len(s))]
    flat.sort()
    events = []
    for _, g, i in flat:
        c, a, f = out_seqs[g][i]
        frame, emits = (f if isinstance(f, tuple) else (f, None))
        if emits is None:
            emits = frame[:7] if frame[0] & 0x80 == 0 else frame
        events.append((c, a, frame, emits, g))
    return events


def formats_capture(seed: int, n_buffers: int, fix: bool = False, edges: bool = True, noise_seed: Optional[int] = None,
                    extra=None):
    """`n_buffers` buffers of noise, each with every class of CLASSES (and FIX_CLASSES when `fix`: damaged copies of
    DF17 / DF18), bursts not overlapping, over every tick % 5 and several amplitudes.  Frames are put across tile seams
    (preamble a few samples in front of a multiple of 7712 positions), at the first samples of a buffer and, when
    `edges`, across each buffer's end (a DF17 of an aircraft of its own each; whole=False: not held to the plan, the
    oracle decides).  Returns (iq, events in time order)."""
    d = _Draw(seed)
    used: set = set()
    iq = synth.noise_numpy(n_buffers * CHUNK, seed=noise_seed if noise_seed is not None else 0xF0A7 + seed)
    events: List[Event] = []
    bursts = []
    k = 0
    for b in range(n_buffers):
        plan = _buffer_plan(d, used, fix, extra(b) if extra else ())
        lo, hi = b * CHUNK + SPAN + 40 + int(d.r.integers(0, 3)), (b + 1) * CHUNK - (SPAN + 200 if edges else SPAN + 2)
        gap = (hi - lo) // len(plan)
        assert gap >= SPAN + 60, gap
        seams = [b * CHUNK + TILE * t - LEAD - int(d.r.integers(0, 250)) for t in range(1, 18)]
        seams = [s for s in seams if lo < s < hi - SPAN]
        pos = []
        for i in range(len(plan)):
            s = lo + i * gap + (int(d.r.integers(0, gap - SPAN - 40)) if i else 0)
            # a seam inside this slot: put the burst there
            for t in seams:
                if lo + i * gap < t <= lo + (i + 1) * gap - SPAN - 40 and i:
                    s = t
            pos.append(s)
        for (c, a, frame, emits, g), s in zip(plan, pos):
            tick = 5 * s + (k % 5)
            amp = AMPLITUDES[k % len(AMPLITUDES)] + int(d.r.integers(0, 500))
            k += 1
            bursts.append(synth.Burst(tick, amp, k % 16, frame))
            events.append(Event(b, s, tick, amp, frame, emits, c, a))
        # the first samples of the buffer, and across its end
        # (the first samples only where no burst comes across the edge from the buffer before)
        first = [b * CHUNK + int(d.r.integers(0, 3))] if b == 0 or not edges else []
        for s in first + ([(b + 1) * CHUNK - int(d.r.integers(60, 200))] if edges else []):
            a = d.addr(used)
            frame = es_frame(17, a, d.u(56))
            tick = 5 * s + (k % 5)
            k += 1
            bursts.append(synth.Burst(tick, 20000, k % 16, frame))
            events.append(Event(b, s, tick, 20000, frame, frame, "edge", a, whole=False))
    synth.add_bursts(iq, bursts)
    _expect(events)
    return iq, events


def _expect(events: List[Event]) -> None:
    """The model over the plan, in time order: the scores each burst's first emission may have.  A burst is sliced by
    up to five phases at one j and they are scored in turn, so a first DF17 can win at 1800 (phase 4 added the
    address, phase 5 finds it) and a first DF11 IID 0 at 1600; a DF18 cannot: it adds addr | 1 << 25 and asks for
    the plain address.  Damaged copies are scored with single-bit repair (1200 when the plain address is known)."""
    f = PyFilter()
    for e in events:
        if not e.whole:
            continue
        if e.cls.startswith("damaged"):
            a = e.addr
            e.expect = (1200,) if e.cls != "damaged_two_bits" and f.test(a) and a != 0 else ()
            continue
        s = score_modes_message(f, e.frame if len(e.frame) == 14 else e.frame + bytes(7))
        if e.cls == "zero7_tail":
            s = score_modes_message(f, e.frame)
        if s is None or s[1] < 0:
            e.expect = ()
        elif s[1] == 1400 and e.frame[0] >> 3 == 17:
            e.expect = (1400, 1800)
        elif s[1] == 750:
            e.expect = (750, 1600)
        else:
            e.expect = (s[1],)


def emitted_df(msg: bytes) -> int:
    return msg[0] >> 3


def class_counts(events: List[Event]) -> Dict[str, int]:
    out: Dict[str, int] = {}
    for e in events:
        out[e.cls] = out.get(e.cls, 0) + 1
    return out


def assert_classes(events: List[Event], n_buffers: int, fix: bool = False) -> None:
    """Every class of the plan, at least its minimum in every buffer (what a test's input must contain)."""
    need = dict(CLASSES, **(FIX_CLASSES if fix else {}))
    for b in range(n_buffers):
        got = class_counts([e for e in events if e.buffer == b and e.whole])
        short = {c: (got.get(c, 0), m) for c, m in need.items() if got.get(c, 0) < m}
        assert not short, (b, short)
    # the expected scores the classes stand for
    by = {}
    for e in events:
        if e.whole:
            by.setdefault(e.cls, set()).add(e.expect)
    assert by["df18_only"] == {(1400,)} and by["df18_known"] == {(1800,)} and by["df18_before_df17"] == {(1400,)}
    assert by["df17_after_df18"] == {(1400, 1800)} and by["df18_after_df17"] == {(1800,)}
    assert by["df11_iid_known"] == {(1000,)} and by["comm_d_known"] == {(1000,)} and by["residual0_long"] == {(1000,)}
    for c in ("ap_of_df18_only", "df11_iid_unknown", "df11_bad_pi", "undefined", "folded", "zero14",
              "ap_short_unknown", "ap_long_unknown", "comm_d_unknown"):
        assert by[c] == {()}, c
    if fix:
        assert by["damaged_df18_known"] == {(1200,)} and by["damaged_df18_only"] == {()}
        assert by["damaged_before_clean"] == {()} and by["damaged_two_bits"] == {()}


def first_emissions(events: List[Event], msgs: List[tuple], carry: bool = False) -> Dict[int, Optional[tuple]]:
    """{event index: the first emission of its bytes within two samples of its preamble, or None}.  `msgs`: keys
    (bytes, score, j, try_phase, chunk, ...) of fix_support.okey / key.  With `carry`, a buffer's j counts from the
    carried samples in front of it, as it does without."""
    at: Dict[Tuple[bytes, int], List[tuple]] = {}
    for m in msgs:
        g = m[4] * CHUNK + m[2] - LEAD
        at.setdefault(m[0], []).append((g, m))
    out = {}
    for i, e in enumerate(events):
        hits = [m for g, m in at.get(e.emits, []) if e.sample - 2 <= g <= e.sample + 2]
        out[i] = hits[0] if hits else None
    return out


def cross_pass(n_passes: int, per_pass: int, seed: int = 0, first_pass: int = 0):
    """`extra` for formats_capture: aircraft heard across passes of `per_pass` buffers in both orders -- X by DF18 in
    even passes and by DF17 (then DF18 and an address/parity reply) in odd ones, Y the other way round."""
    r = np.random.default_rng([0xC055, seed])
    xs = [0xC00000 + int(v) for v in r.integers(0, 1 << 18, size=4)]
    ys = [0xD00000 + int(v) for v in r.integers(0, 1 << 18, size=4)]

    def extra(b):
        p = first_pass + b // per_pass
        if b % per_pass != per_pass - 1:
            return []
        out = []
        for a in xs:
            me = int(r.integers(0, 1 << 56))
            out.append([("x_df18", a, es_frame(18, a, me))] if p % 2 == 0 else
                       [("x_df17", a, es_frame(17, a, me)), ("x_df18", a, es_frame(18, a, me + 1)), ("x_ap", a, ap_frame(20, a, me))])
        for a in ys:
            me = int(r.integers(0, 1 << 56))
            out.append([("y_df17", a, es_frame(17, a, me)), ("y_ap", a, ap_frame(4, a, me))] if p % 2 == 0 else
                       [("y_df18", a, es_frame(18, a, me)), ("y_ap", a, ap_frame(24 + p % 8, a, me))])
        return out
    return extra


def packed_buffer(seed: int, noise_seed: int = 77) -> np.ndarray:
    """One buffer of back-to-back frames of every class (three buffers' plans at 300-sample spacing): more hits than a
    buffer's bucket of 1024 holds on a dense stream."""
    d = _Draw(seed)
    used: set = set()
    plan = [x for _ in range(3) for x in _buffer_plan(d, used, False)]
    iq = synth.noise_numpy(CHUNK, seed=noise_seed)
    n = min(len(plan), (CHUNK - 400) // 300)
    synth.add_bursts(iq, [synth.Burst(5 * (200 + 300 * q) + q % 5, AMPLITUDES[q % 5], q % 16, plan[q][2]) for q in range(n)])
    return iq


def fill_capture(seed: int, n_buffers: int, per_buffer: int = 80) -> np.ndarray:
    """A dense stream of thousands of distinct aircraft: new DF17 and new DF18-only ones, a second DF18 of recent
    DF18-only ones, address/parity replies and all-call replies of recent DF17 ones and of recent DF18-only ones, and
    residual-0 replies -- enough new addresses to fill the 4096-slot table and go on past it."""
    d = _Draw(seed)
    iq = synth.noise_numpy(n_buffers * CHUNK, seed=0xF111 + seed)
    bursts = []
    d17, d18 = [], []
    gap = (CHUNK - 400) // per_buffer
    for b in range(n_buffers):
        for q in range(per_buffer):
            kind = q % 8
            a = 0x100000 + int(d.r.integers(0, 0xE00000))
            if kind in (0, 3):
                d17.append(a)
                f = es_frame(17, a, d.u(56))
            elif kind in (1, 5):
                d18.append(a)
                f = es_frame(18, a, d.u(56))
            elif kind == 2 and d18:
                a = d18[-1 - int(d.r.integers(0, min(len(d18), 30)))]
                f = es_frame(18, a, d.u(56)) if q % 16 == 2 else ap_frame(d.pick(AP_SHORT + AP_LONG + COMM_D), a, d.u(64))
            elif kind == 4 and d17:
                a = d17[-1 - int(d.r.integers(0, min(len(d17), 30)))]
                f = ap_frame(d.pick(AP_SHORT + AP_LONG + COMM_D), a, d.u(64)) if q % 16 == 4 else df11_frame(a, 1 + q % 127)
            elif kind == 6:
                f = ap_frame(d.pick(AP_SHORT + AP_LONG + COMM_D), 0, d.u(64))
            else:
                f = df11_frame(a, 0)
            s = b * CHUNK + 200 + q * gap + int(d.r.integers(0, gap - SPAN - 20))
            bursts.append(synth.Burst(5 * s + q % 5, AMPLITUDES[(q + b) % 5], (q + b) % 16, f))
    synth.add_bursts(iq, bursts)
    return iq

"""Shared by the tests of two-bit repair (ADSB_FIX_2BIT): the CPU restatement (tests/fix2_restatement.c, compiled here
against oracle/liboracle.so into a temporary directory) and a stream that holds every two-bit copy of a known DF17."""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from dump1090_rs_amd import synth
from tests import fix_support as fs

ROOT = Path(__file__).resolve().parent.parent
CHUNK = fs.CHUNK
FIX2 = 3
FIRST, SPACING = 2000, 700
PER_BUFFER = (CHUNK - 400 - FIRST) // SPACING + 1   # burst slots a buffer holds (the last ends well before its edge)
PAIRS = [(a, b) for a in range(5, 112) for b in range(a + 1, 112)]
_restate = None


def restatement() -> C.CDLL:
    """The restatement library (built once per process)."""
    global _restate
    if _restate is None:
        from oracle import binding
        binding.build()
        out = Path(tempfile.mkdtemp(prefix="fix2_restatement_")) / "libfix2_restatement.so"
        subprocess.run(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-I", str(ROOT / "oracle"),
                        str(ROOT / "tests" / "fix2_restatement.c"), "-o", str(out), str(binding.LIB_PATH),
                        "-Wl,-rpath," + str(binding.LIB_PATH.parent)], check=True, capture_output=True, timeout=120)
        L = C.CDLL(str(out))
        vp, sz = C.c_void_p, C.c_size_t
        L.fix2_demod_iq.argtypes = [vp, vp, sz, C.c_int, vp, vp, sz]
        L.fix2_demod_iq.restype = sz
        L.fix2_demodulate2400.argtypes = [vp, vp, C.c_int, vp, sz]
        L.fix2_demodulate2400.restype = sz
        L.fix2_pair_syndromes.argtypes = [vp]
        _restate = L
    return _restate


class Restated(fs.Restated):
    """fix_support.Restated in modes 0, 1 and 3, through the two-bit restatement."""

    def demod_iq(self, iq) -> list:
        from oracle import binding
        a = np.ascontiguousarray(iq, dtype=np.int16)
        cap = max(4096, a.shape[0] // 16)
        out = (binding.OrcMsg * cap)()
        n = restatement().fix2_demod_iq(C.byref(self.filter), a.ctypes.data, a.shape[0], self.mode,
                                        None if self.carry is None else self.carry.ctypes.data, out, cap)
        assert n <= cap
        return [fs.okey(m) for m in out[:n]]

    def demodulate2400(self, data: np.ndarray, length: int) -> list:
        from oracle import binding
        mb = binding.OrcMagBuf()
        C.memmove(mb.data, np.ascontiguousarray(data, dtype=np.uint16).ctypes.data, 2 * binding.MAG_DATA_LEN)
        mb.length = length
        out = (binding.OrcMsg * 65536)()
        n = restatement().fix2_demodulate2400(C.byref(self.filter), C.byref(mb), self.mode, out, 65536)
        return [fs.okey(m) for m in out[:n]]


def flip2(frame: bytes, a: int, b: int) -> bytes:
    return fs.flip(fs.flip(frame, a), b)


def pair_stream(seed: int = 8100, pairs=None, extras: bool = True):
    """Buffers of noise, PER_BUFFER burst slots each, SPACING samples apart from FIRST on: a clean DF17 from each of
    fix_support.KNOWN, then (extras) every single-bit copy of KNOWN[1]'s, two-bit copies of DF17s from
    fix_support.UNKNOWN and two-bit copies of KNOWN[2]'s that touch the DF bits 0..4 (one of them, bits 3 and 4, a DF18),
    then every pair of `pairs`
    (default: all 5671) flipped in KNOWN[0]'s clean frame.
    Returns (iq, {slot: (kind, clean frame)}) with slot = buffer * PER_BUFFER + index, kind "clean", "1bit", "2bit",
    "unknown" or "df"."""
    pairs = PAIRS if pairs is None else pairs
    clean = {a: synth.df17_frame(a, 0x58C382D690C8AC + 0x1000 * i) for i, a in enumerate(fs.KNOWN)}
    frames = [("clean", clean[a], clean[a]) for a in fs.KNOWN]
    if extras:
        good = clean[fs.KNOWN[1]]
        frames += [("1bit", fs.flip(good, b), good) for b in range(5, 112)]
        for k, a in enumerate(fs.UNKNOWN):
            f = synth.df17_frame(a, 0x77 + k)
            frames.append(("unknown", flip2(f, 12 + k, 60 + 5 * k), f))
        good = clean[fs.KNOWN[2]]
        # (a single flipped DF bit takes DF17 out of the DF17/18 branch; (3, 4) makes it DF18, whose residual is then
        # syn(3) ^ syn(4): a pair the table must not hold)
        frames += [("df", flip2(good, a, b), good) for a in range(5) for b in (7, 30, 70, 111)] + [("df", flip2(good, 3, 4), good)]
    good = clean[fs.KNOWN[0]]
    frames += [("2bit", flip2(good, a, b), good) for a, b in pairs]
    n_buf = (len(frames) + PER_BUFFER - 1) // PER_BUFFER
    iq = np.concatenate([synth.noise_numpy(CHUNK, seed + k) for k in range(n_buf)])
    bursts, want = [], {}
    for slot, (kind, frame, good) in enumerate(frames):
        t = (slot // PER_BUFFER) * CHUNK + FIRST + SPACING * (slot % PER_BUFFER)
        bursts.append(synth.Burst(5 * t + (slot % 5), 21000 + 97 * (slot % 50), slot % 16, frame))
        want[slot] = (kind, good)
    synth.add_bursts(iq, bursts)
    return iq, want


def slot_of(k) -> int:
    """the burst slot of pair_stream a message key (fix_support.key / okey) sits at"""
    j = k[2] + CHUNK * k[4]
    buf, off = divmod(j, CHUNK)
    return buf * PER_BUFFER + int(round((off - FIRST) / SPACING))


def repaired(keys: list, score: int) -> dict:
    """{slot: the bytes of every message with this score there}; a slot holds at most two (neighbouring j)"""
    out, counts = {}, {}
    for k in keys:
        if k[1] != score:
            continue
        s = slot_of(k)
        assert out.setdefault(s, k[0]) == k[0], s
        counts[s] = counts.get(s, 0) + 1
    assert max(counts.values(), default=0) <= 2, counts
    return out


def check_pair_stream(got: list, want: dict) -> None:
    """every two-bit copy came back repaired with the clean bytes, every one-bit copy as 1200, nothing else was
    repaired: the unknown addresses and the pairs touching the DF bits are not.  A two-bit copy comes back as 1100,
    or -- a handful in the 5671, where the noise lets another trial phase slice one of the two bits right -- as 1200,
    which the best of five prefers."""
    two = {s: g for s, (kind, g) in want.items() if kind == "2bit"}
    r2, r1 = repaired(got, 1100), repaired(got, 1200)
    assert set(r2) <= set(two) and all(r2[s] == two[s] for s in r2)
    assert {s: g for s, g in r1.items() if s not in two} == {s: g for s, (kind, g) in want.items() if kind == "1bit"}
    assert {**{s: g for s, g in r1.items() if s in two}, **r2} == two
    assert len(r2) >= 0.99 * len(two)

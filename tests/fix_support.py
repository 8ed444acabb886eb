"""Shared by the tests of single-bit repair (ADSB_FIX_1BIT): the CPU restatement (tests/fix_restatement.c, compiled
here against oracle/liboracle.so into a temporary directory), a capture of damaged DF17s, and message keys."""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from dump1090_rs_amd import synth

ROOT = Path(__file__).resolve().parent.parent
CHUNK = 131072
_restate = None


def restatement() -> C.CDLL:
    """The restatement library (built once per process)."""
    global _restate
    if _restate is None:
        from oracle import binding
        binding.build()
        out = Path(tempfile.mkdtemp(prefix="fix_restatement_")) / "libfix_restatement.so"
        subprocess.run(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-I", str(ROOT / "oracle"),
                        str(ROOT / "tests" / "fix_restatement.c"), "-o", str(out), str(binding.LIB_PATH),
                        "-Wl,-rpath," + str(binding.LIB_PATH.parent)], check=True, capture_output=True, timeout=120)
        L = C.CDLL(str(out))
        vp, sz = C.c_void_p, C.c_size_t
        L.fix_demod_iq.argtypes = [vp, vp, sz, C.c_int, vp, vp, sz]
        L.fix_demod_iq.restype = sz
        L.fix_demodulate2400.argtypes = [vp, vp, C.c_int, vp, sz]
        L.fix_demodulate2400.restype = sz
        L.fix_syndrome_table.argtypes = [vp]
        _restate = L
    return _restate


class Restated:
    """One stream through the restatement: the filter (and, with carry-over, the last 326 samples) persist across
    calls, as on a context."""

    def __init__(self, mode: int, carry: bool = False):
        from oracle import binding
        self.mode = mode
        self.filter = binding.OrcFilter()
        self.carry = np.zeros(2 * 326, dtype=np.int16) if carry else None

    def icao_flush(self):
        from oracle import binding
        self.filter = binding.OrcFilter()

    def demod_iq(self, iq) -> list:
        from oracle import binding
        a = np.ascontiguousarray(iq, dtype=np.int16)
        cap = max(4096, a.shape[0] // 16)
        out = (binding.OrcMsg * cap)()
        n = restatement().fix_demod_iq(C.byref(self.filter), a.ctypes.data, a.shape[0], self.mode,
                                       None if self.carry is None else self.carry.ctypes.data, out, cap)
        assert n <= cap
        return [okey(m) for m in out[:n]]

    def demodulate2400(self, data: np.ndarray, length: int) -> list:
        from oracle import binding
        mb = binding.OrcMagBuf()
        C.memmove(mb.data, np.ascontiguousarray(data, dtype=np.uint16).ctypes.data, 2 * binding.MAG_DATA_LEN)
        mb.length = length
        out = (binding.OrcMsg * 65536)()
        n = restatement().fix_demodulate2400(C.byref(self.filter), C.byref(mb), self.mode, out, 65536)
        return [okey(m) for m in out[:n]]


def okey(m) -> tuple:
    """(buffer bytes, score, j, try_phase, chunk, signal_level) of an oracle message"""
    return (bytes(m.msg[: m.len]), int(m.score), int(m.j), int(m.try_phase), int(m.chunk), float(m.signal_level))


def key(m) -> tuple:
    """... of a library message (ModeSMessage)"""
    return (m.buffer(), int(m.score), int(m.j), int(m.try_phase), int(m.chunk), float(m.signal_level))


def flip(frame: bytes, b: int) -> bytes:
    f = bytearray(frame)
    f[b >> 3] ^= 0x80 >> (b & 7)
    return bytes(f)


KNOWN = [0xA1B2C3, 0x4840D6, 0x3C6589, 0x06A0AF]
UNKNOWN = [0x7C0001 + 0x111 * k for k in range(8)]


def repaired_by_slot(fixed: list, mode0: list, spacing: int = 700) -> dict:
    """{burst slot of damaged_capture: the bytes repaired there} from the score-1200 keys of a run and the keys of a mode-0
    run (its first message is the first clean frame, slot 0).  A frame can be repaired at two neighbouring positions
    j, j + 1 (both slice it with the one bad bit): a slot holds at most two, always the same bytes."""
    j0 = mode0[0][2] + CHUNK * mode0[0][4]
    out = {}
    for k in fixed:
        slot = (k[2] + CHUNK * k[4] - j0 + spacing // 2) // spacing
        assert out.setdefault(slot, k[0]) == k[0], slot
    counts = {}
    for k in fixed:
        slot = (k[2] + CHUNK * k[4] - j0 + spacing // 2) // spacing
        counts[slot] = counts.get(slot, 0) + 1
    assert max(counts.values(), default=0) <= 2, counts
    return out


def damaged_capture(seed: int = 7001, n_samples: int = CHUNK, first: int = 2000, spacing: int = 700):
    """Noise with: a clean DF17 from each KNOWN aircraft, then a copy with exactly one bit flipped for every bit
    0..111 (aircraft b % 4), then damaged DF17s (bit 40 + k) from UNKNOWN addresses never heard cleanly.
    Returns (iq, clean frames by bit, {bit: clean frame} of the repairable copies)."""
    iq = synth.noise_numpy(n_samples, seed)
    bursts, repairable = [], {}
    t = first

    def put(frame, k):
        nonlocal t
        bursts.append(synth.Burst(5 * t + (k % 5), 21000 + 97 * (k % 50), k % 16, frame))
        t += spacing

    clean = {a: synth.df17_frame(a, 0x58C382D690C8AC + 0x1000 * i) for i, a in enumerate(KNOWN)}
    for i, a in enumerate(KNOWN):
        put(clean[a], i)
    for b in range(112):
        good = clean[KNOWN[b % 4]]
        put(flip(good, b), b)
        if b >= 5:
            repairable[b] = good
    for k, a in enumerate(UNKNOWN):
        put(flip(synth.df17_frame(a, 0x99 + k), 40 + k), 200 + k)
    assert 5 * t < 5 * n_samples - 2000
    synth.add_bursts(iq, bursts)
    return iq, clean, repairable

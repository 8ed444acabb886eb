"""Shared by tests/test_score_rounds_cpu.py and tests/test_gpu_score_rounds.py: the four fixed sizes that govern device-side
ordering and scoring, restated (csrc/adsb_scan_fast.hip: kHitCap; csrc/adsb_device.h: kTileBucket, kOrderBucket,
kScoreBlocks; csrc/adsb_context.cpp: ScoreDev::cap), the arithmetic of the score grid (csrc/adsb_score_dev.h: score_body /
emit_body), and streams on an all-zero background whose passes leave an EXACT number of hits: frames written as small
patches, each patch's own record count measured once on the device (only to compose inputs; what the passes over those
inputs return is judged against the CPU oracle), subsets chosen so that the counts sum to the target.

Geometry.  A tile is TILE = 7712 preamble positions j of a buffer (17 per buffer, the last one 7680); a burst whose first
sample is s has its preamble at j = s + 325..326 (LEAD), so a tile's frames start at tile * TILE - LEAD + 80 + 320 q,
q = 0 .. 22: 320 samples apart (a 112-bit burst covers 290), every trial of a frame inside the tile."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from dump1090_rs_amd import synth
from tests import formats_support as F

CHUNK = F.CHUNK
TILE = F.TILE
LEAD = F.LEAD
TILES_PER_CHUNK = -(-CHUNK // TILE)          # 17 (fastgeo::kTilesPerChunk)
HIT_CAP = 32                                 # kHitCap: hits a tile stages in LDS
TILE_BUCKET = 56                             # kTileBucket: places in a tile's sub-bucket of order_tmp
ORDER_BUCKET = 1024                          # kOrderBucket: places in a buffer's bucket
SCORE_BLOCKS = 256                           # kScoreBlocks: blocks of k_score / k_emit ...
SCORE_THREADS = 256                          # ... and their threads (launch_score: the same number)
SCORE_CAP_MAX = 262144
SLOT = 320                                   # samples between two frames of a tile
SLOTS_PER_TILE = 23
SLOT_FIRST = 80


# ------------------------------------------------------------------------------------ the arithmetic, restated
def score_cap(max_chunks: int) -> int:
    """ScoreDev::cap of a context created for `max_chunks` buffers: the most hits a pass may have to be scored on the device."""
    return min(4096 + 1024 * max_chunks, SCORE_CAP_MAX)


def per_block(n: int) -> int:
    """hits block b of the score grid owns: [b * per, min(n, (b + 1) * per))"""
    return -(-n // SCORE_BLOCKS)


def rounds(n: int) -> int:
    """rounds of emit_body's loop in a full block (SCORE_THREADS hits a round)"""
    return -(-per_block(n) // SCORE_THREADS)


def boundaries(n: int) -> List[int]:
    """Every index i in (0, n) at which hit i starts another block of the score grid or another round of its block."""
    per = per_block(n)
    out = set()
    for b in range(SCORE_BLOCKS):
        first, last = b * per, min(n, (b + 1) * per)
        out.update(range(first, last, SCORE_THREADS))
    return sorted(i for i in out if 0 < i < n)


def straddling_groups(pos: np.ndarray, n: Optional[int] = None) -> List[Tuple[int, int, int]]:
    """`pos`: the position (buffer << 24 | j) of every hit of a pass in device order, ascending.  -> (boundary, first
    index, last index) of every group of two or more trials of one position that has hits on both sides of a block or
    round boundary of the score grid."""
    pos = np.asarray(pos, dtype=np.uint64)
    n = len(pos) if n is None else n
    assert n == len(pos) and (n < 2 or bool(np.all(pos[1:] >= pos[:-1])))
    out = []
    for m in boundaries(n):
        if pos[m - 1] == pos[m]:
            g0, g1 = m - 1, m
            while g0 > 0 and pos[g0 - 1] == pos[m]:
                g0 -= 1
            while g1 + 1 < n and pos[g1 + 1] == pos[m]:
                g1 += 1
            out.append((m, g0, g1))
    return out


# ------------------------------------------------------------------------------------ subset sums
def choose(counts: Sequence[int], target: int) -> Optional[List[int]]:
    """indices of a subset of `counts` that sums to `target` (subset sum), or None"""
    reach: Dict[int, List[int]] = {0: []}
    for i, r in enumerate(counts):
        if r <= 0:
            continue
        for s, idx in list(reach.items()):
            if s + r <= target and s + r not in reach:
                reach[s + r] = idx + [i]
        if target in reach:
            return reach[target]
    return reach.get(target)


def choose_slots(options: Sequence[Sequence[Tuple[int, int, object]]], accept: Callable[[int, int], bool],
                 limit: int = TILE_BUCKET + 8) -> Optional[List[object]]:
    """One tile: options[q] = the patches that can stand in slot q as (scan hits, match hits, id); at most one per slot.
    -> the ids of a selection whose sums (scan, match) satisfy `accept`, scan + match <= limit; or None."""
    reach: Dict[Tuple[int, int], List[object]] = {(0, 0): []}
    for opts in options:
        for (s, m), ids in list(reach.items()):
            for ds, dm, ident in opts:
                k = (s + ds, m + dm)
                if ds + dm > 0 and k[0] + k[1] <= limit and k not in reach:
                    reach[k] = ids + [ident]
    for (s, m), ids in sorted(reach.items(), key=lambda kv: (len(kv[1]), kv[0])):
        if accept(s, m):
            return ids
    return None


# ------------------------------------------------------------------------------------ places and patches
def slot_sample(buffer: int, tile: int, q: int) -> int:
    """first sample of the patch in slot q of `tile` of `buffer`"""
    assert 0 <= tile < TILES_PER_CHUNK and 0 <= q < SLOTS_PER_TILE
    s = tile * TILE - LEAD + SLOT_FIRST + SLOT * q
    assert 0 <= s and s + SLOT <= CHUNK, (tile, q)
    return buffer * CHUNK + s


def tile_of(sample_in_buffer: int) -> int:
    return (sample_in_buffer + LEAD) // TILE


def frame_patch(k: int, frame: bytes, amp: int) -> np.ndarray:
    """SLOT samples of zeros with `frame` starting at its first sample: sub-sample phase k % 5, carrier angle k % 16"""
    patch = np.zeros((SLOT, 2), dtype=np.int16)
    synth.add_bursts(patch, [synth.Burst(k % 5, amp, k % 16, frame)])
    return patch


POOL_ADDR = 0x510000
TEACHER_ADDRS = (0x6A1B2C, 0x6C3D4E)     # leg 2: taught in an earlier / in a later buffer of the pass


def strong_patch(q: int) -> np.ndarray:
    """slot q's self-validating frame: DF17, every third a DF11 (IID 0); a spread of amplitudes and sub-sample phases"""
    a = POOL_ADDR + q * 0x10F
    frame = synth.df11_frame(a) if q % 3 == 2 else synth.df17_frame(a, 0x1234567 * (q + 1))
    return frame_patch(q, frame, 9000 + 2500 * (q % 8))


def faint_patch(q: int) -> np.ndarray:
    """... the slot's other choice: another address, the kinds and the sub-sample phases shifted, weaker (on an all-zero
    background a frame decodes at any amplitude: the sub-sample phase decides how many of the five trial phases do)"""
    a = POOL_ADDR + 0x4000 + q * 0x111
    frame = synth.df11_frame(a) if q % 3 == 1 else synth.df17_frame(a, 0xABCDEF123 * (q + 1))
    return frame_patch(q + 2, frame, FAINT_AMPS[q])


FAINT_AMPS = tuple(6000 + 700 * (q % 9) for q in range(SLOTS_PER_TILE))


def reply_patch(q: int) -> np.ndarray:
    """... an address/parity reply (DF4 / DF20 / DF5 / DF21) to the first teacher's address; to the second one's in slot 0"""
    df = (4, 20, 5, 21)[q % 4]
    return frame_patch(q + 1, F.ap_frame(df, TEACHER_ADDRS[1 if q == 0 else 0], 0x5A5A5A5A5A5A5A5A ^ (q * 0x0101010101010101)),
                       11000 + 2000 * (q % 7))


def teacher_patch(which: int) -> np.ndarray:
    return frame_patch(3 + which, synth.df17_frame(TEACHER_ADDRS[which], 0x77665544332211 + which), 21000)


# ------------------------------------------------------------------------------------ raw message lists
MSG = np.dtype([("msg", "u1", (14,)), ("len", "u1"), ("try_phase", "u1"), ("score", "<i4"), ("j", "<u4"), ("chunk", "<u8"),
                ("level", "<u8")])            # adsb_msg and the oracle's message alike; `level`: the bits of signal_level
assert MSG.itemsize == 40
KEY = ("chunk", "j", "try_phase", "score", "msg", "level")
OUT_CAP = 1 << 19


def first_difference(got: np.ndarray, want: np.ndarray) -> Optional[tuple]:
    """None when the two lists have the same (chunk, j, try_phase, score, msg, signal_level bits) in the same order;
    else (index, got's key, want's key) of the first place where they part ways."""
    n = min(len(got), len(want))
    same = np.ones(n, dtype=bool)
    for f in KEY:
        e = got[f][:n] == want[f][:n]
        same &= e.all(axis=1) if e.ndim == 2 else e
    if same.all() and len(got) == len(want):
        return None
    i = int(np.argmin(same)) if not same.all() else n

    def show(a):
        return None if i >= len(a) else tuple(bytes(a[f][i]).hex() if f == "msg" else int(a[f][i]) for f in KEY)
    return (i, len(got), len(want), show(got), show(want))


class Device:
    """The raw calls of a context: message lists as MSG arrays (no Python object per message: the large legs have a
    quarter of a million), the two host counters, and the three ways a pass is handed in."""

    def __init__(self, ctx, fmt: str = "cs16", receivers: Optional[np.ndarray] = None):
        self.c, self.L, self.h = ctx, ctx._L, ctx._h
        self.fmt = fmt
        self.map = None if receivers is None else np.ascontiguousarray(receivers, dtype=np.uint32)
        self.out = np.zeros(OUT_CAP, dtype=MSG)

    def counters(self) -> Tuple[int, int]:
        """(adsb_host_replays, adsb_host_sorts)"""
        return int(self.L.adsb_host_replays(self.h)), int(self.L.adsb_host_sorts(self.h))

    def submit(self, ptr: int, n: int) -> None:
        if self.map is not None:
            m = self.map[: -(-n // CHUNK)]
            self.c._check(self.L.adsb_submit_iq_device_rx(self.h, ptr, n, m.ctypes.data), "adsb_submit_iq_device_rx")
        elif self.fmt == "cu8":
            self.c._check(self.L.adsb_submit_iq_device_u8(self.h, ptr, n), "adsb_submit_iq_device_u8")
        else:
            self.c._check(self.L.adsb_submit_iq_device(self.h, ptr, n), "adsb_submit_iq_device")

    def collect(self) -> np.ndarray:
        n = C.c_size_t()
        self.c._check(self.L.adsb_collect(self.h, self.out.ctypes.data, OUT_CAP, C.byref(n)), "adsb_collect")
        return self.out[: n.value].copy()

    def blocking(self, ptr: int, n: int) -> np.ndarray:
        if self.map is not None or self.fmt == "cu8":
            self.submit(ptr, n)
            return self.collect()
        k = C.c_size_t()
        self.c._check(self.L.adsb_demod_iq_device(self.h, ptr, n, self.out.ctypes.data, OUT_CAP, C.byref(k)), "adsb_demod_iq_device")
        return self.out[: k.value].copy()


def oracle_list(orc, iq: np.ndarray, threads: int = 16) -> np.ndarray:
    """orc.demod_iq(iq, threads=16) as a MSG array"""
    from oracle import binding
    a = binding.as_iq(iq)
    out = np.zeros(OUT_CAP, dtype=MSG)
    st = binding.OrcStats()
    n = orc.L.orc_demod_iq_mt(C.byref(orc.filter), a.ctypes.data, a.shape[0], out.ctypes.data, OUT_CAP, C.byref(st), threads)
    assert n <= OUT_CAP
    return out[:n].copy()


def oracle_list_rx(orcs: Sequence, iq: np.ndarray, receivers: Sequence[int]) -> np.ndarray:
    """receivers_support.Model.feed as a MSG array: buffer b through receiver receivers[b]'s own oracle, one demod_iq per
    buffer, every message relabelled with b; the receivers side by side on threads of their own (each stream in order)."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import binding
    a = binding.as_iq(iq)
    n_buf = -(-a.shape[0] // CHUNK)
    parts: List[Optional[np.ndarray]] = [None] * n_buf

    def run(r: int) -> None:
        out = np.zeros(1 << 14, dtype=MSG)
        st = binding.OrcStats()
        for b in range(n_buf):
            if int(receivers[b]) != r:
                continue
            part = np.ascontiguousarray(a[b * CHUNK:(b + 1) * CHUNK])
            n = orcs[r].L.orc_demod_iq(C.byref(orcs[r].filter), part.ctypes.data, part.shape[0], out.ctypes.data, len(out), C.byref(st))
            assert n <= len(out)
            got = out[:n].copy()
            got["chunk"] = b
            parts[b] = got
    with ThreadPoolExecutor(max_workers=len(orcs)) as ex:
        list(ex.map(run, range(len(orcs))))
    return np.concatenate([p for p in parts if p is not None]) if n_buf else np.zeros(0, dtype=MSG)


def quantise(iq: np.ndarray) -> np.ndarray:
    """Any CS16 stream -> CU8 bytes near it (tests/test_gpu_u8.py)"""
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def widen(b: np.ndarray) -> np.ndarray:
    """CU8 bytes -> the CS16 samples the library's default table makes of them (tests/test_gpu_u8.py: t_soapy, widen)"""
    x = np.arange(256, dtype=np.float32)
    table = np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)
    return np.ascontiguousarray(table[b.reshape(-1, 2)])


# ------------------------------------------------------------------------------------ measuring on the device
class Meter:
    """A context of `n_buffers` and an all-zero capture in device memory: the record count a set of patches leaves when it
    is alone in the capture, behind an icao_flush (the context never sees a dense pass: the host orders, nothing overflows
    a tile's sub-bucket)."""

    def __init__(self, n_buffers: int = 17, fmt: str = "cs16", fix: int = 0):
        import torch
        from dump1090_rs_amd import Context
        self.torch = torch
        self.fmt = fmt
        self.n = n_buffers * CHUNK
        self.dev = self.to_device(np.zeros((self.n, 2), dtype=np.int16))
        self.ctx = Context(0, n_buffers)
        if fix:
            self.ctx.set_error_correction(fix)
        self.out = np.zeros(1 << 16, dtype=MSG)

    def host(self, iq: np.ndarray) -> np.ndarray:
        """the CS16 samples this meter's passes see: the samples themselves, or what the CU8 bytes made of them mean"""
        return widen(quantise(iq)) if self.fmt == "cu8" else iq

    def to_device(self, iq: np.ndarray):
        """CS16 samples as this meter's passes read them (CU8: quantised)"""
        d = self.torch.from_numpy(quantise(iq) if self.fmt == "cu8" else np.ascontiguousarray(iq)).cuda()
        self.torch.cuda.synchronize()
        return d

    def close(self) -> None:
        self.ctx.close()
        self.dev = None

    def count(self, patches: Iterable[Tuple[int, np.ndarray]]) -> int:
        patches = list(patches)
        zero = self.dev[:SLOT].clone()      # (this meter's all-zero background: CU8's is a byte near 127)
        for s0, p in patches:
            self.dev[s0:s0 + len(p)] = self.to_device(p)
        self.torch.cuda.synchronize()
        n = self.count_device(self.dev, self.n)
        for s0, p in patches:
            assert len(p) == SLOT
            self.dev[s0:s0 + SLOT] = zero
        return n

    def count_device(self, dev, n_samples: int) -> int:
        k = C.c_size_t()
        self.ctx.icao_flush()
        call = self.ctx._L.adsb_demod_iq_device_u8 if self.fmt == "cu8" else self.ctx._L.adsb_demod_iq_device
        st = call(self.ctx._h, dev.data_ptr(), n_samples, self.out.ctypes.data, len(self.out), C.byref(k))
        if st != -5:   # ADSB_ERR_CAPACITY: the pass is consumed, its messages are not wanted
            self.ctx._check(st, "adsb_demod_iq_device")
        s = self.ctx.stats()
        assert s["retries"] == 0, s
        return int(s["n_records"])


class Pool:
    """The measured counts of the slot patches: strong[q], faint[q] (self-validating: scan hits), reply[q] (match hits,
    with both teachers in the pass), teacher[w]; measured in the middle tile of buffer 8 of a 17-buffer capture.
    A patch is offered to a selection only where the device's count is the number of self-validating trials the oracle's
    trial records hold for it (strong_cpu, faint_cpu): a frame that is followed, alone in the capture, by positions whose
    sliced bits are all zero has records of its own that go away in company (the bitmap always holds address 0)."""
    TEACH_AT = (2 * CHUNK + 40000, 12 * CHUNK + 40000)     # the teachers' places: an earlier and a later buffer

    def __init__(self, meter: Meter):
        at = lambda q: slot_sample(8, 8, q)
        self.strong_p = [strong_patch(q) for q in range(SLOTS_PER_TILE)]
        self.faint_p = [faint_patch(q) for q in range(SLOTS_PER_TILE)]
        self.reply_p = [reply_patch(q) for q in range(SLOTS_PER_TILE)]
        self.teacher_p = [teacher_patch(w) for w in range(2)]
        self.strong = [meter.count([(at(q), p)]) for q, p in enumerate(self.strong_p)]
        self.faint = [meter.count([(at(q), p)]) for q, p in enumerate(self.faint_p)]
        cpu = lambda q, p: len(scan_hits_cpu(meter.host(paste(1, [(slot_sample(0, 8, q), p)]))))
        self.strong_cpu = [cpu(q, p) for q, p in enumerate(self.strong_p)]
        self.faint_cpu = [cpu(q, p) for q, p in enumerate(self.faint_p)]
        teach = [(self.TEACH_AT[w], p) for w, p in enumerate(self.teacher_p)]
        self.teacher = [meter.count([t]) for t in teach]
        both = meter.count(teach)
        assert both == sum(self.teacher)
        self.reply = [meter.count(teach + [(at(q), p)]) - both for q, p in enumerate(self.reply_p)]
        self.reply_alone = [meter.count([(at(q), p)]) for q, p in enumerate(self.reply_p)]

    def patch(self, ident: Tuple[str, int]) -> np.ndarray:
        kind, q = ident
        return {"strong": self.strong_p, "faint": self.faint_p, "reply": self.reply_p}[kind][q]

    def scan_options(self) -> List[List[Tuple[int, int, object]]]:
        return [[(n, 0, (kind, q)) for kind, n, n_cpu in (("strong", self.strong[q], self.strong_cpu[q]), ("faint", self.faint[q], self.faint_cpu[q]))
                 if n == n_cpu] for q in range(SLOTS_PER_TILE)]

    def all_options(self) -> List[List[Tuple[int, int, object]]]:
        return [o + [(0, self.reply[q], ("reply", q))] for q, o in enumerate(self.scan_options())]

    def describe(self) -> str:
        return (f"strong {self.strong} (oracle: {self.strong_cpu}) faint {self.faint} (oracle: {self.faint_cpu}) reply {self.reply} "
                f"reply alone {self.reply_alone} teachers {self.teacher}")


def write_tile(iq: np.ndarray, pool: Pool, buffer: int, tile: int, ids: Sequence[Tuple[str, int]]) -> None:
    for kind, q in ids:
        s0 = slot_sample(buffer, tile, q)
        iq[s0:s0 + SLOT] = pool.patch((kind, q))


def spread(pool: Pool, want: int, salt: int = 0) -> Optional[List[Tuple[int, np.ndarray]]]:
    """Patches whose counts sum to `want`, never many in one tile: strong frames 1280 samples apart in tiles 3, 9 and 14 of
    buffer after buffer, and a selection in the last (ragged) tile of the last buffer for the rest.  A single hit is
    one_hit_patch; 2 is not to be had."""
    if want == 0:
        return []
    if want < 3:
        return [(slot_sample(8, 8, 4), one_hit_patch(salt))] if want == 1 else None
    out, left = [], want
    for b, t, q in ((b, t, q) for b in range(17) for t in (3, 9, 14) for q in (1, 5, 9, 13, 17, 21)):
        if left - pool.strong[q] < 12:
            break
        out.append((slot_sample(b, t, q), pool.strong_p[q]))
        left -= pool.strong[q]
    if left > 40:
        return None
    ids = choose_slots(without_slot(pool.scan_options(), salt), lambda s, m: s == left)
    return None if ids is None else out + tile_patches(pool, 16, 16, ids)


def one_hit_patch(salt: int = 0) -> np.ndarray:
    """A DF17 so deep in SLOT samples of noise that a single trial phase decodes (0, 1 and 6 records at amplitudes 6000,
    7000 and 8000 on the MI355X); `salt` walks the amplitudes around 7000."""
    amp = 7000 + (0, 250, -250, 500, -500, 750, 125, -125, 375, -375)[salt % 10]
    patch = synth.noise_numpy(SLOT, seed=9100 + 7000)
    synth.add_bursts(patch, [synth.Burst(5 * 8 + 2, amp, 3, synth.df17_frame(0x600111, 0xABCDEF123))])
    return patch


def settle(count: Callable[[object], object], target, make: Callable[[int, int], object], accept=None, tries: int = 24):
    """make(want, salt) -> an input whose counts ADD UP to `want`; count(input) -> what the device (or the oracle) finds in
    it.  Neighbouring frames are not quite independent -- a position behind a frame whose sliced bits are all zero is an
    address/parity trial with residual 0, which the address bitmap always holds, and whether there is one depends on what
    follows the frame -- so the sum is a first guess: the input is measured whole, and `want` moved by what it missed.
    -> (input, measured) of the first input whose measured count is accepted (default: equals `target`)."""
    accept = accept or (lambda got: got == target)
    want, log = target, []
    for salt in range(tries):
        made = make(want, salt)
        if made is None:
            log.append((want, None))
            want = target + (salt + 1) // 2 * (1 if salt % 2 else -1)
            continue
        got = count(made)
        log.append((want, got))
        if accept(got):
            return made, got
        want += target - (got if isinstance(got, int) else got[0])   # (a tuple's first member is the count `want` steers)
    raise AssertionError(("no input with the wanted count", target, log))


def scan_hits_cpu(iq_buffer: np.ndarray) -> List[Tuple[int, int]]:
    """(j, try_phase) of the self-validating trials of one buffer, from the oracle's trial records: a DF17 / DF18 with
    residual 0, a DF11 whose residual is an interrogator id (< 128) -- the hits the SCAN finds, whatever the bitmap holds."""
    from oracle import binding
    L = binding.lib()
    _, tr = binding.all_trials(iq_buffer, 0)
    out = []
    for r in tr:
        msg = bytes(r["msg"])
        df = msg[0] >> 3
        if df in (17, 18) and L.orc_modes_checksum(msg, 112) == 0 or df == 11 and L.orc_modes_checksum(msg, 56) < 128:
            out.append((int(r["j_tp"]) & 0xFFFFFF, int(r["j_tp"]) >> 24))
    return out


def scan_hits_in_tile(iq: np.ndarray, buffer: int, tile: int) -> int:
    part = np.ascontiguousarray(iq[buffer * CHUNK:(buffer + 1) * CHUNK])
    return sum(1 for j, _ in scan_hits_cpu(part) if j // TILE == tile)


def tile_patches(pool: Pool, buffer: int, tile: int, ids: Sequence[Tuple[str, int]]) -> List[Tuple[int, np.ndarray]]:
    return [(slot_sample(buffer, tile, q), pool.patch((kind, q))) for kind, q in ids]


def paste(n_buffers: int, patches: Iterable[Tuple[int, np.ndarray]]) -> np.ndarray:
    iq = np.zeros((n_buffers * CHUNK, 2), dtype=np.int16)
    for s0, p in patches:
        iq[s0:s0 + len(p)] = p
    return iq


def without_slot(options, salt: int):
    """the options of a tile with one slot left empty: another selection for every salt"""
    return [([] if salt and q == (salt * 7) % len(options) else o) for q, o in enumerate(options)]


# ------------------------------------------------------------------------------------ many hits: templates
TEMPLATE_TILES = 15                      # a template's frames stand in tiles 0 .. 14; 15 and 16 are for topping up
TEMPLATE_RANGE = (498, 508)              # hits of a template buffer alone in a pass


def template_frames(k: int, count: int) -> List[Tuple[int, np.ndarray]]:
    """(sample in the buffer, patch) of template k's first `count` frames.  Sixteen addresses of its own; frame i stands in
    tile i % 15, in every second slot first (640 samples apart), and is by i % 8: a DF17, a DF4 reply, a DF11 with IID 0, a
    DF20 reply, a DF18 of a taught address, a DF11 with IID != 0, a DF5 / DF21 reply, a DF17 again; the addresses walk
    with another stride than the kinds, so replies stand before and behind the frames that teach their address.  Frame 5
    is a DF18 of an address nothing teaches (it adds addr | 1 << 25 every time)."""
    addrs = [0x700000 + 0x1000 * k + 0x111 * i for i in range(16)]
    out = []
    for i in range(count):
        a = addrs[(5 * i + i // 8) % 16]
        pay = (0x9E3779B97F4A7C15 * (i + 1 + 1000 * k)) & ((1 << 64) - 1)
        kind = i % 8
        if i == 5:
            frame = F.es_frame(18, 0x7F0000 + k, pay)
        elif kind in (0, 7):
            frame = F.es_frame(17, a, pay)
        elif kind == 1:
            frame = F.ap_frame(4, a, pay)
        elif kind == 2:
            frame = F.df11_frame(a, 0)
        elif kind == 3:
            frame = F.ap_frame(20, a, pay)
        elif kind == 4:
            frame = F.es_frame(18, a, pay)
        elif kind == 5:
            frame = F.df11_frame(a, 1 + (i + k) % 127)
        else:
            frame = F.ap_frame((5, 21)[(i // 8) % 2], a, pay)
        tile, turn = i % TEMPLATE_TILES, i // TEMPLATE_TILES
        assert turn < 11, count
        q = 1 if tile == 0 and turn == 0 else 2 * turn
        # (the sub-sample phase walks inside a tile too: with i alone every frame of tile t would have phase t % 5)
        out.append((slot_sample(0, tile, q), frame_patch(i + turn + k, frame, 9000 + 2500 * ((i + k) % 8))))
    return out


class Templates:
    """Eight template buffers with disjoint address sets, each trimmed on the device to TEMPLATE_RANGE hits."""

    def __init__(self, meter: Meter):
        self.buffers, self.counts, self.frames = [], [], []
        lo, hi = TEMPLATE_RANGE
        for k in range(8):
            made, got = settle(lambda fr: meter.count(fr), (lo + hi) // 2,
                               lambda want, salt, k=k: template_frames(k, max(8, min(160, want // 4 + salt % 2))),
                               accept=lambda got: lo <= got <= hi)
            self.frames.append(len(made))
            self.counts.append(got)
            self.buffers.append(paste(1, made))

    def hits_per_frame(self) -> float:
        return sum(self.counts) / sum(self.frames)


def topup_places(n_buffers: int) -> List[Tuple[int, int, int]]:
    """(buffer, tile, slot) for topping a templated stream up: every second slot of tile 16, buffer after buffer"""
    return [(b, 16, q) for q in range(0, SLOTS_PER_TILE, 2) for b in range(n_buffers)]


def compose(pool: Pool, templates: Templates, n_buffers: int, want: int, salt: int = 0) -> Optional[np.ndarray]:
    """Buffer b holds template b % 8; strong pool patches in the last tile of buffer after buffer bring the sum of the
    counts to within a few of `want`, and a selection in tile 15 of buffer `salt` makes it exact."""
    iq = np.zeros((n_buffers * CHUNK, 2), dtype=np.int16)
    for b in range(n_buffers):
        iq[b * CHUNK:(b + 1) * CHUNK] = templates.buffers[b % 8]
    left = want - sum(templates.counts[b % 8] for b in range(n_buffers))
    if left < 0:
        return None
    for b, t, q in topup_places(n_buffers):
        if left - pool.strong[q] < 12:
            break
        s0 = slot_sample(b, t, q)
        iq[s0:s0 + SLOT] = pool.strong_p[q]
        left -= pool.strong[q]
    if left >= 30:
        return None
    if left:
        ids = choose_slots(without_slot(pool.scan_options(), salt), lambda s, m: s == left)
        if ids is None:
            return None
        write_tile(iq, pool, salt % n_buffers, 15, ids)
    return iq


def device_records(ctx, dev_ptr: int, n_samples: int) -> np.ndarray:
    """The trial records the device makes of a capture on an empty filter, through the shard hooks of a context of its own
    (adsb_shard_scan / adsb_shard_finish), in (buffer, j, try_phase) order: the order a device-ordered pass scores them in."""
    ctx.icao_flush()
    ctx.shard_scan(dev_ptr, n_samples)
    rec = ctx.shard_finish(np.zeros(0, dtype=np.uint32))
    j, tp = rec["j_tp"] & 0xFFFFFF, rec["j_tp"] >> 24
    order = np.lexsort((tp, j, rec["chunk"]))
    return rec[order]


def positions(rec: np.ndarray) -> np.ndarray:
    return (rec["chunk"].astype(np.uint64) << np.uint64(24)) | (rec["j_tp"] & 0xFFFFFF).astype(np.uint64)

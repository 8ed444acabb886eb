"""Scoring per receiver on the device, the part that needs no GPU: the parallel formulation the keyed kernels implement,
restated in a few lines and compared with the sequential replay (adsb_replay_records_rx); the new kernels' ISA for gfx950;
and the declarations of the new entry points."""
import re
import shutil
import subprocess

import numpy as np

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS
from tests.conftest import ROOT
from tests.test_fix_scored_cpu import kernel_figures

CSRC = ROOT / "dump1090_rs_amd" / "csrc"
CHUNK = RS.CHUNK
NEW_KERNELS = ("k_rx_adders", "k_score_rx", "k_emit_rx", "k_rx_set_fill", "k_rx_set_lookup")
# what a trial asks the filter about, as the record builder classifies it (adsb_device.h: ScoreKind)
OTHER, AP_SHORT, AP_LONG, DF11_IID0, DF11, DF17, DF18, NONE = range(8)


def classify(msg: bytes):
    """(kind, value) of one trial: src/mode_s/mod.rs:56-135 without the filter"""
    if not any(msg):
        return NONE, 0
    df = F.getbits(msg, 1, 5)
    nbits = 112 if df & 0x10 else 56
    if df in (0, 4, 5):
        return AP_SHORT, F.crc_residual(msg, nbits)
    if df == 11:
        crc = F.crc_residual(msg, nbits)
        if crc & 0xFFFF80:
            return OTHER, 0
        return (DF11_IID0 if crc & 0x7F == 0 else DF11), F.getbits(msg, 9, 32)
    if df in (17, 18):
        if F.crc_residual(msg, nbits):
            return OTHER, 0
        return (DF17 if df == 17 else DF18), F.getbits(msg, 9, 32)
    if df in F.AP_LONG or df >= 24:
        return AP_LONG, F.crc_residual(msg, 112)
    return OTHER, 0


def parallel_pass(records, receivers, before):
    """One pass as k_rx_adders / k_score_rx / k_emit_rx compute it.  `before`: the (receiver, value) pairs in the filters
    when the pass begins.  -> (messages [(chunk, j, try_phase, score, bytes)], additions [(receiver, value)] in order)"""
    order = np.lexsort((records["j_tp"] >> 24, records["j_tp"] & 0xFFFFFF, records["chunk"]))
    rec = records[order]
    n = len(rec)
    kinds = [classify(bytes(m)) for m in rec["msg"]]
    rx = [int(receivers[int(c)]) for c in rec["chunk"]]
    first = {}                                           # k_rx_adders: atomic-min of the index per (receiver, value)
    for i, (kind, v) in enumerate(kinds):
        if kind in (DF11_IID0, DF17):
            first[(rx[i], v)] = min(first.get((rx[i], v), n), i)
    in_filter = lambda i, v: v == 0 or (rx[i], v) in before or first.get((rx[i], v), n) < i   # noqa: E731
    score, adds = [], []
    for i, (kind, v) in enumerate(kinds):                # k_score_rx: every trial on its own
        known = in_filter(i, v)
        add = 0
        if kind == AP_SHORT or kind == DF11:
            s = 1000 if known else -1
        elif kind == AP_LONG:
            s = 1000 if known else -2
        elif kind == DF11_IID0:
            s, add = (1600, 0) if known else (750, v)
        elif kind in (DF17, DF18):
            s, add = (1800, 0) if known else (1400, v if kind == DF17 else v | F.ADSB_NT)
        else:
            s = -3 if kind == NONE else -2
        score.append(s)
        adds.append(add)
    pos = [(int(r["chunk"]), int(r["j_tp"]) & 0xFFFFFF) for r in rec]
    msgs, additions = [], []
    i = 0
    while i < n:                                         # ... the best of a position's trials, strictly greater from -2
        z = i
        while z < n and pos[z] == pos[i]:
            z += 1
        best, win = -2, None
        for k in range(i, z):
            if score[k] > best:
                best, win = score[k], k
        if win is not None and best >= 0:
            m = bytes(rec["msg"][win])
            msgs.append((pos[i][0], pos[i][1], int(rec["j_tp"][win]) >> 24, best, m[:14 if m[0] & 0x80 else 7]))
        i = z
    for i in range(n):                                   # k_emit_rx: the additions in order, with their receiver
        if adds[i]:
            additions.append((rx[i], adds[i]))
    return msgs, additions


def small_dense_input():
    """Six buffers of the dense stream, three receivers, and an aircraft X that receivers 0 and 1 add in opposite order:
    0 hears its DF17 (buffer 0) before its reply (buffer 3), 1 gets the reply (buffer 1) before the DF17 (buffer 2)."""
    x = 0x4B1A2C
    df17, reply = synth.df17_frame(x, 0x58B986D0B3BD25), F.ap_frame(4, x, 0x1234567)[:7]
    iq = F.fill_capture(900, 6, per_buffer=60)
    bursts = []
    for k, (b, frame) in enumerate([(0, df17), (1, reply), (2, df17), (3, reply)]):
        a = b * CHUNK + 40000 + 977 * k
        iq[a - 100:a + 500] = synth.noise_numpy(600, seed=4242 + k)
        bursts.append(synth.Burst(5 * a + 1 + k, 24000, 1 + k, frame))
    synth.add_bursts(iq, bursts)
    return iq, np.array([0, 1, 1, 0, 2, 2], dtype=np.uint32), reply


def test_the_parallel_formulation_equals_the_sequential_replay(hip_lib, oracle_mod):
    from dump1090_rs_amd.context import replay_records_rx
    n_receivers = 3
    iq, m, reply = small_dense_input()
    records = RS.trial_records(iq)
    assert len(records) >= 8 * 6
    tables = np.zeros((n_receivers, 4096), dtype=np.uint32)
    mine = [F.PyFilter() for _ in range(n_receivers)]
    # two passes without a flush, the second with the receivers swapped round: first-adder table, then keyed set
    for k, receivers in enumerate((m, (m + 1) % n_receivers)):
        before = {(r, a) for r in range(n_receivers) for a in mine[r].a if 0 < a <= 0xFFFFFF}
        truth = replay_records_rx(records, receivers, tables, cap=1 << 16)
        want = [(t.chunk, t.j, t.try_phase, t.score, bytes(t.msg[:t.msglen])) for t in truth]
        got, additions = parallel_pass(records, receivers, before)
        assert got == want, k
        for r, a in additions:
            mine[r].add(a)
        for r in range(n_receivers):
            assert mine[r].a == tables[r].tolist(), (k, r)
        if k == 0:
            # opposite order: receiver 0's reply (buffer 3, behind its DF17) scores 1000, receiver 1's (buffer 1, in
            # front of its DF17) is not emitted -- and both receivers add X, each once
            assert sorted((g[0], g[3]) for g in got if g[4] == reply) == [(3, 1000)]
            assert sorted(r for r, a in additions if a == 0x4B1A2C) == [0, 1]
            assert len({r for r, _ in additions}) == n_receivers


def spill_counts(asm: str, kernel: str) -> dict:
    """.sgpr_spill_count / .vgpr_spill_count of the kernel's entry in the code object's metadata"""
    m = re.search(r"\.name:\s+_ZN4adsb12_GLOBAL__N_1\d+" + kernel + r"E\S*\n(.*?)\.wavefront_size", asm, re.S)
    assert m, kernel
    return {f: int(re.search(r"\." + f + r":\s+(\d+)", m.group(1)).group(1)) for f in ("sgpr_spill_count", "vgpr_spill_count")}


def test_the_new_kernels_cross_compile_for_gfx950_without_scratch(tmp_path):
    from dump1090_rs_amd import build
    assert CSRC / "adsb_score_rx.hip" in build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in build.FLAGS if f != "-shared"]
    subprocess.run([hipcc, *flags, "-Werror", "-save-temps", "-c", str(CSRC / "adsb_score_rx.hip"), "-o", str(tmp_path / "rx.o")],
                   check=True, cwd=tmp_path, capture_output=True, timeout=600)
    asm = next(tmp_path.glob("adsb_score_rx*amdgcn-amd-amdhsa-gfx950.s")).read_text()
    for kernel in NEW_KERNELS:
        f = kernel_figures(asm, kernel)
        body = f.pop("body")
        spills = spill_counts(asm, kernel)
        print(kernel, f, spills)
        assert f["scratch"] == 0 and spills["vgpr_spill_count"] == 0, (kernel, f, spills)
        assert "scratch_" not in body, kernel
    # k_emit_rx stages its messages as k_emit does: the same LDS
    assert kernel_figures(asm, "k_emit_rx")["lds"] == 12368


def test_the_new_entry_points_are_declared_everywhere():
    header = (ROOT / "include" / "adsb_hip.h").read_text()
    lib_py = (ROOT / "dump1090_rs_amd" / "_lib.py").read_text()
    rust = (ROOT / "integration" / "rust" / "src" / "hip_ffi.rs").read_text()
    context_py = (ROOT / "dump1090_rs_amd" / "context.py").read_text()
    for decl in ("int adsb_set_receiver_scoring(adsb_ctx *ctx, int enabled);",
                 "int adsb_get_receiver_scoring(const adsb_ctx *ctx);",
                 "int adsb_selftest_rx_score_counters(const adsb_ctx *ctx, uint64_t *out4);",
                 "int adsb_selftest_rx_score_tune(adsb_ctx *ctx, uint32_t set_lg, uint32_t probe_max);",
                 "uint32_t adsb_rx_set_home(uint64_t key, uint32_t set_lg);"):
        assert decl in header, decl
    assert re.search(r"int adsb_selftest_rx_set_lookup\(adsb_ctx \*ctx, const uint64_t \*keys, size_t n_keys, const uint64_t \*queries,\s+"
                     r"size_t n_q,\s+uint32_t \*out\);", header)
    for name in ("adsb_set_receiver_scoring", "adsb_get_receiver_scoring", "adsb_selftest_rx_score_counters",
                 "adsb_selftest_rx_score_tune", "adsb_selftest_rx_set_lookup", "adsb_rx_set_home"):
        assert f"L.{name}.argtypes" in lib_py, name
        assert f"pub fn {name}(" in rust, name
    for method in ("def set_receiver_scoring", "def get_receiver_scoring", "def selftest_rx_score_counters",
                   "def selftest_rx_score_tune", "def selftest_rx_set_lookup", "def rx_set_home"):
        assert method in context_py, method
    # the scoring item has left the header's "Not offered" list; the others stay
    not_offered = header[header.index("Not offered: carry-over with receivers"):]
    not_offered = not_offered[:not_offered.index("*/")]
    assert "scoring on the device" not in not_offered
    for item in ("carry-over with receivers", "valid lengths per", "adsb_multi / the shard calls", "adsb_feed"):
        assert item in not_offered, item


def test_the_host_side_hooks_without_a_device(hip_lib):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd.context import rx_set_home
    import ctypes as C
    L = _lib.lib()
    assert L.adsb_set_receiver_scoring(None, 1) == -1 and L.adsb_get_receiver_scoring(None) == -1
    assert L.adsb_selftest_rx_score_counters(None, (C.c_uint64 * 4)()) == -1 and L.adsb_selftest_rx_score_tune(None, 0, 0) == -1
    # the home slot: the top set_lg bits of key x 2^64 / phi, and nothing for a geometry that is none
    for key in (0, 1, (16383 << 24) | 0xFFFFFF, (5 << 24) | 0x4B1A2C):
        for lg in (1, 6, 13, 22, 32):
            assert rx_set_home(key, lg) == ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - lg)
    assert rx_set_home(12345, 0) == 0 and rx_set_home(12345, 33) == 0

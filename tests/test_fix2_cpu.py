"""Two-bit repair of DF17/18 (ADSB_FIX_2BIT, include/adsb_hip.h "Error correction") without a GPU: the pair
syndromes, the host lookup, the scan kernels' pair table, the host replay in every mode against the CPU restatement
(tests/fix2_restatement.c), and the ISA of the two-bit kernels against their twins."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fix2_support as f2
from tests import fix_support as fs
from tests.test_fix_cpu import captures, gf_divx, gf_mulx, oracle_records
from tests.test_u8_cpu import SCAN_FAST, kernel_figures, HEAD_CS16

# What hipcc --offload-arch=gfx950 made of the eight k_scan_fix instantiations before two-bit repair existed (template
# arguments FROM_MAG, FUSED, FIELDS, U8 as mangled): the two-bit kernel shares their body and must not move them.
HEAD_FIX = {
    "Lb0ELb0ELb0ELb0E": {"insts": 2447, "sgpr": 100, "vgpr": 102, "accum_offset": 104, "lds": 33280, "scratch": 0, "sgpr_spill": 18, "vgpr_spill": 0},
    "Lb0ELb0ELb0ELb1E": {"insts": 3270, "sgpr": 100, "vgpr": 97, "accum_offset": 96, "lds": 34304, "scratch": 0, "sgpr_spill": 22, "vgpr_spill": 0},
    "Lb0ELb0ELb1ELb0E": {"insts": 2488, "sgpr": 100, "vgpr": 104, "accum_offset": 104, "lds": 33920, "scratch": 0, "sgpr_spill": 22, "vgpr_spill": 0},
    "Lb0ELb0ELb1ELb1E": {"insts": 3275, "sgpr": 100, "vgpr": 97, "accum_offset": 96, "lds": 34944, "scratch": 0, "sgpr_spill": 26, "vgpr_spill": 0},
    "Lb0ELb1ELb1ELb0E": {"insts": 7945, "sgpr": 100, "vgpr": 129, "accum_offset": 120, "lds": 52720, "scratch": 0, "sgpr_spill": 52, "vgpr_spill": 0},
    "Lb0ELb1ELb1ELb1E": {"insts": 9266, "sgpr": 100, "vgpr": 129, "accum_offset": 108, "lds": 53744, "scratch": 0, "sgpr_spill": 60, "vgpr_spill": 0},
    "Lb1ELb0ELb0ELb0E": {"insts": 2042, "sgpr": 100, "vgpr": 97, "accum_offset": 84, "lds": 33280, "scratch": 0, "sgpr_spill": 8, "vgpr_spill": 0},
    "Lb1ELb1ELb1ELb0E": {"insts": 6752, "sgpr": 100, "vgpr": 129, "accum_offset": 96, "lds": 52720, "scratch": 0, "sgpr_spill": 35, "vgpr_spill": 0},
}


def syndromes(oracle_mod):
    O = oracle_mod.lib()
    syn = []
    for b in range(112):
        e = bytearray(14)
        e[b >> 3] = 0x80 >> (b & 7)
        syn.append(O.orc_modes_checksum(bytes(e), 112))
    return syn


def key_of(b):
    """H' of the 112-bit message with only bit b set: x^(55 - b)"""
    p = 1
    for _ in range(111 - b):
        p = gf_mulx(p)
    for _ in range(56):
        p = gf_divx(p)
    return p


def test_pair_syndromes_are_distinct_nonzero_and_never_a_single_bits(oracle_mod):
    syn = syndromes(oracle_mod)
    single = syn[5:]
    pairs = [syn[a] ^ syn[b] for a, b in f2.PAIRS]
    assert len(pairs) == 5671 and len(set(pairs)) == 5671 and 0 not in pairs
    assert not set(pairs) & set(single)
    got = (C.c_uint32 * 5671)()
    assert f2.restatement().fix2_pair_syndromes(got) == 5671
    assert list(got) == pairs


def replay(rec, mode):
    from dump1090_rs_amd.context import replay_records
    return [fs.key(m) for m in replay_records(rec, mode=mode)]


def test_host_lookup_repairs_every_pair_and_only_in_mode_3():
    """Hand-made records: a clean DF17 that teaches the filter, then its 5671 two-bit copies and the copies of an
    unknown aircraft, one position each.  The replay computes the residuals itself (pad 0) and finds each pair."""
    from dump1090_rs_amd.context import TRIAL_DTYPE
    from dump1090_rs_amd import synth
    good = synth.df17_frame(fs.KNOWN[0], 0x1234)
    other = synth.df17_frame(0x7C1234, 0x99)
    frames = [good] + [f2.flip2(good, a, b) for a, b in f2.PAIRS] + [f2.flip2(other, a, b) for a, b in f2.PAIRS[::97]]
    rec = np.zeros(len(frames), dtype=TRIAL_DTYPE)
    for i, f in enumerate(frames):
        rec[i]["msg"] = np.frombuffer(f, dtype=np.uint8)
        rec[i]["j_tp"] = (1000 + 400 * i) % 131072 | 4 << 24
        rec[i]["chunk"] = (1000 + 400 * i) // 131072
        rec[i]["power"] = 10 ** 9
    got3 = replay(rec, f2.FIX2)
    assert got3[0][1] == 1400 and got3[0][0] == good
    assert [k[1] for k in got3[1:]] == [1100] * 5671
    assert all(k[0] == good for k in got3[1:])
    for mode in (0, 1):
        got = replay(rec, mode)
        assert len(got) == 1 and got[0] == got3[0]


def test_the_device_pair_table_is_complete_and_its_probes_bounded(oracle_mod):
    from dump1090_rs_amd import _lib
    L = _lib.lib()
    params = (C.c_uint32 * 4)()
    tab = np.zeros(4 * 8192, dtype=np.uint32)
    assert L.adsb_selftest_fix2_table(params, tab.ctypes.data, 4 * 8192 - 1) == _lib.ADSB_ERR_CAPACITY
    assert L.adsb_selftest_fix2_table(params, tab.ctypes.data, tab.size) == 0
    m0, m1, lg, probes = list(params)
    assert m0 & 1 and m1 & 1 and lg == 13
    # the bound k_scan_fix2 and k_scan_simple_fix2 assume: two buckets of two entries, no further probing
    assert probes == 4
    syn = syndromes(oracle_mod)
    H = {b: key_of(b) for b in range(5, 112)}
    want = {H[a] ^ H[b]: (a, b) for a, b in f2.PAIRS}
    assert len(want) == 5671 and not set(want) & set(H.values())
    ent = tab.reshape(-1, 2, 2)   # bucket, way, (key | a << 24, residual | b << 24)
    found = {}
    for bucket in range(1 << lg):
        for way in range(2):
            k, r = int(ent[bucket, way, 0]), int(ent[bucket, way, 1])
            if k == 0 and r == 0:
                continue
            key, a, res, b = k & 0xFFFFFF, k >> 24, r & 0xFFFFFF, r >> 24
            assert want.get(key) == (a, b), (bucket, way)           # no foreign keys
            assert res == syn[a] ^ syn[b]                           # the residual the hit carries
            homes = {((key * m) & 0xFFFFFFFF) >> (32 - lg) for m in (m0, m1)}
            assert bucket in homes                                  # where its probes look
            assert key not in found
            found[key] = bucket
    assert len(found) == 5671


@pytest.mark.parametrize("name", ["fixture0", "fixture1", "fixture2", "damaged", "synth", "pairs"])
def test_replays_in_every_mode_are_the_restatements(name, fixture_iq, oracle_mod):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd.context import ModeSMessage
    caps = captures(fixture_iq)
    names = sorted(n for n in caps if n not in ("damaged", "synth"))
    if name == "pairs":
        iq = f2.pair_stream(pairs=f2.PAIRS[::23])[0]
    else:
        iq = caps[names[int(name[-1])]] if name.startswith("fixture") else caps[name]
    rec = oracle_records(iq, oracle_mod)
    want = {mode: f2.Restated(mode).demod_iq(iq) for mode in (0, 1, f2.FIX2)}
    # modes 0 and 1 of this restatement are the existing ones
    assert want[0] == fs.Restated(0).demod_iq(iq) and want[1] == fs.Restated(1).demod_iq(iq)
    for mode in (0, 1, f2.FIX2):
        assert replay(rec, mode) == want[mode], mode
    if name == "pairs":
        assert sum(k[1] == 1100 for k in want[f2.FIX2]) >= len(f2.PAIRS[::23])
    L = _lib.lib()
    out = (_lib.AdsbMsg * 16384)()
    n = C.c_size_t()
    t = np.zeros(4096, dtype=np.uint32)
    assert L.adsb_replay_records_fix(t.ctypes.data, np.ascontiguousarray(rec).ctypes.data, len(rec), 2, out, 16384,
                                     C.byref(n)) == -1
    for mode in (0, 1, f2.FIX2):
        for runs, parts in ((1, 1), (3, 7), (5, 16)):
            table = np.zeros(4096, dtype=np.uint32)
            par = C.c_int()
            st = L.adsb_selftest_parallel_replay_fix(table.ctypes.data, np.ascontiguousarray(rec).ctypes.data, len(rec),
                                                     runs, parts, 4, mode, out, 16384, C.byref(n), C.byref(par))
            assert st == 0
            got = [fs.key(ModeSMessage(bytes(m.msg), int(m.len), float(m.signal_level), int(m.score), int(m.j),
                                       int(m.try_phase), int(m.chunk))) for m in out[: n.value]]
            assert got == want[mode], (mode, runs, parts)


def test_restatement_repairs_every_two_bit_copy_of_a_known_aircraft():
    iq, want = f2.pair_stream()
    assert len(iq) <= 32 * fs.CHUNK
    got = f2.Restated(f2.FIX2).demod_iq(iq)
    f2.check_pair_stream(got, want)
    assert not any(k[1] in (1100, 1200) for k in f2.Restated(0).demod_iq(iq[: 2 * fs.CHUNK]))


def test_fix2_kernels_keep_their_twins_occupancy_and_leave_k_scan_fix_as_it_was(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                    "-save-temps", "-c", str(SCAN_FAST), "-o", str(tmp_path / "scan.o")],
                   check=True, cwd=tmp_path, capture_output=True, timeout=600)
    asm = next(tmp_path.glob("*amdgcn-amd-amdhsa-gfx950.s")).read_text()
    import tests.test_u8_cpu as u8
    fast = kernel_figures(asm)
    saved = u8.PREFIX
    try:
        u8.PREFIX = "_ZN4adsb12_GLOBAL__N_110k_scan_fixI"
        fix = kernel_figures(asm)
        u8.PREFIX = "_ZN4adsb12_GLOBAL__N_111k_scan_fix2I"
        fix2 = kernel_figures(asm)
    finally:
        u8.PREFIX = saved
    assert fix == HEAD_FIX
    for args, want in HEAD_CS16.items():
        assert fast[args + "Lb0E"] == want
    assert set(fix2) == set(HEAD_FIX)
    for args, f in sorted(fix2.items()):
        a = re.findall(r"Lb([01])E", args)
        twin = fix[args]
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (args, f)
        assert f["lds"] == twin["lds"], (args, f, twin)   # the pair table is in global memory
        per_cu = 2 if a[1] == "1" else 4
        assert per_cu * f["lds"] <= 160 * 1024
        assert f["vgpr"] <= (128 if per_cu == 4 else 256)
        print(args, "insts %+d" % (f["insts"] - twin["insts"]), "sgpr_spill %+d" % (f["sgpr_spill"] - twin["sgpr_spill"]),
              "vgpr %d -> %d" % (twin["vgpr"], f["vgpr"]))

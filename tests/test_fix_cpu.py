"""Single-bit repair of DF17/18 (ADSB_FIX_1BIT, include/adsb_hip.h "Error correction") without a GPU: the syndromes,
the scan kernels' table, the host replay in both modes against the CPU restatement (tests/fix_restatement.c), and the
ISA of the fix kernels against their twins."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fix_support as fs
from tests.test_u8_cpu import SCAN_FAST, kernel_figures, HEAD_CS16

G = 0xFFF409


def gf_mulx(a):
    a <<= 1
    return (a ^ G) & 0xFFFFFF if a & 0x1000000 else a


def gf_divx(a):
    return ((a ^ G) >> 1) | 0x800000 if a & 1 else a >> 1


def test_syndromes_are_the_oracles_and_distinct(oracle_mod):
    from dump1090_rs_amd import _lib
    L = _lib.lib()
    got = (C.c_uint32 * 112)()
    assert L.adsb_selftest_fix_table(got) == 0
    O = oracle_mod.lib()
    for b in range(112):
        e = bytearray(14)
        e[b >> 3] = 0x80 >> (b & 7)
        assert got[b] == O.orc_modes_checksum(bytes(e), 112), b
    rep = list(got)[5:]
    assert len(set(rep)) == 107 and 0 not in rep
    # the restatement uses the same ones
    mine = (C.c_uint32 * 112)()
    fs.restatement().fix_syndrome_table(mine)
    assert list(mine) == list(got)


def test_the_device_table_is_complete_and_collision_free():
    from dump1090_rs_amd import _lib
    L = _lib.lib()
    mult, tab = C.c_uint32(), (C.c_uint32 * 512)()
    assert L.adsb_selftest_fix_hash(C.byref(mult), tab, 512) == 0
    assert mult.value & 1
    # keys: H' = x^-56 * syn(b) = x^(55 - b)
    seen = {}
    for b in range(5, 112):
        p = 1
        for _ in range(111 - b):
            p = gf_mulx(p)
        for _ in range(56):
            p = gf_divx(p)
        slot = ((p * mult.value) & 0xFFFFFFFF) >> (32 - 9)
        assert tab[slot] == p | b << 24, b
        seen[slot] = b
    assert len(seen) == 107
    assert sum(1 for v in tab if v) == 107


def oracle_records(iq, oracle_mod) -> np.ndarray:
    """The oracle's trials of every buffer of a capture, as adsb_trial records (residual left to the replay)."""
    parts = []
    for chunk, off in enumerate(range(0, len(iq), fs.CHUNK)):
        _, tr = oracle_mod.all_trials(np.ascontiguousarray(iq[off:off + fs.CHUNK]), chunk)
        parts.append(tr)
    return np.concatenate(parts)


def captures(fixture_iq):
    from dump1090_rs_amd import synth
    out = {name: iq for name, iq in fixture_iq.items()}
    out["damaged"] = fs.damaged_capture()[0]
    out["synth"] = synth.make_iq(3 * fs.CHUNK, n_bursts=900, seed=4242, n_icao=40)
    return out


def test_restatement_repairs_every_damaged_copy_of_a_known_aircraft():
    iq, clean, repairable = fs.damaged_capture()
    got1 = fs.Restated(1).demod_iq(iq)
    got0 = fs.Restated(0).demod_iq(iq)
    fixed = [k for k in got1 if k[1] == 1200]
    assert fs.repaired_by_slot(fixed, got0) == {4 + b: f for b, f in repairable.items()}
    assert all(k[1] != 1200 for k in got0)
    assert set(got0) <= set(got1)
    assert [k for k in got1 if k[1] != 1200] == got0
    assert {k[0] for k in got0} >= set(clean.values())


@pytest.mark.parametrize("name", ["fixture0", "fixture1", "fixture2", "damaged", "synth"])
def test_replay_mode0_is_adsb_replay_records_and_mode1_is_the_restatement(name, fixture_iq, oracle_mod):
    from dump1090_rs_amd.context import replay_records
    caps = captures(fixture_iq)
    names = sorted(n for n in caps if n not in ("damaged", "synth"))
    iq = caps[names[int(name[-1])]] if name.startswith("fixture") else caps[name]
    rec = oracle_records(iq, oracle_mod)
    plain = [fs.key(m) for m in replay_records(rec)]
    assert [fs.key(m) for m in replay_records(rec, mode=0)] == plain
    from dump1090_rs_amd import _lib
    L = _lib.lib()
    t = np.zeros(4096, dtype=np.uint32)
    out = (_lib.AdsbMsg * 8192)()
    n = C.c_size_t()
    assert L.adsb_replay_records_fix(t.ctypes.data, np.ascontiguousarray(rec).ctypes.data, len(rec), 0, out, 8192,
                                     C.byref(n)) == 0
    assert n.value == len(plain)
    assert plain == fs.Restated(0).demod_iq(iq)
    want1 = fs.Restated(1).demod_iq(iq)
    assert [fs.key(m) for m in replay_records(rec, mode=1)] == want1
    assert L.adsb_replay_records_fix(t.ctypes.data, np.ascontiguousarray(rec).ctypes.data, len(rec), 2, out, 8192,
                                     C.byref(n)) == -1
    # the parallel replay (what adsb_multi_collect does with large captures), runs at buffer boundaries
    for mode, want in ((0, plain), (1, want1)):
        for runs, parts in ((1, 1), (3, 7), (5, 16)):
            table = np.zeros(4096, dtype=np.uint32)
            par = C.c_int()
            st = L.adsb_selftest_parallel_replay_fix(table.ctypes.data, np.ascontiguousarray(rec).ctypes.data, len(rec),
                                                     runs, parts, 4, mode, out, 8192, C.byref(n), C.byref(par))
            assert st == 0
            from dump1090_rs_amd.context import ModeSMessage
            got = [fs.key(ModeSMessage(bytes(m.msg), int(m.len), float(m.signal_level), int(m.score), int(m.j),
                                       int(m.try_phase), int(m.chunk))) for m in out[: n.value]]
            assert got == want, (mode, runs, parts)


def test_fix_kernels_keep_their_twins_occupancy_and_add_only_the_table(tmp_path):
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
    finally:
        u8.PREFIX = saved
    # FROM_MAG, FUSED, FIELDS, U8: the sparse, dense and one-launch scans of CS16 and CU8, caller magnitudes and
    # their one-launch form
    assert set(fix) == {"Lb0ELb0ELb0ELb0E", "Lb0ELb0ELb1ELb0E", "Lb0ELb1ELb1ELb0E", "Lb0ELb0ELb0ELb1E",
                        "Lb0ELb0ELb1ELb1E", "Lb0ELb1ELb1ELb1E", "Lb1ELb0ELb0ELb0E", "Lb1ELb1ELb1ELb0E"}
    for args, f in sorted(fix.items()):
        a = re.findall(r"Lb([01])E", args)
        twin = fast["Lb%sELb0ELb%sELb%sELb%sE" % tuple(a)]
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (args, f)
        assert f["lds"] == twin["lds"] + 2048, (args, f, twin)
        # occupancy: 4 workgroups of 256 threads a CU for the sparse and dense scans, 2 for the one-launch one
        per_cu = 2 if a[1] == "1" else 4
        assert per_cu * f["lds"] <= 160 * 1024
        assert f["vgpr"] <= (128 if per_cu == 4 else 256) and twin["vgpr"] <= (128 if per_cu == 4 else 256)
        print(args, "insts %+d" % (f["insts"] - twin["insts"]), "sgpr_spill %+d" % (f["sgpr_spill"] - twin["sgpr_spill"]),
              "vgpr %d -> %d" % (twin["vgpr"], f["vgpr"]))
    # and the non-fix scan is what it was
    for args, want in HEAD_CS16.items():
        assert fast[args + "Lb0E"] == want

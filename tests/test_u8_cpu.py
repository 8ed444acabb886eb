"""CU8 (8-bit RTL-SDR IQ) without a GPU: the widening table the library uses, the claim that the reference's
captures are CU8 widened through it, and the fast scan's ISA -- the CU8 instantiations must leave the CS16 ones
exactly as they were.  (include/adsb_hip.h, "8-bit IQ".)"""
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
SCAN_FAST = ROOT / "dump1090_rs_amd" / "csrc" / "adsb_scan_fast.hip"


def t_soapy_numpy() -> np.ndarray:
    """(int16_t)(((float)x - 127.4f) * (1.0f / 128.0f) * 32767.0f), f32 per operation, truncation."""
    x = np.arange(256, dtype=np.float32)
    v = (x - np.float32(127.4)) * np.float32(1.0 / 128.0)
    v = v * np.float32(32767.0)
    assert v.dtype == np.float32
    return np.trunc(v).astype(np.int16)


def test_library_t_soapy_is_the_f32_formula():
    from dump1090_rs_amd import _lib
    L = _lib.lib()
    out = np.zeros(256, dtype=np.int16)
    assert L.adsb_selftest_u8_table(None, out.ctypes.data) == 0
    want = t_soapy_numpy()
    assert np.array_equal(out, want)
    assert len(set(out.tolist())) == 256              # injective: CU8 -> CS16 loses nothing
    assert out[0] == -32613 and out[255] == 32664


def test_golden_captures_are_cu8_widened_through_t_soapy():
    """Every i16 of the three reference captures is an entry of T_soapy, so each narrows to bytes uniquely and
    widens back byte for byte."""
    t = t_soapy_numpy()
    inverse = {int(v): b for b, v in enumerate(t)}
    lut = np.full(65536, -1, dtype=np.int32)
    lut[t.astype(np.int64) + 32768] = np.arange(256)
    golden = json.loads((GOLDEN / "reference_frames.json").read_text())
    assert len(golden["fixtures"]) == 3
    for fx in golden["fixtures"]:
        raw = np.fromfile(GOLDEN / fx["file"], dtype="<i2")
        b = lut[raw.astype(np.int64) + 32768]
        assert (b >= 0).all(), fx["file"]
        assert all(inverse[int(v)] == int(k) for v, k in zip(raw[:64], b[:64]))
        widened = t[b]
        assert widened.tobytes() == raw.tobytes()
        assert 120 <= len(np.unique(raw)) <= 256


# ----------------------------------------------------------------------------------------------- ISA guard
# What hipcc --offload-arch=gfx950 made of every CS16 instantiation of k_scan_fast before CU8 existed (template
# arguments FROM_MAG, SELFTEST, FUSED, FIELDS as mangled): the CU8 parameter is a compile-time one and must not move
# any of them by a single instruction, register, spill or byte of LDS.
HEAD_CS16 = {
    "Lb0ELb0ELb0ELb0E": {"insts": 2392, "sgpr": 100, "vgpr": 102, "accum_offset": 104, "sgpr_spill": 16, "vgpr_spill": 0, "lds": 31232, "scratch": 0},  # sparse stream
    "Lb0ELb0ELb0ELb1E": {"insts": 2430, "sgpr": 100, "vgpr": 104, "accum_offset": 104, "sgpr_spill": 18, "vgpr_spill": 0, "lds": 31872, "scratch": 0},  # dense (FIELDS)
    "Lb0ELb0ELb1ELb1E": {"insts": 7903, "sgpr": 100, "vgpr": 129, "accum_offset": 120, "sgpr_spill": 55, "vgpr_spill": 0, "lds": 50672, "scratch": 0},  # one launch (FUSED)
    "Lb0ELb1ELb0ELb0E": {"insts": 2647, "sgpr": 100, "vgpr": 102, "accum_offset": 104, "sgpr_spill": 24, "vgpr_spill": 0, "lds": 31232, "scratch": 0},  # self-test
    "Lb1ELb0ELb0ELb0E": {"insts": 2003, "sgpr": 100, "vgpr": 83, "accum_offset": 84, "sgpr_spill": 8, "vgpr_spill": 0, "lds": 31232, "scratch": 0},  # caller magnitudes
    "Lb1ELb0ELb1ELb1E": {"insts": 6698, "sgpr": 100, "vgpr": 129, "accum_offset": 96, "sgpr_spill": 33, "vgpr_spill": 0, "lds": 50672, "scratch": 0},  # caller magnitudes, one launch
}
PREFIX = "_ZN4adsb12_GLOBAL__N_111k_scan_fastI"
SUFFIX = "EEvNS_10ScanParamsE"


def kernel_figures(asm: str) -> dict:
    """{mangled template arguments: figures} of every k_scan_fast in a gfx950 .s file."""
    out = {}
    for m in re.finditer(r"^" + PREFIX + r"(\w+?)" + SUFFIX + r":", asm, re.M):
        end = asm.index(".Lfunc_end", m.end())
        body = asm[m.end():end]
        insts = sum(1 for ln in body.splitlines()
                    if ln.startswith("\t") and ln.strip() and not ln.lstrip().startswith((".", ";")))
        out[m.group(1)] = {"insts": insts}
    for m in re.finditer(r"\.amdhsa_kernel " + PREFIX + r"(\w+?)" + SUFFIX + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        d = out[m.group(1)]
        for key, field in (("sgpr", "next_free_sgpr"), ("vgpr", "next_free_vgpr"), ("accum_offset", "accum_offset"),
                           ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size")):
            d[key] = int(re.search(r"\.amdhsa_" + field + r" (\d+)", m.group(2)).group(1))
    for blk in re.split(r"\n  - \.", asm):
        nm = re.search(r"\.name:\s+" + PREFIX + r"(\w+?)" + SUFFIX + r"\s*$", blk, re.M)
        if nm and nm.group(1) in out:
            for key, field in (("sgpr_spill", "sgpr_spill_count"), ("vgpr_spill", "vgpr_spill_count")):
                out[nm.group(1)][key] = int(re.search(r"\." + field + r":\s+(\d+)", blk).group(1))
    return out


def test_cu8_leaves_the_cs16_scan_instantiations_as_they_were(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                    "-save-temps", "-c", str(SCAN_FAST), "-o", str(tmp_path / "scan.o")],
                   check=True, cwd=tmp_path, capture_output=True, timeout=600)
    asm = next(tmp_path.glob("*amdgcn-amd-amdhsa-gfx950.s")).read_text()
    got = kernel_figures(asm)
    for args, want in HEAD_CS16.items():
        # (the CU8 parameter is the last template argument: false in every CS16 instantiation)
        assert got.get(args + "Lb0E") == want, (args, got.get(args + "Lb0E"))
    cu8 = {a: f for a, f in got.items() if a.endswith("Lb1E")}
    # the sparse, dense and one-launch scans of CU8; no self-test and no caller-magnitude forms
    assert set(cu8) == {"Lb0ELb0ELb0ELb0ELb1E", "Lb0ELb0ELb0ELb1ELb1E", "Lb0ELb0ELb1ELb1ELb1E"}
    for args, f in cu8.items():
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (args, f)
        # the widening table (256 f32) is all the LDS they add to their CS16 twins'
        assert f["lds"] == HEAD_CS16[args[:-4]]["lds"] + 1024, (args, f)
    assert len(got) == len(HEAD_CS16) + len(cu8)

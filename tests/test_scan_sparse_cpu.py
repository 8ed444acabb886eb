"""k_scan_sparse without a GPU: the ISA hipcc makes of the sparse stream's folded scan kernel (adsb_scan_fast.hip) set
against the sparse instantiation of k_scan_fast compiled beside it -- no spill, no scratch, the same LDS, no more
registers, fewer instructions -- and its instruction count pinned, so that the next run-time feature of the scan cannot
grow the headline kernel silently: its field gets a constant in k_scan_sparse and a line in sparse_scan_eligible().
Only counts and kernel metadata are looked at, never which instructions appear."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SCAN_FAST = ROOT / "dump1090_rs_amd" / "csrc" / "adsb_scan_fast.hip"
SUFFIX = "EEvNS_10ScanParamsE"
SPARSE_ARGS = "Lb0ELb0ELb0ELb0ELb0E"     # FROM_MAG, SELFTEST, FUSED, FIELDS, U8: all false
PINNED_INSTS = 2125                      # what this commit compiles k_scan_sparse to (k_scan_fast's sparse form: 2392)


def mangled_prefix(name: str) -> str:
    return "_ZN4adsb12_GLOBAL__N_1%d%sI" % (len(name), name)


def kernel_figures(asm: str, name: str) -> dict:
    """{mangled template arguments: figures} of every instantiation of the kernel template `name` in a gfx950 .s file
    (the figures of tests/test_u8_cpu.py: instruction lines, registers, spills, LDS, scratch)."""
    prefix = re.escape(mangled_prefix(name))
    out = {}
    for m in re.finditer(r"^" + prefix + r"(\w+?)" + SUFFIX + r":", asm, re.M):
        body = asm[m.end():asm.index(".Lfunc_end", m.end())]
        insts = sum(1 for ln in body.splitlines()
                    if ln.startswith("\t") and ln.strip() and not ln.lstrip().startswith((".", ";")))
        out[m.group(1)] = {"insts": insts}
    for m in re.finditer(r"\.amdhsa_kernel " + prefix + r"(\w+?)" + SUFFIX + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        d = out[m.group(1)]
        for key, field in (("sgpr", "next_free_sgpr"), ("vgpr", "next_free_vgpr"), ("accum_offset", "accum_offset"),
                           ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size")):
            d[key] = int(re.search(r"\.amdhsa_" + field + r" (\d+)", m.group(2)).group(1))
    for blk in re.split(r"\n  - \.", asm):
        nm = re.search(r"\.name:\s+" + prefix + r"(\w+?)" + SUFFIX + r"\s*$", blk, re.M)
        if nm and nm.group(1) in out:
            for key, field in (("sgpr_spill", "sgpr_spill_count"), ("vgpr_spill", "vgpr_spill_count")):
                out[nm.group(1)][key] = int(re.search(r"\." + field + r":\s+(\d+)", blk).group(1))
    return out


@pytest.fixture(scope="module")
def scan_asm(tmp_path_factory) -> str:
    tmp = tmp_path_factory.mktemp("scan_sparse_isa")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # (the flags of tests/test_u8_cpu.py, which are the library's: dump1090_rs_amd/build.py)
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                    "-save-temps", "-c", str(SCAN_FAST), "-o", str(tmp / "scan.o")],
                   check=True, cwd=tmp, capture_output=True, timeout=600)
    return next(tmp.glob("*amdgcn-amd-amdhsa-gfx950.s")).read_text()


def test_only_the_sparse_form_of_the_folded_kernel_exists(scan_asm):
    assert set(kernel_figures(scan_asm, "k_scan_sparse")) == {SPARSE_ARGS}


def test_the_folded_kernel_spills_nothing_and_is_leaner_than_the_sparse_k_scan_fast(scan_asm):
    lean = kernel_figures(scan_asm, "k_scan_sparse")[SPARSE_ARGS]
    fast = kernel_figures(scan_asm, "k_scan_fast")[SPARSE_ARGS]
    print("k_scan_sparse", lean)
    print("k_scan_fast  ", fast)
    assert lean["sgpr_spill"] == 0 and lean["vgpr_spill"] == 0 and lean["scratch"] == 0, lean
    assert lean["lds"] == fast["lds"], (lean, fast)          # the same workgroups per CU by LDS ...
    assert lean["vgpr"] <= fast["vgpr"], (lean, fast)        # ... and by registers: scan_resident_blocks() holds for both
    assert lean["insts"] < fast["insts"], (lean, fast)
    assert lean["insts"] == PINNED_INSTS, lean

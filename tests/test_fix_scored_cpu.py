"""Device-side scoring of repaired trials, the part that needs no GPU: the conditions tests/test_gpu_fix_scored.py's
ordered stream must meet (from the CPU restatement alone), the scoring kernels' ISA for gfx950, and the new entry point's
declarations."""
import re
import shutil
import subprocess

from tests import fix2_support as f2
from tests import fix_scored_support as S
from tests.conftest import ROOT

CSRC = ROOT / "dump1090_rs_amd" / "csrc"
# k_score / k_emit before they scored repaired trials (the commit "Test the preamble gates and bit slicer at exact ties
# and thresholds"), for the print below -- not a pin
BEFORE = {"k_score": {"insts": 761, "vgpr": 36, "sgpr": 61, "lds": 8, "scratch": 0},
          "k_emit": {"insts": 744, "vgpr": 46, "sgpr": 60, "lds": 12368, "scratch": 0}}


def test_the_ordered_stream_decides_by_order_inside_a_pass():
    """From the restatement alone: the early copies yield no message, the late ones 1200 / 1100 with the clean bytes (at
    least 20 of each class), the second call without a flush brings the early ones back, and the stream holds positions
    where a clean trial phase competes with a one-bit one -- which the clean one wins."""
    iq, want = S.order_stream()
    assert len(iq) == S.N_BUFFERS * S.CHUNK and S.N_BUFFERS > 16
    r = f2.Restated(f2.FIX2)
    first = r.demod_iq(iq)
    S.check_first_call(first, want)
    second = r.demod_iq(iq)
    S.check_second_call(second, want)
    assert first != second
    # dense: at least 8 trial records a buffer is what makes a context order and score on the device
    per_buffer = {}
    for k in first:
        per_buffer[k[4]] = per_buffer.get(k[4], 0) + 1
    assert len(per_buffer) == S.N_BUFFERS and min(per_buffer.values()) >= 8
    competing = S.competing_positions(iq, first)
    assert len(competing) >= 3 and all(k[1] in S.CLEAN for k in competing), len(competing)
    # mode 1: the one-bit classes as above, no two-bit repair anywhere
    r1 = f2.Restated(1)
    one = r1.demod_iq(iq)
    assert not any(k[1] == 1100 for k in one)
    got = S.by_slot(one)
    for kind in S.ONE_BIT:
        slots = [s for s, (k, _) in want.items() if k == kind]
        assert sum(all(m == (want[s][1], 1200) for m in got.get(s, [])) and s in got for s in slots) >= 20, kind
    for s, (kind, _) in want.items():
        if kind in ("early1", "early2", "only18"):
            assert s not in got, (s, kind)


def test_the_victim_streams_tell_a_damaged_address_from_a_heard_one():
    """The capture tests/test_gpu_fix_scored.py sends through adsb_multi with a short fresh list, from the restatement
    alone: behind the ordered stream, whose damaged copies carry the one-bit neighbours of LATE and EARLY in their
    address field, those very addresses are unknown until their own first clean frame."""
    import numpy as np
    victims = S.damaged_addresses()
    assert len(victims) == 48 and len(set(victims)) == 48
    parts = [S.order_stream(), S.victim_stream(9900, victims[:24]), S.victim_stream(9950, victims[24:])]
    iq = np.concatenate([p[0] for p in parts])
    # the ordered stream does carry them: a damaged copy whose sliced address is each of LATE's neighbours
    carried = {int.from_bytes(f[1:4], "big") for f in (S.fs.flip(S.synth.df17_frame(S.LATE, S.ME), b) for b in S.ADDRESS_BITS)}
    assert carried == set(victims[:24])
    for mode in (f2.FIX2, 1):
        got = f2.Restated(mode).demod_iq(iq)
        S.check_victims(got, parts[1][1], S.N_BUFFERS, mode)
        S.check_victims(got, parts[2][1], 2 * S.N_BUFFERS, mode)


def kernel_figures(asm: str, kernel: str) -> dict:
    m = re.search(r"^(_ZN4adsb12_GLOBAL__N_1\d+" + kernel + r"E[^:\n]*):", asm, re.M)
    assert m, kernel
    body = asm[m.end():asm.index(".Lfunc_end", m.end())]
    insts = sum(1 for ln in body.splitlines() if ln.startswith("\t") and ln.strip() and not ln.lstrip().startswith((".", ";")))
    hsa = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
    field = lambda f: int(re.search(r"\.amdhsa_" + f + r" (\d+)", hsa).group(1))
    return {"insts": insts, "vgpr": field("next_free_vgpr"), "sgpr": field("next_free_sgpr"),
            "lds": field("group_segment_fixed_size"), "scratch": field("private_segment_fixed_size"), "body": body}


def test_scoring_kernels_cross_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for src in ("adsb_aux.hip", "adsb_scan_simple.hip"):
        subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wextra",
                        "-Werror", "-save-temps", "-c", str(CSRC / src), "-o", str(tmp_path / (src + ".o"))],
                       check=True, cwd=tmp_path, capture_output=True, timeout=600)
    asm = next(tmp_path.glob("adsb_aux*amdgcn-amd-amdhsa-gfx950.s")).read_text()
    for kernel in ("k_score", "k_emit", "k_fix_lookup"):
        f = kernel_figures(asm, kernel)
        body = f.pop("body")
        print(kernel, "before", BEFORE.get(kernel), "now", f)
        assert f["scratch"] == 0, (kernel, f)
        assert "scratch_" not in body, kernel
    assert kernel_figures(asm, "k_emit")["lds"] == BEFORE["k_emit"]["lds"]


def test_the_lookup_entry_point_is_declared_everywhere():
    header = (ROOT / "include" / "adsb_hip.h").read_text()
    assert re.search(r"int adsb_selftest_fix_lookup\(adsb_ctx \*ctx, const uint32_t \*residuals, size_t n, int mode, uint32_t \*out\);", header)
    assert "adsb_selftest_fix_lookup.argtypes" in (ROOT / "dump1090_rs_amd" / "_lib.py").read_text()
    rust = (ROOT / "integration" / "rust" / "src" / "hip_ffi.rs").read_text()
    assert "pub fn adsb_selftest_fix_lookup(ctx: *mut AdsbCtx, residuals: *const u32, n: usize, mode: c_int, out: *mut u32) -> c_int;" in rust

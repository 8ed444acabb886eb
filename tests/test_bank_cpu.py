"""Resampler banks (include/adsb_hip.h, "Resampler banks") without a GPU: the ABI in the header, the library, the Rust
shim and the Python bindings, the argument checks that need no device, the per-stream count arithmetic against the numpy
restatement (tests/resamp_support.py), and the new kernels' code-object metadata for gfx950."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np

from tests import resamp_support as rs
from tests import test_rust_shim as shim
from tests.conftest import ROOT

HEADER = ROOT / "include" / "adsb_hip.h"
FFI = ROOT / "integration" / "rust" / "src" / "hip_ffi.rs"
CSRC = ROOT / "dump1090_rs_amd" / "csrc"
NAMES = ("adsb_bank_create", "adsb_bank_destroy", "adsb_bank_streams", "adsb_bank_reset", "adsb_bank_consumed",
         "adsb_bank_out_count", "adsb_bank_inputs_for", "adsb_bank_run_device", "adsb_bank_set_mixer", "adsb_bank_get_mixer",
         "adsb_bank_set_scale", "adsb_bank_get_scale", "adsb_bank_selftest_depth")


def header_prototypes():
    """name -> (Rust parameter types, Rust return type) of every adsb_bank_* prototype of the header
    (tests/test_resamp_cpu.py's parser with this family's pattern)."""
    text = shim.strip_comments(HEADER.read_text())
    out = {}
    for m in re.finditer(r"(?:ADSB_MUST_CHECK|extern)?\s*\b(int|void|uint32_t|float)\s+(adsb_bank_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        params = []
        if args and args != "void":
            for a in args.split(","):
                params.append(shim.c_type_to_rust(re.match(r"^(.*?)(\w+)$", a.strip()).group(1).strip()))
        out[name] = (params, None if ret == "void" else shim.c_type_to_rust(ret))
    return out


def rust_prototypes():
    text = shim.strip_comments(FFI.read_text())
    out = {}
    for f in re.finditer(r"pub\s+fn\s+(adsb_bank_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", text, flags=re.S):
        args = " ".join(f.group(2).split())
        params = [" ".join(a.split(":", 1)[1].split()) for a in args.split(",") if a.strip()]
        out[f.group(1)] = (params, " ".join(f.group(3).split()) if f.group(3) else None)
    return out


def test_the_functions_are_declared_exported_and_bound(hip_lib, monkeypatch):
    import dump1090_rs_amd as pkg
    monkeypatch.setitem(shim.BASE, "adsb_bank", "AdsbBank")
    hdr, ffi = header_prototypes(), rust_prototypes()
    assert sorted(hdr) == sorted(NAMES)
    assert sorted(hdr) == sorted(ffi)
    for name in hdr:
        assert hdr[name] == ffi[name], f"{name}: header {hdr[name]} vs hip_ffi.rs {ffi[name]}"
        assert hasattr(hip_lib, name), f"{name} is not exported"
        assert getattr(hip_lib, name).argtypes is not None, f"{name} has no ctypes prototype"
        assert len(getattr(hip_lib, name).argtypes) == len(hdr[name][0]), name
    assert hdr["adsb_bank_create"][0] == ["*mut AdsbCtx", "u32", "u32", "u32", "*const i16", "u32", "u32", "*mut *mut AdsbBank"]
    assert hdr["adsb_bank_run_device"] == (["*mut AdsbBank", "c_int", "u32", "*const u32", "*const *const c_void", "*const usize",
                                            "*const *mut c_void", "*const usize", "*mut usize"], "c_int")
    assert hdr["adsb_bank_inputs_for"] == (["*const AdsbBank", "u32", "usize", "*mut usize", "*mut usize"], "c_int")
    assert hdr["adsb_bank_selftest_depth"] == ([], "u32")
    text = HEADER.read_text()
    assert "typedef struct adsb_bank adsb_bank;" in text and re.search(r"#define\s+ADSB_BANK_ALL\s+0xFFFFFFFFu", text)
    # the header is written so that the shim's own test does not see the family: every prototype behind a marker, none in
    # the first block of hip_ffi.rs, no anonymous struct
    assert not [n for n in shim.header_functions() if n.startswith("adsb_bank_")]
    assert not [n for n in shim.rust_functions() if n.startswith("adsb_bank_")]
    assert "ResamplerBank" in pkg.__all__ and hasattr(pkg, "ResamplerBank")
    assert hasattr(pkg.Context, "resampler_bank")
    for method in ("reset", "consumed", "out_count", "inputs_for", "run_device", "set_mixer", "mixer_period", "set_scale", "scale",
                   "close", "__enter__", "__exit__"):
        assert hasattr(pkg.ResamplerBank, method)
    assert pkg.ResamplerBank.ALL == 0xFFFFFFFF
    assert hip_lib.adsb_bank_selftest_depth() >= 2
    # ... and no call of the family matches a pattern the decimator's, resampler's, mixer's or format tests pin
    stripped = shim.strip_comments(text)
    for family, count in [("resamp", 10), ("decim", 8), ("mix", 6), ("fmt", 4)]:
        names = set(re.findall(r"\b(adsb_" + family + r"_\w+)\s*\(", stripped))
        assert len(names) == count, (family, sorted(names))


def test_argument_checks_that_need_no_device(hip_lib):
    from dump1090_rs_amd import _lib
    INV = _lib.ADSB_ERR_INVALID
    taps = (C.c_int16 * 1)(1)
    h = C.c_void_p(0x1234)
    assert hip_lib.adsb_bank_create(None, 1, 1, 2, taps, 1, 0, C.byref(h)) == INV
    assert h.value is None   # (and the out-pointer does not keep a stale handle)
    fake_ctx = C.c_void_p(0x1000)   # never dereferenced: every check below comes before the device is touched
    assert hip_lib.adsb_bank_create(fake_ctx, 1, 1, 2, taps, 1, 0, None) == INV
    assert hip_lib.adsb_bank_create(fake_ctx, 1, 1, 2, None, 1, 0, C.byref(h)) == INV
    one = [1]
    for N, L, M, t, s, why in [
            (0, 1, 2, one, 0, "no stream"), (16385, 1, 2, one, 0, "N > ADSB_MAX_RECEIVERS"), (0xFFFFFFFF, 1, 2, one, 0, "N = ALL"),
            # adsb_resamp_create's limits, every one of them
            (3, 2, 4, one, 0, "gcd != 1"), (3, 0, 1, one, 0, "L = 0"), (3, 1, 0, one, 0, "M = 0"), (3, 129, 128, one, 0, "L > 128"),
            (3, 1, 129, one, 0, "M > 128"), (3, 3, 1, one, 0, "L > 2 M"), (3, 1, 17, one, 0, "M > 16 L"),
            (3, 1, 2, [1] * 513, 0, "K > 512"), (3, 16, 17, [1] * 4097, 0, "T > 4096"),
            (3, 2, 3, [1, 32767, 1, 32767, 1, 1], 0, "a phase at 65535"), (3, 1, 2, [], 0, "T = 0"), (3, 1, 2, one, 17, "s = 17")]:
        a = np.ascontiguousarray(list(t) + [0], dtype=np.int16)
        h = C.c_void_p(0x1234)
        assert hip_lib.adsb_bank_create(fake_ctx, N, L, M, a.ctypes.data, len(a) - 1, s, C.byref(h)) == INV, why
        assert h.value is None, why
    n, p = C.c_size_t(), C.c_uint64()
    assert hip_lib.adsb_bank_streams(None) == 0
    assert hip_lib.adsb_bank_reset(None, 0) == INV and hip_lib.adsb_bank_reset(None, 0xFFFFFFFF) == INV
    assert hip_lib.adsb_bank_consumed(None, 0, C.byref(p)) == INV
    assert hip_lib.adsb_bank_out_count(None, 0, 1, C.byref(n)) == INV
    assert hip_lib.adsb_bank_inputs_for(None, 0, 1, C.byref(n), C.byref(n)) == INV
    assert hip_lib.adsb_bank_run_device(None, 0, 0, None, None, None, None, None, None) == INV
    assert hip_lib.adsb_bank_set_mixer(None, None, 0) == INV
    assert hip_lib.adsb_bank_set_scale(None, 1.0) == INV
    assert hip_lib.adsb_bank_get_mixer(None) == 0 and hip_lib.adsb_bank_get_scale(None) == 0.0
    hip_lib.adsb_bank_destroy(None)


def test_inputs_for_agrees_with_the_restatement(hip_lib):
    """adsb_bank_inputs_for and adsb_bank_out_count are, per stream, the host arithmetic of the single resampler
    (adsb_resamp_host.h: plan, inputs_for), which adsb_resamp_plan exposes without a handle: over random (L, M, P, n),
    L > M included, the fewest inputs and what they give equal tests/resamp_support.py's Python integers.  A bank itself
    needs a device, and its P moves only by runs: tests/test_gpu_bank.py holds the bank's own two calls to the same
    restatement at every P its streams reach."""
    from dump1090_rs_amd import _lib
    assert hasattr(hip_lib, "adsb_bank_inputs_for") and hasattr(hip_lib, "adsb_bank_out_count")
    rng = np.random.default_rng(21)
    ratios = rs.accepted_ratios()
    up = 0
    for i in range(3000):
        L, M = ratios[int(rng.integers(len(ratios)))]
        P = int(rng.integers(0, 1 << 20)) if i % 2 else (1 << 44) - int(rng.integers(0, 1 << 16))
        want = int(rng.choice([1, 2, 5, 17, 300, 131072, int(rng.integers(1, 1 << 24))]))
        n_in = rs.inputs_for(L, M, P, want)
        made = rs.out_count(L, M, P, n_in)
        first, n = C.c_uint64(), C.c_uint64()
        assert hip_lib.adsb_resamp_plan(L, M, P, n_in, C.byref(first), C.byref(n)) == _lib.ADSB_OK
        assert n.value == made and want <= made <= want + (L > M)
        assert rs.out_count(L, M, P, n_in - 1) < want   # the fewest
        up += L > M
    assert up > 300
    assert rs.inputs_for(6, 5, 0, 0) == 0


def kernel_metadata(asm: str, kernel: str):
    """[(mangled name, {field: value})] of every instantiation of `kernel` in the code object's metadata."""
    out = []
    for m in re.finditer(r"\.name:\s+(_ZN4adsb12_GLOBAL__N_1\d+" + kernel + r"I\S*)\n(.*?)\.wavefront_size", asm, re.S):
        fields = {f: int(re.search(r"\." + f + r":\s+(\d+)", m.group(2)).group(1))
                  for f in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "vgpr_count")}
        out.append((m.group(1), fields))
    return out


def test_the_new_kernels_cross_compile_for_gfx950_without_scratch(tmp_path):
    from dump1090_rs_amd import build
    assert CSRC / "adsb_bank.cpp" in build.SOURCES and CSRC / "adsb_resamp_body.inc" in build.HEADERS
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in build.FLAGS if f != "-shared"]
    subprocess.run([hipcc, *flags, "-Werror", "-save-temps", "-c", str(CSRC / "adsb_resamp.hip"), "-o", str(tmp_path / "resamp.o")],
                   check=True, cwd=tmp_path, capture_output=True, timeout=600)
    asm = next(tmp_path.glob("adsb_resamp*amdgcn-amd-amdhsa-gfx950.s")).read_text()
    for kernel in ("k_resamp_bank", "k_resamp_bank_history"):
        found = kernel_metadata(asm, kernel)
        assert len(found) == 8, (kernel, [n for n, _ in found])   # four formats, with and without the mixer
        for name, f in found:
            print(name, f)
            assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
    # ... and beside the kernels they share a body with, not in their place
    assert len(kernel_metadata(asm, "k_resamp")) == 8 and len(kernel_metadata(asm, "k_resamp_history")) == 8

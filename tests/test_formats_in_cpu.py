"""CF32 and REAL16 input of the decimator and the resampler (include/adsb_hip.h, "Sample formats") without a GPU: the
ABI in the header, the library, the Rust shim and the Python package, every edge value of q spelled out, adsb_feed's
usage, the argument checks that need no device, and the real-sample construction the GPU tests feed the device with.
(The scale's accepted range needs a handle, and a handle needs a device: tests/test_gpu_formats_in.py asserts it.)"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from tests import formats_in_support as fi
from tests import mix_support as ms
from tests import test_rust_shim as shim
from tests.conftest import ROOT

HEADER = ROOT / "include" / "adsb_hip.h"
FFI = ROOT / "integration" / "rust" / "src" / "hip_ffi.rs"
NAMES = ("adsb_fmt_set_scale_decim", "adsb_fmt_set_scale_resamp", "adsb_fmt_get_scale_decim", "adsb_fmt_get_scale_resamp")
PATTERN = r"adsb_fmt_\w+"


def header_prototypes():
    text = shim.strip_comments(HEADER.read_text())
    out = {}
    for m in re.finditer(r"\b(int|float)\s+(" + PATTERN + r")\s*\(([^)]*)\)\s*;", text, flags=re.S):
        args = " ".join(m.group(3).split())
        params = [shim.c_type_to_rust(re.match(r"^(.*?)(\w+)$", a.strip()).group(1).strip()) for a in args.split(",")]
        out[m.group(2)] = (params, shim.c_type_to_rust(m.group(1)))
    return out


def rust_prototypes():
    text = shim.strip_comments(FFI.read_text())
    out = {}
    for f in re.finditer(r"pub\s+fn\s+(" + PATTERN + r")\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", text, flags=re.S):
        params = [" ".join(a.split(":", 1)[1].split()) for a in " ".join(f.group(2).split()).split(",") if a.strip()]
        out[f.group(1)] = (params, " ".join(f.group(3).split()) if f.group(3) else None)
    return out


def test_the_abi_is_declared_exported_and_bound(hip_lib, monkeypatch):
    import dump1090_rs_amd as pkg
    from dump1090_rs_amd import _lib
    monkeypatch.setitem(shim.BASE, "adsb_decim", "AdsbDecim")
    monkeypatch.setitem(shim.BASE, "adsb_resamp", "AdsbResamp")
    hdr, ffi = header_prototypes(), rust_prototypes()
    assert sorted(hdr) == sorted(NAMES) == sorted(ffi)
    for name in hdr:
        assert hdr[name] == ffi[name], f"{name}: header {hdr[name]} vs hip_ffi.rs {ffi[name]}"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hdr["adsb_fmt_set_scale_decim"] == (["*mut AdsbDecim", "f32"], "c_int")
    assert hdr["adsb_fmt_get_scale_resamp"] == (["*const AdsbResamp"], "f32")
    assert hip_lib.adsb_fmt_get_scale_decim.restype is C.c_float and hip_lib.adsb_fmt_set_scale_resamp.argtypes[1] is C.c_float
    text, rust = HEADER.read_text(), FFI.read_text()
    for name, value in (("ADSB_DECIM_CF32", 2), ("ADSB_DECIM_REAL16", 3)):
        assert re.search(rf"#define {name}\s+{value}\b", text) and f"pub const {name}: i32 = {value};" in rust
        assert getattr(_lib, name) == value == getattr(pkg, name) and name in pkg.__all__
    for name, alias in (("ADSB_RESAMP_CF32", "ADSB_DECIM_CF32"), ("ADSB_RESAMP_REAL16", "ADSB_DECIM_REAL16")):
        assert re.search(rf"#define {name}\s+{alias}\b", text) and f"pub const {name}: i32 = {alias};" in rust
    assert (fi.CS16, fi.U8, fi.CF32, fi.REAL16) == (_lib.ADSB_DECIM_CS16, _lib.ADSB_DECIM_8BIT, _lib.ADSB_DECIM_CF32, _lib.ADSB_DECIM_REAL16)
    for cls in (pkg.Decimator, pkg.Resampler):
        assert hasattr(cls, "set_scale") and isinstance(cls.scale, property)
    assert hasattr(pkg.Context, "converter")
    # the families of the decimator and the resampler gained no function
    assert "Sample formats" in text and text.index("Sample formats --") > text.index("Frequency shift --")


def test_argument_errors_that_need_no_device(hip_lib):
    from dump1090_rs_amd import _lib
    n = C.c_size_t()
    assert hip_lib.adsb_fmt_set_scale_decim(None, 32768.0) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_fmt_set_scale_resamp(None, 1.0) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_fmt_get_scale_decim(None) == 0.0 and hip_lib.adsb_fmt_get_scale_resamp(None) == 0.0
    for fmt in (fi.CF32, fi.REAL16):
        assert hip_lib.adsb_decim_run_device(None, fmt, None, 0, None, 0, C.byref(n)) == _lib.ADSB_ERR_INVALID
        assert hip_lib.adsb_resamp_demod_iq(None, fmt, None, 0, None, 0, C.byref(n)) == _lib.ADSB_ERR_INVALID


# ----------------------------------------------------------------------------------------------- q, value by value
def test_every_edge_value_of_q_is_what_the_definition_says():
    x = fi.edge_values()
    assert np.isnan(x[18]) and np.signbit(x[22]) and x[22] == 0 and 0 < x[23] < np.finfo(np.float32).tiny
    for column, g in ((1, fi.DEFAULT_SCALE), (2, fi.G2)):
        want = [e[column] for e in fi.Q_EDGES]
        assert fi.q(x, g).tolist() == want
        assert [fi.q_exact(float(v), g) for v in x] == want
    # the ties are ties: the binary32 product is exactly k + 1/2
    for i, k in ((0, 0.5), (2, 1.5), (4, 2.5), (6, 32767.5)):
        assert float(x[i] * np.float32(32768)) == k and float(x[i + 1] * np.float32(32768)) == -k
    for i, k in ((8, 0.5), (10, 1.5), (12, 2.5), (14, 32767.5)):
        assert float(x[i] * np.float32(fi.G2)) == k and float(x[i + 1] * np.float32(fi.G2)) == -k
    assert fi.G2 == float.fromhex("0x1.f40cccp+9") and fi.G2 != 1000.1


def test_q_agrees_with_exact_arithmetic_on_random_floats():
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([bits.view(np.float32), rng.uniform(-1.2, 1.2, 4000).astype(np.float32),
                        (rng.integers(-70000, 70000, 2000) / 65536).astype(np.float32)])
    for g in (fi.DEFAULT_SCALE, fi.G2, 1.0, 2.0 ** 31, float(np.float32(1e-3))):
        assert fi.q(x, g).tolist() == [fi.q_exact(float(v), g) for v in x]
    # a subnormal gives 0 at the largest scale whether or not it is flushed
    sub = np.array([fi.F32_MAX_SUBNORMAL, -fi.F32_MAX_SUBNORMAL, float.fromhex("0x1p-149")], np.float32)
    assert fi.q(sub, 2.0 ** 31).tolist() == [0, 0, 0] and fi.q(np.zeros(3, np.float32), 2.0 ** 31).tolist() == [0, 0, 0]


def test_cs16_through_cf32_is_the_identity():
    x = np.array([[-32768, 32767], [0, -1], [1, 12345]], np.int16)
    f = fi.cs16_as_cf32(x)
    assert f.dtype == np.float32 and np.array_equal(fi.to_cs16(f, fi.CF32), x)
    assert np.array_equal(fi.to_cs16(np.array([5, -7, 0], np.int16), fi.REAL16), [[5, 0], [-7, 0], [0, 0]])


# ----------------------------------------------------------------------------------------------- adsb_feed
def test_adsb_feed_new_formats_are_usage_errors_without_a_filter(hip_lib):
    feed = str(ROOT / "dump1090_rs_amd" / "adsb_feed")
    for args in (["--format", "cf32", "x.iq"], ["--format", "s16real", "x.iq"], ["--format", "cf32", "--scale", "2", "x.iq"],
                 ["--scale", "2", "--decimate", "4", "x.iq"], ["--format", "s16real", "--scale", "2", "--decimate", "4", "x.iq"],
                 ["--format", "cu8", "--scale", "2", "--resample", "6/25", "x.iq"],
                 ["--format", "cf32", "--scale", "0", "--decimate", "4", "x.iq"], ["--format", "cf32", "--scale", "nan", "--decimate", "4", "x.iq"],
                 ["--format", "cf32", "--scale", "inf", "--decimate", "4", "x.iq"], ["--format", "cf32", "--scale", "-1", "--decimate", "4", "x.iq"],
                 ["--format", "cf32", "--scale", "4294967296", "--resample", "1/1", "x.iq"],
                 ["--format", "cf32", "--scale", "abc", "--resample", "1/1", "x.iq"], ["--format", "f32", "--decimate", "4", "x.iq"]):
        r = subprocess.run([feed, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr and "[--scale G]" in r.stderr, args
    r = subprocess.run([feed, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--format cs16|cu8|cf32|s16real]" in r.stderr
    assert "[--decimate D | --resample L/M] [--shift HZ] [--scale G]" in r.stderr


# ----------------------------------------------------------------------------------------------- real samples
def test_the_real_carrier_decimates_to_the_capture_and_the_oracle_finds_the_reference_frames(oracle_mod, golden, fixture_iq):
    """r[4 n] = re x[n], r[4 n - 1] = im x[n] through the exact table of 3/4 turn, D = 4, taps [1, 1], shift 0 is x with
    the im of sample 0 zeroed -- in the restatement -- and zeroing that one component changes no capture's frame list."""
    back = ms.rotation(3)
    for fx in golden["fixtures"]:
        cap = fixture_iq[fx["file"]]
        r = fi.real_carrier(cap)
        assert r.dtype == np.int16 and len(r) == 4 * len(cap) - 3 and cap.min() > -32768
        y = ms.decimate(fi.real_to_cs16(r), [1, 1], 4, 0, back)
        want = cap.copy()
        want[0, 1] = 0
        assert np.array_equal(y, want)
        frames, _ = oracle_mod.Oracle().demod_iq(y)
        assert [f["buffer"].hex() for f in frames] == fx["frames"]
        assert [int(f["j"]) for f in frames] == fx["j"]

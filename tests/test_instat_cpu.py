"""Input statistics (include/adsb_hip.h, "Input statistics") without a GPU: the ABI in the header, the library, the Rust
shim and the Python bindings; the record's layout in C, ctypes, numpy and Rust; adsb_input_bin on every int16;
adsb_input_summary on hand-made records; the argument checks that need no device; and the kernels' code-object metadata
for gfx950."""
import ctypes as C
import math
import re
import shutil
import subprocess

import numpy as np

from tests import instat_support as ist
from tests import test_rust_shim as shim
from tests.conftest import ROOT

HEADER = ROOT / "include" / "adsb_hip.h"
FFI = ROOT / "integration" / "rust" / "src" / "hip_ffi.rs"
CSRC = ROOT / "dump1090_rs_amd" / "csrc"
KINDS = ("decim", "resamp", "bank")
NAMES = tuple(f"adsb_instat_{call}_{kind}" for call in ("set", "get", "fetch", "selftest_launches") for kind in KINDS) + (
    "adsb_input_bin", "adsb_input_summary", "adsb_instat_selftest_geometry")
PATTERN = r"adsb_(?:instat|input)_\w+"
EXTRA = {"adsb_decim": "AdsbDecim", "adsb_resamp": "AdsbResamp", "adsb_bank": "AdsbBank", "adsb_input_stats": "AdsbInputStats",
         "adsb_input_summary_t": "AdsbInputSummary", "int64_t": "i64"}
RUST_SIZE = dict(shim.RUST_SIZE, i64=8)


def header_prototypes():
    """name -> (Rust parameter types, Rust return type) of every prototype of the family in the header
    (tests/test_bank_cpu.py's parser with this family's pattern)."""
    text = shim.strip_comments(HEADER.read_text())
    out = {}
    for m in re.finditer(r"(?:ADSB_MUST_CHECK|extern)?\s*\b(int|void|uint32_t|uint64_t|float)\s+(" + PATTERN + r")\s*\(([^)]*)\)\s*;", text,
                         flags=re.S):
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
    for f in re.finditer(r"pub\s+fn\s+(" + PATTERN + r")\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", text, flags=re.S):
        args = " ".join(f.group(2).split())
        params = [" ".join(a.split(":", 1)[1].split()) for a in args.split(",") if a.strip()]
        out[f.group(1)] = (params, " ".join(f.group(3).split()) if f.group(3) else None)
    return out


def header_struct(name: str):
    """[(field, Rust type)] of `typedef struct <name> { ... } <name>;` in the header."""
    text = shim.strip_comments(HEADER.read_text()).replace("ADSB_INPUT_BINS", "17")
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for n in names.split(","):
            m = re.match(r"^(\w+)(?:\[(\w+)\])?$", n.strip())
            rt = shim.BASE[ctype]
            fields.append((m.group(1), f"[{rt}; {m.group(2)}]" if m.group(2) else rt))
    return fields


def layout(fields):
    off, offsets, align_max = 0, [], 1
    for _, t in fields:
        arr = re.match(r"^\[(\w+); (\d+)\]$", t)
        elem, count = (arr.group(1), int(arr.group(2))) if arr else (t, 1)
        a = RUST_SIZE[elem]
        off = (off + a - 1) // a * a
        offsets.append(off)
        off += a * count
        align_max = max(align_max, a)
    return offsets, (off + align_max - 1) // align_max * align_max


def test_the_functions_are_declared_exported_and_bound(hip_lib, monkeypatch):
    import dump1090_rs_amd as pkg
    for k, v in EXTRA.items():
        monkeypatch.setitem(shim.BASE, k, v)
    hdr, ffi = header_prototypes(), rust_prototypes()
    assert sorted(hdr) == sorted(NAMES)
    assert sorted(hdr) == sorted(ffi)
    for name in hdr:
        assert hdr[name] == ffi[name], f"{name}: header {hdr[name]} vs hip_ffi.rs {ffi[name]}"
        assert hasattr(hip_lib, name), f"{name} is not exported"
        assert getattr(hip_lib, name).argtypes is not None, f"{name} has no ctypes prototype"
        assert len(getattr(hip_lib, name).argtypes) == len(hdr[name][0]), name
    assert hdr["adsb_instat_set_decim"] == (["*mut AdsbDecim", "c_int"], "c_int")
    assert hdr["adsb_instat_get_resamp"] == (["*const AdsbResamp"], "c_int")
    assert hdr["adsb_instat_fetch_bank"] == (["*mut AdsbBank", "u32", "u32", "*mut AdsbInputStats"], "c_int")
    assert hdr["adsb_input_bin"] == (["i16"], "c_int")
    assert hdr["adsb_input_summary"] == (["*const AdsbInputStats", "usize", "*mut AdsbInputSummary"], "c_int")
    assert hdr["adsb_instat_selftest_geometry"] == (["c_int", "*mut u32", "*mut u32"], "c_int")
    assert hdr["adsb_instat_selftest_launches_bank"] == (["*const AdsbBank"], "u64")
    # every call that returns a status must be checked
    text = HEADER.read_text()
    for name, (_, ret) in hdr.items():
        if ret == "c_int" and name != "adsb_input_bin":
            assert re.search(r"ADSB_MUST_CHECK\s+int\s+" + name + r"\s*\(", text), name
    # the header is written so that the shim's own test does not see the family (every prototype behind a marker, no
    # anonymous struct), and no call of it matches a pattern the other families' tests pin
    assert not [n for n in shim.header_functions() if re.fullmatch(PATTERN, n)]
    assert not [n for n in shim.rust_functions() if re.fullmatch(PATTERN, n)]
    stripped = shim.strip_comments(text)
    for family, count in [("resamp", 10), ("decim", 8), ("mix", 6), ("fmt", 4), ("bank", 13)]:
        names = set(re.findall(r"\b(adsb_" + family + r"_\w+)\s*\(", stripped))
        assert len(names) == count, (family, sorted(names))
    assert "input_summary" in pkg.__all__ and hasattr(pkg, "input_summary")
    for cls in (pkg.Decimator, pkg.Resampler, pkg.ResamplerBank):
        for method in ("set_input_stats", "input_stats", "input_stats_enabled"):
            assert hasattr(cls, method), (cls, method)


def test_the_record_has_one_layout_in_c_ctypes_numpy_and_rust(hip_lib, monkeypatch, tmp_path):
    from dump1090_rs_amd import _lib, context
    for k, v in EXTRA.items():
        monkeypatch.setitem(shim.BASE, k, v)
    rust = shim.rust_structs()
    for cname, rname, ct, size in [("adsb_input_stats", "AdsbInputStats", _lib.AdsbInputStats, 208),
                                   ("adsb_input_summary_t", "AdsbInputSummary", _lib.AdsbInputSummary, 80)]:
        hdr = header_struct(cname)
        assert rust[rname] == hdr, f"{rname}: field order / types differ between hip_ffi.rs and the header"
        offsets, total = layout(hdr)
        assert total == C.sizeof(ct) == size
        assert [f[0] for f in ct._fields_] == [f[0] for f in hdr]
        assert offsets == [getattr(ct, f[0]).offset for f in ct._fields_]
    for dt in (ist.DTYPE, context.INPUT_STATS_DTYPE):
        assert dt.itemsize == 208 and list(dt.names) == [f[0] for f in _lib.AdsbInputStats._fields_]
        assert [dt.fields[n][1] for n in dt.names] == [getattr(_lib.AdsbInputStats, n).offset for n in dt.names]
    assert _lib.ADSB_INPUT_BINS == ist.BINS == 17 and re.search(r"#define\s+ADSB_INPUT_BINS\s+17\b", HEADER.read_text())
    # ... and in C itself
    src = tmp_path / "layout.c"
    checks = "\n".join(f'_Static_assert(offsetof(adsb_input_stats, {n}) == {getattr(_lib.AdsbInputStats, n).offset}, "{n}");'
                       for n, _ in _lib.AdsbInputStats._fields_)
    src.write_text('#include <stddef.h>\n#include "adsb_hip.h"\n_Static_assert(sizeof(adsb_input_stats) == 208, "size");\n'
                   '_Static_assert(sizeof(adsb_input_summary_t) == 80, "size");\n' + checks + "\nint main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src), "-o", str(tmp_path / "layout.o")],
                   check=True, capture_output=True, timeout=120)


def test_input_bin_on_every_int16(hip_lib):
    v = np.arange(-32768, 32768, dtype=np.int64)
    got = np.array([hip_lib.adsb_input_bin(int(x)) for x in v])
    want = np.where(v == 0, 0, 1 + np.floor(np.log2(np.maximum(np.abs(v), 1)))).astype(np.int64)
    assert np.array_equal(got, want) and np.array_equal(want, ist.input_bin(v))
    assert got.min() == 0 and got.max() == 16 and got[0] == 16 and got[32768] == 0 and got[32768 + 1] == 1 and got[-1] == 15
    assert (got == 16).sum() == 1 and (got == 0).sum() == 1


def summary_of(hip_lib, records):
    from dump1090_rs_amd import input_summary
    return input_summary(records)


def test_input_summary(hip_lib):
    from dump1090_rs_amd import _lib
    # no records, and records of no samples: -inf, never NaN
    for records in (np.zeros(0, ist.DTYPE), np.zeros(3, ist.DTYPE)):
        s = summary_of(hip_lib, records)
        assert s["n_records"] == len(records) and s["n_samples"] == 0
        assert s["mean_power_dbfs"] == -math.inf and s["peak_dbfs"] == -math.inf and s["iq_gain_db"] == -math.inf
        assert s["dc_re"] == 0 and s["dc_im"] == 0 and s["clipped_fraction"] == 0 and s["nan_fraction"] == 0 and s["bits_used"] == 0
        assert not any(isinstance(v, float) and math.isnan(v) for v in s.values())
    # all-zero samples: the logarithms of zero
    z = ist.record(np.zeros((50, 2), np.int16), ist.CS16)
    s = summary_of(hip_lib, z)
    assert s["n_samples"] == 50 and s["mean_power_dbfs"] == -math.inf and s["peak_dbfs"] == -math.inf and s["iq_gain_db"] == -math.inf
    assert s["bits_used"] == 0 and not any(isinstance(v, float) and math.isnan(v) for v in s.values())
    # constant (1000, -1000), in two records
    x = np.tile(np.array([[1000, -1000]], np.int16), (300, 1))
    recs = np.array([ist.record(x[:100], ist.CS16), ist.record(x[100:], ist.CS16)], dtype=ist.DTYPE)
    s = summary_of(hip_lib, recs)
    assert s["n_records"] == 2 and s["n_samples"] == 300
    assert s["dc_re"] == 1000.0 and s["dc_im"] == -1000.0 and s["iq_gain_db"] == 0.0
    assert s["clipped_fraction"] == 0.0 and s["nan_fraction"] == 0.0
    assert s["bits_used"] == 10                                    # 512 <= 1000 < 1024
    assert abs(s["mean_power_dbfs"] - 10 * math.log10(2 * 1000.0 ** 2 / 32768.0 ** 2)) < 1e-9
    assert abs(s["peak_dbfs"] - 20 * math.log10(1000 / 32768.0)) < 1e-9
    # bits_used: the highest non-empty bin, over all records; the fractions; a real stream has no im power
    r = ist.record(np.array([3, -32768, 0, 0], np.int16), ist.REAL16)
    s = summary_of(hip_lib, r)
    assert s["bits_used"] == 16 and s["peak_dbfs"] == 0.0 and s["clipped_fraction"] == 0.25 and s["iq_gain_db"] == math.inf
    f = np.array([[np.nan, 0.5], [0.25, 0.25], [1.0, 0.0], [0.0, np.nan]], np.float32)
    s = summary_of(hip_lib, ist.record(f, ist.CF32))
    assert s["nan_fraction"] == 0.5 and s["clipped_fraction"] == 0.25 and s["bits_used"] == 15
    one = ist.record(np.array([[1, 0]], np.int16), ist.CS16)
    assert summary_of(hip_lib, one)["bits_used"] == 1
    # argument checks
    out = _lib.AdsbInputSummary()
    assert hip_lib.adsb_input_summary(None, 1, C.byref(out)) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_input_summary(None, 0, None) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_input_summary(None, 0, C.byref(out)) == _lib.ADSB_OK


def test_argument_checks_that_need_no_device(hip_lib):
    from dump1090_rs_amd import _lib
    INV = _lib.ADSB_ERR_INVALID
    rec = _lib.AdsbInputStats()
    for kind in KINDS:
        assert getattr(hip_lib, f"adsb_instat_set_{kind}")(None, 1) == INV
        assert getattr(hip_lib, f"adsb_instat_set_{kind}")(None, 0) == INV
        assert getattr(hip_lib, f"adsb_instat_get_{kind}")(None) == INV
        assert getattr(hip_lib, f"adsb_instat_selftest_launches_{kind}")(None) == 0
    assert hip_lib.adsb_instat_fetch_decim(None, C.byref(rec)) == INV
    assert hip_lib.adsb_instat_fetch_resamp(None, C.byref(rec)) == INV
    assert hip_lib.adsb_instat_fetch_bank(None, 0, 1, C.byref(rec)) == INV
    t, g = C.c_uint32(), C.c_uint32()
    for fmt in (-1, 4, 100):
        assert hip_lib.adsb_instat_selftest_geometry(fmt, C.byref(t), C.byref(g)) == INV
    assert hip_lib.adsb_instat_selftest_geometry(0, None, C.byref(g)) == INV
    assert hip_lib.adsb_instat_selftest_geometry(0, C.byref(t), None) == INV
    tiles = {}
    for fmt in ist.FORMATS:
        assert hip_lib.adsb_instat_selftest_geometry(fmt, C.byref(t), C.byref(g)) == _lib.ADSB_OK
        tiles[fmt] = t.value
        assert t.value >= 64 and g.value >= 2
    # a tile is the same number of BYTES in every format
    assert tiles[ist.CS16] * 4 == tiles[ist.U8] * 2 == tiles[ist.CF32] * 8 == tiles[ist.REAL16] * 2


def kernel_metadata(asm: str, kernel: str):
    """[(mangled name, {field: value})] of every instantiation of `kernel` in the code object's metadata."""
    out = []
    for m in re.finditer(r"\.name:\s+(_ZN4adsb12_GLOBAL__N_1\d+" + kernel + r"I\S*)\n(.*?)\.wavefront_size", asm, re.S):
        fields = {f: int(re.search(r"\." + f + r":\s+(\d+)", m.group(2)).group(1))
                  for f in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "vgpr_count")}
        out.append((m.group(1), fields))
    return out


def test_the_kernels_cross_compile_for_gfx950_without_scratch(tmp_path):
    from dump1090_rs_amd import build
    assert CSRC / "adsb_instat.hip" in build.SOURCES and CSRC / "adsb_instat.cpp" in build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in build.FLAGS if f != "-shared"]
    subprocess.run([hipcc, *flags, "-Werror", "-save-temps", "-c", str(CSRC / "adsb_instat.hip"), "-o", str(tmp_path / "instat.o")],
                   check=True, cwd=tmp_path, capture_output=True, timeout=600)
    asm = next(tmp_path.glob("adsb_instat*amdgcn-amd-amdhsa-gfx950.s")).read_text()
    found = kernel_metadata(asm, "k_instat") + kernel_metadata(asm, "k_instat_bank")
    assert len(found) == 8, [n for n, _ in found]   # four formats, a single handle's and a bank's
    for name, f in found:
        print(name, f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)

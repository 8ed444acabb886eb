"""Signal statistics (include/adsb_hip.h, "Signal statistics") without a GPU: the declarations, the record's layout in C,
ctypes, numpy and the Rust shim, adsb_signal_bin over every magnitude, adsb_signal_summary against numpy, and what
hipcc makes of k_signal_stats."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import signal_support as ss
from tests.conftest import ROOT

HEADER = ROOT / "include" / "adsb_hip.h"
FFI = ROOT / "integration" / "rust" / "src" / "hip_ffi.rs"
KERNEL = ROOT / "dump1090_rs_amd" / "csrc" / "adsb_stats.hip"
NEW = ("adsb_set_signal_stats", "adsb_get_signal_stats", "adsb_fetch_signal_stats", "adsb_signal_bin",
       "adsb_signal_summary", "adsb_selftest_signal_launches")
C_TO_NP = {"uint64_t": "<u8", "uint32_t": "<u4", "double": "<f8"}
C_TO_RUST = {"uint64_t": "u64", "uint32_t": "u32", "double": "f64"}


def strip_comments(text: str) -> str:
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def header_struct(name: str):
    """[(field, C type, count)] of `typedef struct <name> { ... } <name>;`."""
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", strip_comments(HEADER.read_text()), flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            mm = re.match(r"^(\w+) (\w+)(?:\[(\d+)\])?$", decl)
            assert mm, decl
            out.append((mm.group(2), mm.group(1), int(mm.group(3) or 1)))
    return out


def test_header_declares_and_library_exports_the_new_symbols(hip_lib):
    text = strip_comments(HEADER.read_text())
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(hip_lib, name), name
    assert "adsb_shard_* / adsb_multi_* do not deliver records" in HEADER.read_text()
    assert re.search(r"adsb_hip 0\.(2[2-9]|[3-9]\d)", hip_lib.adsb_version().decode())


def test_record_is_272_bytes_in_c_and_the_mirrors_agree_field_by_field(tmp_path):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "adsb_hip.h"\n'
                   "_Static_assert(sizeof(adsb_signal_stats) == 272, \"size\");\n"
                   "_Static_assert(offsetof(adsb_signal_stats, hist) == 32, \"hist\");\n"
                   "_Static_assert(sizeof(adsb_signal_summary_t) == 56, \"summary\");\nint main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{HEADER.parent}", "-fsyntax-only", str(src)], check=True)
    fields = header_struct("adsb_signal_stats")
    assert [f[0] for f in fields] == ["chunk", "sum_power", "n_samples", "peak", "n_strong", "n_clipped", "hist"]
    assert fields[-1] == ("hist", "uint32_t", 60)
    ct = _lib.AdsbSignalStats
    assert C.sizeof(ct) == SIGNAL_STATS_DTYPE.itemsize == 272
    assert [f[0] for f in ct._fields_] == list(SIGNAL_STATS_DTYPE.names) == [f[0] for f in fields]
    for name, ctype, count in fields:
        assert getattr(ct, name).offset == SIGNAL_STATS_DTYPE.fields[name][1]
        assert getattr(ct, name).size == SIGNAL_STATS_DTYPE.fields[name][0].itemsize == np.dtype(C_TO_NP[ctype]).itemsize * count
        assert SIGNAL_STATS_DTYPE.fields[name][0].base == np.dtype(C_TO_NP[ctype])
    sfields = header_struct("adsb_signal_summary_t")
    assert [f[0] for f in sfields] == [f[0] for f in _lib.AdsbSignalSummary._fields_]
    assert C.sizeof(_lib.AdsbSignalSummary) == 56


def test_rust_shim_declares_the_records_and_the_calls_as_the_header_does():
    rust = strip_comments(FFI.read_text())
    for cname, rname in (("adsb_signal_stats", "AdsbSignalStats"), ("adsb_signal_summary_t", "AdsbSignalSummary")):
        m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub\s+struct\s+" + rname + r"\s*\{(.*?)\}", rust, flags=re.S)
        assert m, rname
        got = [tuple(" ".join(x.split()) for x in d.replace("pub ", "").split(":")) for d in m.group(1).split(",") if d.strip()]
        want = [(n, C_TO_RUST[t] if k == 1 else f"[{C_TO_RUST[t]}; {k}]") for n, t, k in header_struct(cname)]
        assert got == want
    flat = " ".join(rust.split())
    for decl in ("pub fn adsb_set_signal_stats(ctx: *mut AdsbCtx, enabled: c_int) -> c_int;",
                 "pub fn adsb_get_signal_stats(ctx: *const AdsbCtx) -> c_int;",
                 "pub fn adsb_fetch_signal_stats(ctx: *mut AdsbCtx, out: *mut AdsbSignalStats, cap: usize, n_out: *mut usize) -> c_int;",
                 "pub fn adsb_signal_bin(m: u16) -> c_int;",
                 "pub fn adsb_signal_summary(s: *const AdsbSignalStats, n: usize, out: *mut AdsbSignalSummary) -> c_int;",
                 "pub fn adsb_selftest_signal_launches(ctx: *const AdsbCtx) -> u64;"):
        assert decl in flat, decl
    hdr = " ".join(strip_comments(HEADER.read_text()).split())
    for decl in ("int adsb_set_signal_stats(adsb_ctx *ctx, int enabled);", "int adsb_get_signal_stats(const adsb_ctx *ctx);",
                 "int adsb_fetch_signal_stats(adsb_ctx *ctx, adsb_signal_stats *out, size_t cap, size_t *n_out);",
                 "int adsb_signal_bin(uint16_t m);",
                 "int adsb_signal_summary(const adsb_signal_stats *s, size_t n, adsb_signal_summary_t *out);",
                 "uint64_t adsb_selftest_signal_launches(const adsb_ctx *ctx);"):
        assert decl in hdr, decl


def test_signal_bin_is_the_restatement_for_every_magnitude(hip_lib):
    got = np.array([hip_lib.adsb_signal_bin(m) for m in range(65536)])
    assert np.array_equal(got, ss.BIN)
    assert (np.diff(got) >= 0).all() and got.max() == 59 and got[0] == 0 and set(got) == set(range(60))
    # quarter octaves: a bin's edges are at most a factor 5/4 apart from 8 on (about 1.9 dB at worst, 1.5 dB on average)
    edges = [ss.bin_edge(b) for b in range(8, 60)] + [65536]
    assert all(hi / lo <= 1.25 for lo, hi in zip(edges[:-1], edges[1:]))


def summary(hip_lib, rec):
    from dump1090_rs_amd import _lib
    out = _lib.AdsbSignalSummary()
    assert hip_lib.adsb_signal_summary(rec.ctypes.data if len(rec) else None, len(rec), C.byref(out)) == 0
    return {name: getattr(out, name) for name, _ in _lib.AdsbSignalSummary._fields_}


def test_signal_summary_is_the_formulas_in_float64(hip_lib):
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE, signal_summary
    rng = np.random.default_rng(7)
    for n_rec in (1, 3, 64):
        rec = np.zeros(n_rec, dtype=SIGNAL_STATS_DTYPE)
        for k in range(n_rec):
            m = np.minimum(rng.rayleigh(300.0 * (k + 1), size=ss.CHUNK - 17 * k), 65535).astype(np.uint64)
            m[:5] = [0, 7, 8, 46341, 65535 if k == 2 else 50000]
            r = rec[k]
            r["chunk"], r["n_samples"], r["sum_power"], r["peak"] = k, len(m), int((m * m).sum()), int(m.max())
            r["n_strong"], r["n_clipped"] = int((2 * m * m >= 65535 ** 2).sum()), int(rng.integers(0, 100))
            r["hist"] = np.bincount(ss.BIN[m.astype(np.int64)], minlength=60)
        got, want = summary(hip_lib, rec), ss.summary_of(rec)
        assert got == signal_summary(rec)
        assert got["n_buffers"] == n_rec and got["n_samples"] == want["n_samples"]
        for key in ("mean_power_dbfs", "peak_dbfs", "median_dbfs"):
            assert np.isfinite(got[key]) and abs(got[key] - want[key]) <= 1e-9, key
        for key in ("clipped_fraction", "strong_fraction"):
            assert abs(got[key] - want[key]) <= 1e-15, key
        # the median is the lower edge of the bin the middle sample is in
        allm = np.sort(np.repeat(np.arange(60), rec["hist"].sum(axis=0).astype(np.int64)))
        mid = allm[(want["n_samples"] + 1) // 2 - 1]
        assert abs(got["median_dbfs"] - 20.0 * np.log10(ss.bin_edge(int(mid)) / 65535.0)) <= 1e-9


def test_signal_summary_of_nothing_is_minus_infinity_never_nan(hip_lib):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
    zero = np.zeros(2, dtype=SIGNAL_STATS_DTYPE)
    zero["n_samples"] = ss.CHUNK
    zero["hist"][:, 0] = ss.CHUNK
    empty = np.zeros(2, dtype=SIGNAL_STATS_DTYPE)   # records of no samples at all
    for rec in (zero, empty, np.zeros(0, dtype=SIGNAL_STATS_DTYPE)):
        got = summary(hip_lib, rec)
        assert got == ss.summary_of(rec)
        for key in ("mean_power_dbfs", "peak_dbfs", "median_dbfs"):
            assert got[key] == -np.inf
        assert got["clipped_fraction"] == 0.0 and got["strong_fraction"] == 0.0
        assert not any(np.isnan(v) for v in got.values())
    out = _lib.AdsbSignalSummary()
    assert hip_lib.adsb_signal_summary(None, 1, C.byref(out)) == -1 and hip_lib.adsb_signal_summary(zero.ctypes.data, 2, None) == -1
    assert hip_lib.adsb_get_signal_stats(None) == -1 and hip_lib.adsb_set_signal_stats(None, 1) == -1
    assert hip_lib.adsb_fetch_signal_stats(None, None, 0, None) == -1 and hip_lib.adsb_selftest_signal_launches(None) == 0


# the instructions a kernel of this library never uses: stores and atomics of the scalar unit and its cache controls
# (spelled in pieces: this file is source too)
SCALAR_WRITES = ["s_" + w for w in ("store", "buffer_" + "store", "scratch_" + "store", "atomic", "buffer_" + "atomic",
                                    "dcache_" + "wb", "dcache_" + "discard")]


def test_stats_kernel_compiles_for_gfx950_without_scratch_or_spills(tmp_path):
    from dump1090_rs_amd import build
    assert KERNEL in build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                    "-save-temps", "-c", str(KERNEL), "-o", str(tmp_path / "stats.o")],
                   check=True, cwd=tmp_path, capture_output=True, timeout=600)
    asm = next(tmp_path.glob("*amdgcn-amd-amdhsa-gfx950.s")).read_text()
    names = re.findall(r"\.amdhsa_kernel (\S*k_signal_stats\S*)", asm)
    assert sorted(n[n.index("k_signal_statsI"):][15:19] for n in names) == ["Lb0E", "Lb1E"]     # CS16 and CU8
    for name in names:
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        insts = [ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and ln.strip() and not ln.lstrip().startswith((".", ";"))]
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        fig = {k: int(re.search(r"\.amdhsa_" + f + r" (\d+)", desc).group(1))
               for k, f in (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("lds", "group_segment_fixed_size"),
                            ("scratch", "private_segment_fixed_size"))}
        meta = next(b for b in re.split(r"\n  - \.", asm) if re.search(r"\.name:\s+" + re.escape(name) + r"\s*$", b, re.M))
        fig["vgpr_spill"] = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        fig["sgpr_spill"] = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1))
        u8 = "Lb1E" in name
        print("k_signal_stats<%s>: insts %d" % ("U8" if u8 else "CS16", len(insts)), fig)
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0, fig
        assert fig["vgpr"] <= 64 and 8 * fig["lds"] <= 160 * 1024        # eight workgroups of four waves a CU
        # one 16-byte load per four CS16 samples, one 8-byte load per four CU8 samples; LDS adds that return nothing;
        # the record leaves in 16-byte stores; no scalar-unit write of any kind
        assert ("buffer_load_dwordx2" if u8 else "buffer_load_dwordx4") in insts
        assert "ds_add_u32" in insts and not any(i.startswith("ds_add_rtn") for i in insts)
        assert "global_store_dwordx4" in insts
        assert not any(i.startswith(tuple(SCALAR_WRITES)) for i in insts)


def test_stats_kernel_source_names_no_scalar_store_or_scalar_atomic():
    text = KERNEL.read_text().lower()
    for word in SCALAR_WRITES:
        assert word not in text, word

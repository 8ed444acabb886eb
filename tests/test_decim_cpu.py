"""The decimator (include/adsb_hip.h, "Decimation") without a GPU: its ABI in the header, the library and the Rust
shim, the argument checks that need no device, the default taps' properties, and the numpy restatement the GPU tests
hold the device to (tests/decim_support.py) checked against itself."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import decim_support as ds
from tests import test_rust_shim as shim
from tests.conftest import ROOT

HEADER = ROOT / "include" / "adsb_hip.h"
FFI = ROOT / "integration" / "rust" / "src" / "hip_ffi.rs"
SEVEN = ("adsb_decim_create", "adsb_decim_destroy", "adsb_decim_reset", "adsb_decim_out_count", "adsb_decim_run_device",
         "adsb_decim_demod_iq", "adsb_decim_default_taps")


def header_prototypes():
    """name -> (Rust parameter types, Rust return type) of every adsb_decim_* prototype of the header."""
    text = shim.strip_comments(HEADER.read_text())
    out = {}
    for m in re.finditer(r"(?:ADSB_MUST_CHECK|extern)?\s*\b(int|void|uint32_t)\s+(adsb_decim_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S):
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
    for f in re.finditer(r"pub\s+fn\s+(adsb_decim_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", text, flags=re.S):
        args = " ".join(f.group(2).split())
        params = [" ".join(a.split(":", 1)[1].split()) for a in args.split(",") if a.strip()]
        out[f.group(1)] = (params, " ".join(f.group(3).split()) if f.group(3) else None)
    return out


def test_the_seven_functions_are_declared_exported_and_bound(hip_lib, monkeypatch):
    monkeypatch.setitem(shim.BASE, "adsb_decim", "AdsbDecim")
    hdr, ffi = header_prototypes(), rust_prototypes()
    assert set(SEVEN) <= set(hdr), sorted(set(SEVEN) - set(hdr))
    assert sorted(hdr) == sorted(ffi)
    for name in hdr:
        assert hdr[name] == ffi[name], f"{name}: header {hdr[name]} vs hip_ffi.rs {ffi[name]}"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hdr["adsb_decim_create"][0] == ["*mut AdsbCtx", "u32", "*const i16", "u32", "u32", "*mut *mut AdsbDecim"]
    text = HEADER.read_text()
    assert "#define ADSB_DECIM_CS16 0" in text and "#define ADSB_DECIM_8BIT 1" in text
    assert "typedef struct adsb_decim adsb_decim;" in text


def test_create_checks_its_pointers_before_it_touches_a_device(hip_lib):
    from dump1090_rs_amd import _lib
    taps = (C.c_int16 * 1)(1)
    h = C.c_void_p(0x1234)
    assert hip_lib.adsb_decim_create(None, 2, taps, 1, 0, C.byref(h)) == _lib.ADSB_ERR_INVALID
    assert h.value is None   # (and the out-pointer does not keep a stale handle)
    fake_ctx = C.c_void_p(0x1000)   # never dereferenced: the out-pointer is checked first
    assert hip_lib.adsb_decim_create(fake_ctx, 2, taps, 1, 0, None) == _lib.ADSB_ERR_INVALID
    n = C.c_size_t()
    assert hip_lib.adsb_decim_out_count(None, 1, C.byref(n)) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_decim_reset(None) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_decim_run_device(None, 0, None, 0, None, 0, C.byref(n)) == _lib.ADSB_ERR_INVALID
    hip_lib.adsb_decim_destroy(None)
    assert hip_lib.adsb_decim_selftest_tile() >= 64


@pytest.mark.parametrize("factor", range(2, 17))
def test_default_taps(hip_lib, factor):
    from dump1090_rs_amd import _lib, default_taps
    taps, shift = default_taps(factor)
    assert taps.dtype == np.int16 and len(taps) == 8 * factor + 1 and shift == 15
    assert np.array_equal(taps, taps[::-1])
    h = taps.astype(np.int64)
    assert np.abs(h).sum() <= 65534
    assert abs(h.sum() - 32768) <= 64
    # the shape it claims: the largest tap in the middle, and close to numpy's table of the same formula
    assert h.argmax() == 4 * factor and np.abs(h - ds.hamming_sinc_taps(factor)).max() <= 64
    # cap too small: the count comes back, nothing is written
    buf = (C.c_int16 * (8 * factor))()
    n, s = C.c_uint32(), C.c_uint32()
    assert hip_lib.adsb_decim_default_taps(factor, buf, 8 * factor, C.byref(n), C.byref(s)) == _lib.ADSB_ERR_CAPACITY
    assert n.value == 8 * factor + 1 and not any(buf)


def test_default_taps_refuses_other_factors(hip_lib):
    from dump1090_rs_amd import _lib
    buf = (C.c_int16 * 200)()
    n, s = C.c_uint32(), C.c_uint32()
    for factor in (0, 1, 17, 1 << 31):
        assert hip_lib.adsb_decim_default_taps(factor, buf, 200, C.byref(n), C.byref(s)) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_decim_default_taps(2, buf, 200, None, C.byref(s)) == _lib.ADSB_ERR_INVALID


# ----------------------------------------------------------------------------------------------- the yardstick itself
@pytest.mark.parametrize("D", [2, 3, 5, 16])
def test_restatement_is_the_identity_on_repeated_samples(D):
    rng = np.random.default_rng(D)
    v = ds.random_iq(rng, 1000, run=20)
    assert np.array_equal(ds.decimate(np.repeat(v, D, axis=0), [1], D, 0), v)
    # ... and one sample short of a multiple of D still has all of them
    assert np.array_equal(ds.decimate(np.repeat(v, D, axis=0)[:-(D - 1)], [1], D, 0), v)


def test_restatement_rounds_and_clamps_as_the_definition_says():
    x = np.array([[-3, -1], [1, 3]], np.int16)
    assert ds.decimate(np.repeat(x, 2, axis=0), [1], 2, 1).tolist() == [[-1, 0], [1, 2]]
    rails = np.array([[-32768, 32767]] * 4, np.int16)
    assert ds.decimate(rails, [32767, 32767], 2, 0)[1].tolist() == [-32768, 32767]


@pytest.mark.parametrize("D, T, s", [(2, 1, 0), (2, 17, 15), (3, 2, 1), (5, 41, 15), (16, 512, 16), (16, 16, 16)])
def test_restatement_streaming_form_is_cut_invariant(D, T, s):
    rng = np.random.default_rng(100 * D + T)
    h = ds.random_taps(rng, T)
    x = ds.random_iq(rng, 3000, run=T)
    want = ds.decimate(x, h, D, s)
    st = ds.Stream(h, D, s)
    lengths = [0, 1, D - 1, D, D + 1, max(T - 2, 0), T - 1, T, 257]
    plan = ds.cut_plan(rng, len(x), lengths, D)
    assert sum(plan) == len(x) and set(lengths) <= set(plan)
    got, at, residues = [], 0, set()
    for n in plan:
        residues.add(st.P % D)
        want_n = st.out_count(n)
        y = st.run(x[at:at + n])
        assert len(y) == want_n
        got.append(y)
        at += n
    assert residues == set(range(D))
    assert np.array_equal(np.concatenate(got), want)
    st.reset()
    assert np.array_equal(st.run(x), want)


def test_random_taps_hit_the_bound():
    rng = np.random.default_rng(1)
    for T in (1, 2, 3, 17, 512):
        h = ds.random_taps(rng, T).astype(np.int64)
        assert np.abs(h).sum() == min(65534, 32767 * T) and len(h) == T


# ----------------------------------------------------------------------------------------------- the edge tests' inputs
def test_worst_case_inputs_reach_the_accumulators_limit():
    """tests/test_gpu_decim_edges.py, "the accumulator at its limit": by the int64 restatement alone, output n0's
    accumulator is the bound the taps and the rails give, it fits an int32 with the rounding term added, and for taps of
    full weight over a whole window it lies within 2^17 of 2^31."""
    t = 256
    sets = ds.worst_case_sets()
    assert [name for name, _, _ in sets] == ["random 2", "random 17", "random 512", "positive", "negative",
                                             "-32768 32766", "-32768", "32767 -32767"]
    assert [int(np.abs(h.astype(np.int64)).sum()) for _, h, _ in sets] == [65534] * 6 + [32768, 65534]
    full_windows = 0
    for D in ds.WORST_D:
        outputs, n = ds.worst_case_outputs(D, t)
        assert n % D and -(-n // D) == 2 * t + 37
        for name, h, shifts in sets:
            T, h64 = len(h), h.astype(np.int64)
            weight = int(np.abs(h64).sum())
            for n0 in outputs:
                for pol in (1, -1):
                    x = ds.worst_case_iq(h, D, n0, n, pol).astype(np.int64)
                    ks = [k for k in range(T) if n0 * D - k >= 0]
                    acc = sum(int(h64[k]) * x[n0 * D - k] for k in ks)   # (python integers: no width at all)
                    bound = ds.worst_case_acc(h, D, n0, pol)
                    assert int(acc[0]) == int(acc[1]) == bound, (D, name, n0, pol)
                    assert bound * pol > 0
                    assert abs(bound) == sum(abs(int(h64[k])) * (32767 if pol * h64[k] > 0 else 32768) for k in ks)
                    for s in shifts:
                        r = (1 << (s - 1)) if s else 0
                        assert abs(bound + r) < 2 ** 31
                        want = min(max((bound + r) >> s, -32768), 32767)
                        assert ds.decimate(x, h, D, s)[n0].tolist() == [want, want]
                    if weight == 65534 and len(ks) == T:
                        assert abs(bound) >= 2 ** 31 - 2 ** 17, (D, name, n0, pol)
                        full_windows += 1
            # every set has an output with its whole window inside the stream
            assert any(n0 * D >= T - 1 for n0 in outputs)
    assert full_windows >= 7 * 2 * 2 * len(ds.WORST_D)
    # the tap -32768 against the sample -32768: 2^30, which clamps
    x = ds.worst_case_iq([-32768], 2, 3, 10, 1)
    assert x[6].tolist() == [-32768, -32768] and ds.decimate(x, [-32768], 2, 0)[3].tolist() == [32767, 32767]
    assert ds.worst_case_acc([-32768], 2, 3, 1) == 2 ** 30 and ds.worst_case_acc([-32768], 2, 3, -1) == -32768 * 32767
    # through bytes and a table with both rails the same accumulators come out
    table = ds.rail_u8_table()
    assert np.array_equal(np.diff(table.astype(np.int64)), np.full(255, 257))
    for name, h, _ in sets:
        if name in ("positive", "negative", "random 512"):
            for pol in (1, -1):
                b = ds.worst_case_iq(h, 7, t, (t + 5) * 7, pol, lo=0, hi=255, dtype=np.uint8)
                assert b.dtype == np.uint8
                x = table[b].astype(np.int64)
                acc = sum(int(hk) * x[t * 7 - k] for k, hk in enumerate(h.astype(np.int64)))
                assert int(acc[0]) == int(acc[1]) == ds.worst_case_acc(h, 7, t, pol)


def test_the_factor_grid_meets_both_parities_of_the_row_length(hip_lib):
    """decim_row_len makes ceil((tile D + T + 15) / D) odd with `| 1`: over the grid of "every factor" the ceiling is
    even (the bump does something) and odd (it does nothing), and so it is for most single factors."""
    t = int(hip_lib.adsb_decim_selftest_tile())
    assert t == 256
    both = 0
    seen = set()
    for D in range(2, 17):
        taps = ds.grid_taps(D)
        assert set(taps) >= {1, D - 1, D + 1, 8 * D + 1, 505, 511, 512} and min(taps) == 1 and max(taps) == 512
        par = {ds.row_ceiling(D, T, t) % 2 for T in taps}
        seen |= par
        both += par == {0, 1}
        # the row holds every local sample of a tile: tile D + T - 1 + 15 of them at most, D to a column
        assert all((ds.row_ceiling(D, T, t) | 1) * D >= t * D + T - 1 + 15 for T in taps)
    assert seen == {0, 1} and both >= 8


def test_decimate_window_agrees_with_decimate():
    rng = np.random.default_rng(77)
    for D, T, s in [(2, 1, 0), (3, 17, 15), (16, 17, 15), (5, 512, 16)]:
        h = ds.random_taps(rng, T)
        x = ds.random_iq(rng, 700 * D + 3, run=T)
        want = ds.decimate(x, h, D, s)
        for first, count in [(0, 1), (0, 40), (1, 5), (T // D, 9), (T // D + 1, 300), (len(want) - 3, 3), (len(want) - 1, 1)]:
            lo, hi = ds.window_inputs(first, count, T, D)
            assert 0 <= lo < hi <= len(x)
            assert lo == 0 or lo == first * D - (T - 1)
            assert np.array_equal(ds.decimate_window(x[lo:hi], first, count, h, D, s), want[first:first + count]), (D, T, first)
        # a window one sample short is refused, not padded
        lo, hi = ds.window_inputs(T // D + 1, 5, T, D)
        with pytest.raises(AssertionError):
            ds.decimate_window(x[lo:hi - 1], T // D + 1, 5, h, D, s)
    # the tile origin the large call's windows are chosen from: 8-sample boundaries, never in front of the call
    assert ds.tile_base(0, 0, 16, 17, 256) == 0 and ds.tile_base(1, 0, 16, 17, 256) == 4096 - 16 - 8
    assert ds.tile_base(1, 3, 2, 17, 256) == (3 + 512 - 16 - 8) & ~7 == 488

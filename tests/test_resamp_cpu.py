"""The resampler (include/adsb_hip.h, "Resampling") without a GPU: its ABI in the header, the library and the Rust shim,
the argument checks that need no device, the count formula, the ratio of a sample rate, the default taps' properties, and
the numpy restatement the GPU tests hold the device to (tests/resamp_support.py) checked against itself and against the
decimator's."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from tests import decim_support as ds
from tests import resamp_support as rs
from tests import test_rust_shim as shim
from tests.conftest import ROOT

HEADER = ROOT / "include" / "adsb_hip.h"
FFI = ROOT / "integration" / "rust" / "src" / "hip_ffi.rs"
NAMES = ("adsb_resamp_create", "adsb_resamp_destroy", "adsb_resamp_reset", "adsb_resamp_out_count", "adsb_resamp_run_device",
          "adsb_resamp_demod_iq", "adsb_resamp_default_taps", "adsb_resamp_ratio_for_rate", "adsb_resamp_plan",
          "adsb_resamp_selftest_tile")


def header_prototypes():
    """name -> (Rust parameter types, Rust return type) of every adsb_resamp_* prototype of the header."""
    text = shim.strip_comments(HEADER.read_text())
    out = {}
    for m in re.finditer(r"(?:ADSB_MUST_CHECK|extern)?\s*\b(int|void|uint32_t)\s+(adsb_resamp_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S):
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
    for f in re.finditer(r"pub\s+fn\s+(adsb_resamp_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", text, flags=re.S):
        args = " ".join(f.group(2).split())
        params = [" ".join(a.split(":", 1)[1].split()) for a in args.split(",") if a.strip()]
        out[f.group(1)] = (params, " ".join(f.group(3).split()) if f.group(3) else None)
    return out


def test_the_functions_are_declared_exported_and_bound(hip_lib, monkeypatch):
    import dump1090_rs_amd as pkg
    monkeypatch.setitem(shim.BASE, "adsb_resamp", "AdsbResamp")
    hdr, ffi = header_prototypes(), rust_prototypes()
    assert sorted(hdr) == sorted(NAMES)
    assert sorted(hdr) == sorted(ffi)
    for name in hdr:
        assert hdr[name] == ffi[name], f"{name}: header {hdr[name]} vs hip_ffi.rs {ffi[name]}"
        assert hasattr(hip_lib, name), f"{name} is not exported"
        assert getattr(hip_lib, name).argtypes is not None, f"{name} has no ctypes prototype"
        assert len(getattr(hip_lib, name).argtypes) == len(hdr[name][0]), name
    assert hdr["adsb_resamp_create"][0] == ["*mut AdsbCtx", "u32", "u32", "*const i16", "u32", "u32", "*mut *mut AdsbResamp"]
    assert hdr["adsb_resamp_plan"] == (["u32", "u32", "u64", "u64", "*mut u64", "*mut u64"], "c_int")
    text = HEADER.read_text()
    assert "typedef struct adsb_resamp adsb_resamp;" in text
    for name in ("Resampler", "default_resampler_taps", "ratio_for_rate"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert hasattr(pkg.Context, "resampler")
    for method in ("reset", "out_count", "run_device", "demod_iq", "close", "__enter__", "__exit__"):
        assert hasattr(pkg.Resampler, method)


def create(hip_lib, ctx, L, M, taps, s, out=None):
    t = np.ascontiguousarray(list(taps) + [0], dtype=np.int16)   # (one more, so that no taps at all still have an address)
    h = C.c_void_p(0x1234) if out is None else out
    st = hip_lib.adsb_resamp_create(ctx, L, M, t.ctypes.data, len(t) - 1, s, C.byref(h))
    return st, h


def test_create_checks_pointers_and_arguments_before_it_touches_a_device(hip_lib):
    from dump1090_rs_amd import _lib
    INV = _lib.ADSB_ERR_INVALID
    taps = (C.c_int16 * 1)(1)
    h = C.c_void_p(0x1234)
    assert hip_lib.adsb_resamp_create(None, 1, 2, taps, 1, 0, C.byref(h)) == INV
    assert h.value is None   # (and the out-pointer does not keep a stale handle)
    fake_ctx = C.c_void_p(0x1000)   # never dereferenced: every check below comes before the device is touched
    assert hip_lib.adsb_resamp_create(fake_ctx, 1, 2, taps, 1, 0, None) == INV
    assert hip_lib.adsb_resamp_create(fake_ctx, 1, 2, None, 1, 0, C.byref(h)) == INV
    one = [1]
    for L, M, t, s, why in [
            (2, 4, one, 0, "gcd != 1"), (6, 4, one, 0, "gcd != 1"), (0, 1, one, 0, "L = 0"), (1, 0, one, 0, "M = 0"),
            (129, 128, one, 0, "L > 128"), (1, 129, one, 0, "M > 128"),
            (3, 1, one, 0, "L > 2 M"), (5, 2, one, 0, "L > 2 M"), (1, 17, one, 0, "M > 16 L"), (3, 49, one, 0, "M > 16 L"),
            (1, 2, [1] * 513, 0, "K > 512"), (3, 4, [1] * (3 * 512 + 1), 0, "K > 512"), (16, 17, [1] * 4097, 0, "T > 4096"),
            (1, 2, [32767, 32767, 1], 0, "a phase at 65535"), (2, 3, [1, 32767, 1, 32767, 1, 1], 0, "a phase at 65535"),
            (1, 2, [], 0, "T = 0"), (1, 2, one, 17, "s = 17")]:
        st, h = create(hip_lib, fake_ctx, L, M, t, s)
        assert st == INV, why
        assert h.value is None, why
    # (the same phase one lighter is not refused by the argument checks: nothing left to check but the device, which this
    # test must not touch -- tests/test_gpu_resamp.py creates such resamplers)
    assert rs.phase_abs_sums([1, 32767, 1, 32767, 1, 1], 2).tolist() == [3, 65535]
    n = C.c_size_t()
    assert hip_lib.adsb_resamp_out_count(None, 1, C.byref(n)) == INV
    assert hip_lib.adsb_resamp_reset(None) == INV
    assert hip_lib.adsb_resamp_run_device(None, 0, None, 0, None, 0, C.byref(n)) == INV
    assert hip_lib.adsb_resamp_demod_iq(None, 0, None, 0, None, 0, C.byref(n)) == INV
    hip_lib.adsb_resamp_destroy(None)


def test_selftest_tile(hip_lib):
    for L, M in rs.TABLE_RATIOS + [(1, 1), (1, 5), (1, 16), (2, 1), (128, 65), (127, 128), (128, 127), (8, 127)]:
        t = int(hip_lib.adsb_resamp_selftest_tile(L, M))
        assert t >= 8 * L and t % L == 0 and t % 4 == 0, (L, M, t)
        assert t // L in (8, 16, 32, 64, 128, 256, 512, 1024)
    for L, M in [(2, 4), (3, 1), (1, 17), (0, 1), (129, 1)]:
        assert hip_lib.adsb_resamp_selftest_tile(L, M) == 0


def test_every_tile_class_is_run_on_the_device(hip_lib):
    """resamp_rows over every ratio adsb_resamp_create accepts: 32 to 1024 rows, never the 16 and 8 it lists, and every
    class of (rows, tile above 2048 outputs, L no multiple of four) is met by a ratio the GPU files launch
    (tests/test_gpu_resamp_edges.py: rs.EDGE_RATIOS; tests/test_gpu_resamp.py and tests/test_gpu_mix.py:
    rs.FIRST_FILES_RATIOS).  A change of resamp_rows that opens another class fails here."""
    def tile(L, M):
        return int(hip_lib.adsb_resamp_selftest_tile(L, M))

    ratios = rs.accepted_ratios()
    assert len(ratios) == 7223 and set(rs.EDGE_RATIOS + rs.FIRST_FILES_RATIOS) <= set(ratios)
    assert not set(rs.EDGE_RATIOS) & set(rs.FIRST_FILES_RATIOS)
    classes = {}
    for L, M in ratios:
        t = tile(L, M)
        assert t > 0 and t % L == 0 and t % 4 == 0 and t <= 8192, (L, M, t)
        assert t // L in (32, 64, 128, 256, 512, 1024), (L, M, t)
        classes.setdefault(rs.tile_class(L, t), []).append((L, M))
    assert max(rows for rows, _, _ in classes) == 1024 and min(rows for rows, _, _ in classes) == 32
    assert sum(len(v) for k, v in classes.items() if k[1]) == 5144   # tiles above 2048 outputs: 71 % of the ratios
    run_on_the_gpu = {rs.tile_class(L, tile(L, M)) for L, M in rs.EDGE_RATIOS + rs.FIRST_FILES_RATIOS}
    assert run_on_the_gpu == set(classes), sorted(set(classes) - run_on_the_gpu)
    # the first files alone leave out every tile above 2048 outputs (four classes) and three more
    first = {rs.tile_class(L, tile(L, M)) for L, M in rs.FIRST_FILES_RATIOS}
    assert not any(big for _, big, _ in first) and len(set(classes) - first) == 7
    # the ratios of three ordinary rates lie in the classes the first files leave out
    from dump1090_rs_amd import ratio_for_rate
    assert [ratio_for_rate(hz) for hz in (2_450_000, 2_375_000, 2_304_000)] == [(48, 49), (96, 95), (25, 24)]
    assert [tile(L, M) for L, M in [(48, 49), (96, 95), (25, 24)]] == [3072, 6144, 1600]
    assert rs.tile_class(25, 1600) == rs.tile_class(31, 31 * 64) and rs.tile_class(25, 1600) not in first
    # the tiles the edge file's docstrings name
    tiles = {r: tile(*r) for r in rs.EDGE_RATIOS}
    assert [tiles[r] for r in [(33, 17), (33, 128), (48, 49), (96, 95), (64, 127), (128, 65)]] == [2112, 2112, 3072, 6144, 4096, 8192]
    rows = [tiles[r] // r[0] for r in [(128, 127), (127, 128), (117, 128), (16, 15), (2, 1), (4, 3), (31, 128)]]
    assert rows == [32, 32, 32, 128, 1024, 512, 64]


def lds_bytes(L, M, rows, K):
    """resamp_lds_words restated from DESIGN.md ("LDS layout"): the polyphase store in rows of an odd length, rounded up
    to 16 bytes, the staged outputs, the 8-bit table."""
    row_len = ((rows * M + K + 15 + M - 1) // M) | 1
    return 4 * (((M * row_len + 3) & ~3) + L * rows + 128)


def test_the_largest_lds_requests_are_among_the_edge_ratios(hip_lib):
    def at_k_512(L, M):
        return lds_bytes(L, M, int(hip_lib.adsb_resamp_selftest_tile(L, M)) // L, 512)

    # (K = 512 needs 512 L <= 4096 taps)
    sizes = sorted(((at_k_512(L, M), (L, M)) for L, M in rs.accepted_ratios() if 512 * L <= 4096), reverse=True)
    assert sizes[0] == (65440, (5, 56)) and (65360, (7, 54)) in sizes[:3] and sizes[0][0] <= 65536
    assert {(5, 56), (7, 54)} <= set(rs.EDGE_RATIOS)
    assert max(at_k_512(L, M) for L, M in rs.FIRST_FILES_RATIOS) < 41 * 1024


@pytest.mark.parametrize("L, M, T, s", [(3, 25, 201, 14), (6, 5, 49, 14), (33, 17, 4096, 16), (2, 1, 3, 0), (127, 128, 1, 0)])
def test_restatement_by_windows_is_a_slice_of_the_whole(L, M, T, s):
    rng = np.random.default_rng(300 + L)
    h = rs.random_phase_taps(rng, T, L)
    K = rs.phase_taps(L, T)
    x = rs.random_iq(rng, 4000, run=K)
    want = rs.resample(x, h, L, M, s)
    assert len(want) >= 480
    for first, count in [(0, 1), (0, 50), (1, 7), (K * L // M + 3, 100), (len(want) // 2, 233), (len(want) - 9, 9), (5, 0)]:
        lo, hi = rs.window_inputs(first, count, T, L, M)
        assert 0 <= lo < hi <= len(x) or count == 0
        if count:
            # the window is exactly what these outputs read: the oldest input of the first, the newest of the last
            assert lo == max((first * M) // L - (K - 1), 0) and hi - 1 == ((first + count - 1) * M) // L
        got = rs.resample_window(x[lo:hi], first, count, h, L, M, s)
        assert np.array_equal(got, want[first:first + count]), (first, count)
        # ... and no more: with a sample less the window is refused
        if count:
            with pytest.raises(AssertionError):
                rs.resample_window(x[lo:hi - 1], first, count, h, L, M, s)


def test_tile_base_is_the_boundary_below_the_first_input_needed():
    for L, M, K, t, q0 in [(3, 25, 67, 768, 0), (3, 25, 67, 768, 7), (128, 127, 9, 4096, 0), (5, 56, 512, 1280, 3), (1, 1, 1, 1024, 0)]:
        for blk in (0, 1, 2, 3, 1000, 41_000):
            need = q0 + blk * (t // L) * M - (K - 1)   # the oldest input of the tile's first output
            assert need == q0 + ((blk * t) * M) // L - (K - 1)
            b = rs.tile_base(blk, q0, L, M, K, t)
            assert b % 8 == 0 and (b == 0 or 8 <= need - b <= 15) and (b > 0 or need < 16)


@pytest.mark.parametrize("L, M, K", [(33, 17, 125), (128, 65, 32), (6, 5, 512)])
def test_rails_behind_an_output_reach_the_bound(L, M, K):
    """rs.rail_window: the accumulator it returns is the one the restatement computes, and it lies where the taps' weight
    and the rails put it."""
    rng = np.random.default_rng(400 + L)
    h = rs.random_phase_taps(rng, rs.max_taps(L), L)
    assert rs.phase_taps(L, len(h)) == K
    for n0 in (K * L, 2111, 2113):
        for pol in (1, -1):
            x = rs.random_iq(rng, (n0 * M) // L + 5, run=0)
            acc, weight = rs.rail_window(x, h, L, M, n0, pol)
            assert weight == 65534 and acc * pol > 0 and 65534 * 32767 <= abs(acc) <= 65534 * 32768 < 2 ** 31 - 32768
            assert x[(n0 * M) // L].tolist() in ([32767, 32767], [-32768, -32768])
            for s in (0, 16):
                r = (1 << (s - 1)) if s else 0
                assert rs.resample(x, h, L, M, s)[n0].tolist() == [min(max((acc + r) >> s, -32768), 32767)] * 2


def test_the_stretched_stream_shares_the_boundaries_the_edge_file_says():
    """(b M) mod L >= M exactly for b = 1 mod 96 at 96/95, and 131 072 = 32 mod 96: behind P = 64 a blocking call's first
    output is 65 and its buffer boundaries 1 and 4 of every three fall between two outputs that share their newest input."""
    L, M, P = 96, 95, 64
    assert rs.out_range(L, M, P, 1)[0] == 65 and rs.CHUNK % L == 32
    for b in range(1, 4 * L):
        assert (((b - 1) * M) // L == (b * M) // L) == ((b * M) % L >= M) == (b % L == 1)
    assert [k for k in range(1, 8) if (65 + k * rs.CHUNK) % L == 1] == [1, 4, 7]


def plan(hip_lib, L, M, P, n_in):
    first, n = C.c_uint64(), C.c_uint64()
    st = hip_lib.adsb_resamp_plan(L, M, P, n_in, C.byref(first), C.byref(n))
    return st, first.value, n.value


def test_plan_agrees_with_python_integers(hip_lib):
    from dump1090_rs_amd import _lib
    rng = np.random.default_rng(11)
    ratios = [(L, M) for L in range(1, 129) for M in range(1, 129) if math.gcd(L, M) == 1 and L <= 2 * M and M <= 16 * L]
    seen_empty = 0
    for i in range(4000):
        L, M = ratios[int(rng.integers(len(ratios)))]
        P = int(rng.integers(0, 1 << 20)) if i % 2 else (1 << 48) - int(rng.integers(0, 1 << 16))
        n_in = int(rng.choice([0, 1, 2, 5, 17, 300, 999, int(rng.integers(0, 1 << 33))]))
        st, first, n = plan(hip_lib, L, M, P, n_in)
        assert st == _lib.ADSB_OK
        assert (first, n) == rs.out_range(L, M, P, n_in), (L, M, P, n_in)
        # the definition itself: the outputs whose newest input lies in the call
        if n:
            assert P <= first * M // L and (first + n - 1) * M // L < P + n_in <= (first + n) * M // L
            assert first == 0 or (first - 1) * M // L < P
        else:
            seen_empty += 1
            assert first * M // L >= P + n_in
    assert seen_empty > 100
    # consecutive calls tile the outputs
    for L, M in [(1, 5), (6, 5), (24, 25), (6, 25), (3, 10), (2, 5), (75, 64)]:
        P = nxt = 0
        for n_in in [0, 1, 2, 5, 17, 300, 999] * 3:
            st, first, n = plan(hip_lib, L, M, P, n_in)
            assert st == _lib.ADSB_OK and first == nxt
            nxt, P = first + n, P + n_in
        assert nxt == rs.ceil_div(P * L, M)
    assert plan(hip_lib, 1, 5, 7, 13)[1:] == (2, 2)   # (P = 7: outputs 2 and 3, whose inputs are 10 and 15)
    for L, M in [(2, 4), (3, 1), (1, 17)]:
        assert plan(hip_lib, L, M, 0, 1)[0] == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_resamp_plan(1, 2, 0, 1, None, None) == _lib.ADSB_ERR_INVALID
    assert plan(hip_lib, 1, 2, 1 << 56, 1)[0] == _lib.ADSB_ERR_INVALID


def test_ratio_for_rate(hip_lib):
    from dump1090_rs_amd import _lib, ratio_for_rate
    from dump1090_rs_amd._lib import AdsbError
    assert len(rs.RADIO_RATES) == 10 and len(rs.TABLE_RATIOS) == 10   # (10 MS/s stands in two rows of the header's list)
    for hz, ratio in rs.RADIO_RATES.items():
        assert ratio_for_rate(hz) == ratio
    assert ratio_for_rate(2_400_000) == (1, 1) and ratio_for_rate(4_800_000) == (1, 2) and ratio_for_rate(24_000_000) == (1, 10)
    assert ratio_for_rate(2_812_500) == (64, 75) and ratio_for_rate(1_200_000) == (2, 1) and ratio_for_rate(2_048_000) == (75, 64)
    up, down = C.c_uint32(), C.c_uint32()
    assert hip_lib.adsb_resamp_ratio_for_rate(2_400_001, C.byref(up), C.byref(down)) == _lib.ADSB_ERR_INVALID
    assert (up.value, down.value) == (2_400_000, 2_400_001)
    for hz in (2_400_001, 1_000_000, 48_000_000, 0):   # L too large, L > 2 M (12/5), M > 16 L (1/20), no rate
        with pytest.raises(AdsbError) as e:
            ratio_for_rate(hz)
        assert e.value.status == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_resamp_ratio_for_rate(3_000_000, None, C.byref(down)) == _lib.ADSB_ERR_INVALID


@pytest.mark.parametrize("L, M", rs.TABLE_RATIOS)
def test_default_taps(hip_lib, L, M):
    from dump1090_rs_amd import _lib, default_resampler_taps
    taps, shift = default_resampler_taps(L, M)
    big = max(L, M)
    assert taps.dtype == np.int16 and len(taps) == 8 * big + 1 and shift == 14
    assert np.array_equal(taps, taps[::-1])
    h = taps.astype(np.int64)
    assert h.argmax() == 4 * big and -32768 < h.min() and h.max() < 32767
    assert rs.phase_abs_sums(h, L).max() <= 65534
    assert np.abs(h - rs.hamming_sinc_taps(L, M)).max() <= 1
    sums = np.array([h[p::L].sum() for p in range(L)])
    assert (np.abs(sums - 16384) <= 163).all(), sums
    assert abs(int(h.sum()) - L * 16384) <= 4 * big + 1   # (every tap rounded on its own)
    # cap too small: the count comes back, nothing is written
    buf = (C.c_int16 * (8 * big))()
    n, s = C.c_uint32(), C.c_uint32()
    assert hip_lib.adsb_resamp_default_taps(L, M, buf, 8 * big, C.byref(n), C.byref(s)) == _lib.ADSB_ERR_CAPACITY
    assert n.value == 8 * big + 1 and s.value == 14 and not any(buf)


def test_default_taps_refuses_other_ratios(hip_lib):
    from dump1090_rs_amd import _lib
    buf = (C.c_int16 * 1100)()
    n, s = C.c_uint32(), C.c_uint32()
    for L, M in [(0, 1), (2, 4), (3, 1), (1, 17), (129, 128), (1 << 31, 1)]:
        assert hip_lib.adsb_resamp_default_taps(L, M, buf, 1100, C.byref(n), C.byref(s)) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_resamp_default_taps(1, 2, buf, 1100, None, C.byref(s)) == _lib.ADSB_ERR_INVALID


# ----------------------------------------------------------------------------------------------- the yardstick itself
@pytest.mark.parametrize("L, M, T, s", [(1, 5, 41, 15), (6, 5, 49, 14), (24, 25, 201, 14), (6, 25, 7, 1), (3, 10, 3, 0),
                                        (2, 5, 1, 0), (75, 64, 601, 14), (1, 1, 9, 3), (2, 1, 1024, 16)])
def test_restatement_streaming_form_is_cut_invariant(L, M, T, s):
    rng = np.random.default_rng(100 * L + M)
    h = rs.random_phase_taps(rng, T, L)
    assert rs.phase_abs_sums(h, L).max() <= 65534
    K = rs.phase_taps(L, T)
    x = rs.random_iq(rng, 3000, run=K)
    want = rs.resample(x, h, L, M, s)
    assert len(want) == rs.ceil_div(3000 * L, M)
    st = rs.Stream(h, L, M, s)
    lengths = [0, 1, 2, 5, 17, 300, 999, max(K - 2, 0), K - 1, K]
    plan_ = rs.cut_plan(rng, len(x), lengths, max(L, M))
    assert sum(plan_) == len(x)
    got, at, res_p, res_n, empty = [], 0, set(), set(), 0
    for n in plan_:
        res_p.add(st.P % M)
        res_n.add(rs.ceil_div(st.P * L, M) % L)
        want_n = st.out_count(n)
        y = st.run(x[at:at + n])
        assert len(y) == want_n
        empty += n > 0 and want_n == 0
        got.append(y)
        at += n
    # every residue of P mod M and every residue mod L a call's first output can have (where L > M two outputs can share
    # their newest input, and the second of them never is a call's first)
    assert res_p == set(range(M)) and res_n == {rs.ceil_div(P * L, M) % L for P in range(M)}
    assert L > M or res_n == set(range(L))
    assert empty > 0 or L >= M
    assert np.array_equal(np.concatenate(got), want)
    st.reset()
    assert np.array_equal(st.run(x), want)


@pytest.mark.parametrize("M, T, s", [(1, 9, 3), (2, 17, 15), (5, 41, 15), (16, 512, 16)])
def test_restatement_is_the_decimators_at_l_1(M, T, s):
    rng = np.random.default_rng(7 * M + T)
    h = ds.random_taps(rng, T)
    x = rs.random_iq(rng, 2500 + M // 2, run=T)
    assert np.array_equal(rs.resample(x, h, 1, M, s), ds.decimate(x, h, M, s))
    a, b = rs.Stream(h, 1, M, s), ds.Stream(h, M, s)
    at = 0
    for n in [0, 1, 2, 5, 17, 300, 999, len(x)]:
        n = min(n, len(x) - at)
        assert a.out_count(n) == b.out_count(n)
        assert np.array_equal(a.run(x[at:at + n]), b.run(x[at:at + n]))
        at += n


@pytest.mark.parametrize("L, M", [(1, 1), (1, 5), (6, 5), (2, 1), (24, 25), (3, 10), (75, 64)])
def test_restatement_with_a_boxcar_is_sample_and_hold(L, M):
    rng = np.random.default_rng(L + M)
    x = rs.random_iq(rng, 777, run=20)
    y = rs.resample(x, [1] * L, L, M, 0)
    n = np.arange(len(y))
    assert len(y) == rs.ceil_div(777 * L, M) and np.array_equal(y, x[(n * M) // L])
    if L <= M:
        assert np.array_equal(rs.resample(rs.hold_input(y, L, M, rng), [1] * L, L, M, 0), y)


def test_restatement_rounds_and_clamps_as_the_definition_says():
    x = np.array([[-3, -1], [1, 3]], np.int16)
    # 2/1: each input twice; (v + 1) >> 1
    assert rs.resample(x, [1, 1], 2, 1, 1).tolist() == [[-1, 0], [-1, 0], [1, 2], [1, 2]]
    rails = np.array([[-32768, 32767]] * 4, np.int16)
    assert rs.resample(rails, [32767, 0, 32767, 0], 2, 1, 0)[2].tolist() == [-32768, 32767]


def test_random_phase_taps_hit_the_bound():
    rng = np.random.default_rng(1)
    for T, L in [(1, 1), (6, 6), (7, 6), (49, 6), (4096, 8), (3072, 6), (1001, 24)]:
        h = rs.random_phase_taps(rng, T, L)
        sums = rs.phase_abs_sums(h, L)
        counts = np.array([len(h[p::L]) for p in range(L)])
        assert len(h) == T and np.array_equal(sums, np.minimum(65534, 32767 * counts))

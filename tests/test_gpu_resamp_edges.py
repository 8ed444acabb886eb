"""The resampler held to its definition where tests/test_gpu_resamp.py and tests/test_gpu_mix.py do not take it
(include/adsb_hip.h, "Resampling"): at every tile geometry resamp_rows can choose -- tiles of up to 8192 outputs, classes of
32 members that leave half of every wave idle, units that do not divide among the four waves, the largest LDS request --
with pointers at odd multiples of 16 bytes and the offsets that must be refused, one call longer than the 2^30-byte buffer
resource of a tile, and the blocking call's carried output in front of tiles larger than 2048.  Tolerance 0; expectations
come from tests/resamp_support.py, tests/mix_support.py, the CPU oracle and the signal-statistics restatement, never from
the library.  tests/test_resamp_cpu.py proves that rs.EDGE_RATIOS and the first files' ratios meet every tile class."""
import ctypes as C
import time

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import mix_support as ms
from tests import resamp_support as rs
from tests import signal_support as ss
from tests.test_gpu_decim_edges import run_at
from tests.test_gpu_resamp import (CHUNK, CS16, U8, assert_same, ctx, hold_taps, n_in_for, run, shared_boundaries,  # noqa: F401
                                   stretched, t_soapy, tap_counts, tile, widen)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------- 1. every tile class
@pytest.mark.parametrize("L, M", rs.EDGE_RATIOS)
def test_exact_at_every_tile_class(hip_lib, ctx, L, M):
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(11_000 + 131 * L + M)
    for T in tap_counts(L, M):
        K = rs.phase_taps(L, T)
        h = rs.random_phase_taps(rng, T, L)   # every phase at sum |h| = 65534 (a phase of one tap: 32767)
        assert rs.phase_abs_sums(h, L).max() == (65534 if K > 1 else 32767)
        assert T < rs.max_taps(L) or K == min(512, rs.ceil_div(4096, L))
        for s in (0, 1, 14, 16):
            with ctx.resampler(L, M, h, s) as res:
                for count in (0, 1, t - 1, t, t + 1, 2 * t + 1):
                    n_in = n_in_for(count, L, M)
                    x = rs.random_iq(rng, n_in, run=min(K, n_in // 3))
                    res.reset()
                    got = run(res, x)
                    assert len(got) == rs.out_count(L, M, 0, n_in) and count <= len(got) <= count + (L > M)
                    assert np.array_equal(got, rs.resample(x, h, L, M, s)), (L, M, T, s, count)


@pytest.mark.parametrize("L, M", rs.EDGE_RATIOS)
def test_8bit_at_every_tile_class(hip_lib, ctx, L, M):
    """The 8-bit table sits behind the staged outputs, at stage + tile: up to 32 KB further into LDS than at the radios'
    ratios."""
    import torch
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(12_000 + 131 * L + M)
    T = 8 * max(L, M) + 1
    K = rs.phase_taps(L, T)
    h, s = rs.random_phase_taps(rng, T, L), 14
    table = rs.rail_u8_table()
    assert table[0] != 0
    b = rng.integers(0, 256, size=(n_in_for(t + 3, L, M) + 2, 2), dtype=np.uint8)
    b[: K + 5] = 0   # bytes 0 at the start: T8[0] behind the stream's start, zeros in front of it
    want = rs.resample(widen(b, table), h, L, M, s)
    assert len(want) >= t + 3
    other = rs.Stream(h, L, M, s)   # (a history of T8[0] in front of the stream would give something else)
    other.hist[:] = table[0]
    assert not np.array_equal(other.run(widen(b, table))[: K - 1], want[: K - 1])
    ctx.set_u8_table(table)
    try:
        with ctx.resampler(L, M, h, s) as res:
            assert np.array_equal(run(res, b, U8), want)
    finally:
        torch.cuda.synchronize()
        ctx.set_u8_table(None)


@pytest.mark.parametrize("N", [256, 7])
@pytest.mark.parametrize("L, M", rs.EDGE_RATIOS)
def test_mixer_at_every_tile_class(hip_lib, ctx, L, M, N):
    """mix_tile_phase takes stride = R M and back = H + e from the tile's geometry.  A first call of 3 inputs: the long
    one starts at P mod N != 0."""
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng([13, L, M, N])
    T = 8 * max(L, M) + 1
    K = rs.phase_taps(L, T)
    h, s = rs.random_phase_taps(rng, T, L), 14
    w = ms.random_table(rng, N)
    with ctx.resampler(L, M, h, s) as res:
        res.set_mixer(w)
        assert res.mixer_period == N
        for count in (t + 1, 2 * t + 1):
            n_in = rs.inputs_for(L, M, 3, count)
            x = rs.random_iq(rng, 3 + n_in, run=min(K, n_in // 3))
            ref = ms.ResampStream(h, L, M, s, w)
            res.reset()
            for lo, hi in ((0, 3), (3, len(x))):
                assert ref.P % N == lo
                got = run(res, x[lo:hi])
                assert np.array_equal(got, ref.run(x[lo:hi])), (L, M, N, count, lo)
            assert count <= len(got) <= count + (L > M)


# ----------------------------------------------------------------------------------------------- 2. cut-invariance
@pytest.mark.parametrize("L, M, N", [(128, 127, 0), (127, 128, 0), (33, 17, 0), (5, 56, 0), (127, 128, 125), (5, 56, 3)])
@pytest.mark.parametrize("which", ["small", "default", "maximal"])
def test_the_cut_is_invisible(hip_lib, ctx, L, M, N, which):
    """tests/test_gpu_resamp.py's construction at tiles of 32 rows, of more than 2048 outputs and at the LDS limit; N: the
    period of a mixer set on the stream (0: none)."""
    t = tile(hip_lib, L, M)
    T, s = {"small": (L + 1, 1), "default": (8 * max(L, M) + 1, 14), "maximal": (rs.max_taps(L), 16)}[which]
    K = rs.phase_taps(L, T)
    rng = np.random.default_rng([2, L, M, T, N])
    h = rs.random_phase_taps(rng, T, L)
    w = ms.random_table(rng, N) if N else None
    x = rs.random_iq(rng, n_in_for(3 * t, L, M) + 7, run=K)
    want = ms.resample(x, h, L, M, s, w)
    lengths = sorted({0, 1, M - 1, M, M + 1, max(K - 2, 0), K - 1, K, t * M // L + 1})
    plan = rs.cut_plan(rng, len(x), lengths, max(L, M))
    assert set(lengths) <= set(plan)
    ref = ms.ResampStream(h, L, M, s, w)
    with ctx.resampler(L, M, h, s) as res:
        res.set_mixer(w)
        got, at, res_p, res_n, empty, short = [], 0, set(), set(), 0, 0
        for n in plan:
            res_p.add(ref.P % M)
            res_n.add(rs.ceil_div(ref.P * L, M) % L)
            assert res.out_count(n) == ref.out_count(n)
            y = run(res, x[at:at + n])
            assert np.array_equal(y, ref.run(x[at:at + n])), (at, n)
            empty += n > 0 and len(y) == 0
            short += 0 < n < K - 1
            got.append(y)
            at += n
        # every residue of P mod M and every residue mod L that a call's first output can have stood at a cut
        assert res_p == set(range(M)) and res_n == {rs.ceil_div(P * L, M) % L for P in range(M)}
        assert L > M or (res_n == set(range(L)) and empty > 0)
        assert short > 0 or K <= 2
        assert np.array_equal(np.concatenate(got), want)
        # and one call is the same; after reset the same stream gives the same outputs again
        res.reset()
        assert np.array_equal(run(res, x), want)
        res.reset()
        assert np.array_equal(np.concatenate([run(res, x[:K // 2 + 3]), run(res, x[K // 2 + 3:])]), want)


# ----------------------------------------------------------------------------------------------- 3. the accumulator
@pytest.mark.parametrize("L, M, K", [(33, 17, 125), (128, 65, 32)])
def test_a_phase_at_the_bound_in_a_large_tile(hip_lib, ctx, L, M, K):
    """One phase at sum |h| = 65534 with every one of its samples at the rail of the sign that maximises |acc|, both
    polarities, the output on either side of a tile's first: the accumulator lies where these taps and the rails put it,
    between 65534 * 32767 and 65534 * 32768 = 2^31 - 2^16, and does not wrap."""
    t = tile(hip_lib, L, M)
    assert t > 2048
    rng = np.random.default_rng(14_000 + L)
    T = rs.max_taps(L)
    assert rs.phase_taps(L, T) == K
    h = rs.random_phase_taps(rng, T, L)
    for n0 in (t - 1, t + 1):
        for pol in (1, -1):
            x = rs.random_iq(rng, n_in_for(t + 2, L, M), run=0)
            acc, weight = rs.rail_window(x, h, L, M, n0, pol)
            # the last output of the first tile and the second of the second: their windows lie across the second tile's
            # origin, the newest input of output t less K - 1
            q, taps = (n0 * M) // L, len(h[(n0 * M) % L::L])
            assert taps in (K - 1, K) and q - (taps - 1) <= (t * M) // L - (K - 1) + 1 and (t * M) // L - 1 <= q
            assert weight == 65534 and acc * pol > 0 and 65534 * 32767 <= abs(acc) <= 65534 * 32768
            for s in (0, 16):
                r = (1 << (s - 1)) if s else 0
                assert abs(acc + r) < 2 ** 31
                with ctx.resampler(L, M, h, s) as res:
                    got = run(res, x)
                assert got[n0].tolist() == [min(max((acc + r) >> s, -32768), 32767)] * 2
                assert np.array_equal(got, rs.resample(x, h, L, M, s))


# ----------------------------------------------------------------------------------------------- 4. pointers
def pointer_stream(rng, L, M, t, fmt):
    """(taps, shift, two tiles and one output's inputs, what they resample to)."""
    T, s = 8 * max(L, M) + 1, 14
    h = rs.random_phase_taps(rng, T, L)
    n_in = n_in_for(2 * t + 1, L, M)
    if fmt == U8:
        x = rng.integers(0, 256, size=(n_in, 2), dtype=np.uint8)
        return h, s, x, rs.resample(widen(x, t_soapy()), h, L, M, s)
    x = rs.random_iq(rng, n_in, run=rs.phase_taps(L, T))
    return h, s, x, rs.resample(x, h, L, M, s)


@pytest.mark.parametrize("fmt", [CS16, U8])
@pytest.mark.parametrize("L, M", [(6, 5), (128, 127)])
def test_pointers_at_odd_multiples_of_16_bytes(hip_lib, ctx, L, M, fmt):
    """The header asks for 16 bytes, torch hands out hundreds: here the input sits at 16 and 48 bytes past a 64-byte
    boundary and the outputs at 16, junk around the input and guards around the outputs.  Two tiles and one output, from
    reset and behind a first call of 3 M + 1 inputs."""
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(15_000 + 2 * L + fmt)
    h, s, x, want = pointer_stream(rng, L, M, t, fmt)
    first = 3 * M + 1
    with ctx.resampler(L, M, h, s) as res:
        for in_off, out_off in [(16, 16), (48, 16), (48, 0), (0, 16)]:
            res.reset()
            assert np.array_equal(run_at(res, x, fmt, in_off, out_off), want), (in_off, out_off)
            res.reset()
            parts = [run_at(res, x[:first], fmt, in_off, out_off), run_at(res, x[first:], fmt, in_off, out_off)]
            assert len(parts[0]) == rs.out_count(L, M, 0, first) > 0 and len(parts[1]) > 2 * t - len(parts[0])
            assert np.array_equal(np.concatenate(parts), want), (in_off, out_off)


@pytest.mark.parametrize("fmt", [CS16, U8])
@pytest.mark.parametrize("L, M", [(6, 5), (128, 127)])
def test_misaligned_pointers_are_refused_and_consume_nothing(hip_lib, ctx, L, M, fmt):
    import torch
    from dump1090_rs_amd import _lib
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(15_100 + 2 * L + fmt)
    h, s, x, want = pointer_stream(rng, L, M, t, fmt)
    with ctx.resampler(L, M, h, s) as res:
        head = run(res, x[:100], fmt)
        rest = np.ascontiguousarray(x[100:])
        probes = [res.out_count(k) for k in range(1, 2 * M + 1)]
        cap = res.out_count(len(rest))
        with torch.cuda.stream(ctx.torch_stream):
            d_in = torch.zeros(rest.nbytes + 64, dtype=torch.uint8, device="cuda")
            d_out = torch.full((cap + 16, 2), 0x5A5A, dtype=torch.int16, device="cuda")
            assert d_in.data_ptr() % 64 == 0 and d_out.data_ptr() % 64 == 0
            for off in (2, 4, 8):
                for in_off, out_off in ((off, 0), (0, off), (off, off)):
                    n = C.c_size_t()
                    st = res._L.adsb_resamp_run_device(res._h, fmt, C.c_void_p(d_in.data_ptr() + in_off), len(rest),
                                                       C.c_void_p(d_out.data_ptr() + out_off), cap, C.byref(n))
                    assert st == _lib.ADSB_ERR_INVALID, (off, in_off, out_off)
                    assert [res.out_count(k) for k in range(1, 2 * M + 1)] == probes and res.out_count(len(rest)) == cap
            assert (d_out.cpu().numpy() == 0x5A5A).all()
        assert np.array_equal(np.concatenate([head, run(res, rest, fmt)]), want)   # the stream goes on where it was


# ----------------------------------------------------------------------------------------------- 5. past the resource cap
def test_one_call_longer_than_a_tiles_buffer_resource(hip_lib, ctx):
    """k_resamp gives a tile a buffer resource of the bytes left behind its origin, 2^30 at most.  2^28 + 3 t M / L + 5
    CS16 samples at 3/25 leave more than that behind the first tiles: outputs are checked in the first two tiles, the
    two on either side of the tile where the bytes left fall below 2^30, and the last two, the ragged one included.
    1.1 GiB of device memory; only the windows come back."""
    import torch
    L, M = 3, 25
    t = tile(hip_lib, L, M)
    T, s = 8 * M + 1, 14
    K = rs.phase_taps(L, T)
    h = rs.random_phase_taps(np.random.default_rng(16_000), T, L)
    n_in = 2 ** 28 + 3 * t * M // L + 5
    n_out = rs.out_count(L, M, 0, n_in)
    blocks = rs.ceil_div(n_out, t)

    def left(blk):
        return (n_in - rs.tile_base(blk, 0, L, M, K, t)) * 4

    switch = next(b for b in range(blocks) if left(b) < 2 ** 30)
    assert left(0) > 2 ** 30 and left(switch - 1) >= 2 ** 30 and 2 <= switch <= blocks - 4 and n_out % t
    windows = [(0, 2 * t), ((switch - 2) * t, 4 * t), ((blocks - 2) * t, n_out - (blocks - 2) * t)]
    with ctx.resampler(L, M, h, s) as res:
        assert res.out_count(n_in) == n_out
        with torch.cuda.stream(ctx.torch_stream):
            d_in = torch.randint(-32768, 32768, (n_in, 2), dtype=torch.int16, device="cuda")
            d_out = torch.full((n_out + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
            ctx.torch_stream.synchronize()
            t0 = time.perf_counter()
            assert res.run_device(d_in.data_ptr(), n_in, d_out.data_ptr(), n_out) == n_out
            ctx.torch_stream.synchronize()
            print(f"3/25, {n_in} inputs, {n_out} outputs in {blocks} tiles: {time.perf_counter() - t0:.4f} s")
            for first, count in windows:
                lo, hi = rs.window_inputs(first, count, T, L, M)
                xw = d_in[lo:hi].cpu().numpy()
                assert xw.min() < -30000 and xw.max() > 30000
                got = d_out[first:first + count].cpu().numpy()
                assert np.array_equal(got, rs.resample_window(xw, first, count, h, L, M, s)), (first, count)
            assert (d_out[n_out:].cpu().numpy() == 0x5A5A).all()
            del d_in, d_out
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------- 6. the carried output
def start_with_both_kinds(L, M, n_out, piece_out):
    """The least P > 0 behind which a blocking call of n_out outputs has a shared piece boundary and one that is not."""
    for P in range(1, L * M):
        kinds = {sh for _, sh in shared_boundaries(L, M, P, rs.inputs_for(L, M, P, n_out), piece_out)}
        if kinds == {True, False}:
            return P
    raise AssertionError("no such start")


@pytest.mark.parametrize("L, M, max_chunks, P, pieces, want_shared", [(96, 95, 1, 64, 4, [1, 4]), (33, 17, 2, None, 2, None)])
def test_the_blocking_call_carries_an_output_across_a_large_tile(hip_lib, oracle_mod, L, M, max_chunks, P, pieces, want_shared):
    """tests/test_gpu_resamp.py's stream of calls at tiles of 6144 and 2112 outputs: where the outputs on both sides of a
    piece boundary share their newest input, the piece in front of it makes one output more than its buffers hold, and the
    next piece's kernel writes behind it, at staged + 1: 4-byte aligned only, the dword-store branch of the final store
    loop, which then makes up to 24 passes.  96/95 from P = 64: the call's first output is 65, and (b M) mod L >= M only for
    b = 1 mod 96, so with 131 072 = 32 mod 96 exactly boundaries 1 and 4 are shared.  Every buffer's signal statistics are
    compared (sums over all of its samples: one wrong or moved sample shows), and the frames where there are any."""
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
    t = tile(hip_lib, L, M)
    assert t > 2048 and L > M
    h, s = hold_taps(L), 14
    piece_out = max_chunks * CHUNK
    n_big = pieces * piece_out + 60_001
    if P is None:
        P = start_with_both_kinds(L, M, n_big, piece_out)
    big = rs.inputs_for(L, M, P, n_big)
    shared = shared_boundaries(L, M, P, big, piece_out)
    assert len(shared) == pieces and {sh for _, sh in shared} == {True, False}
    assert want_shared is None or (rs.out_range(L, M, P, big)[0] == P + 1 and [k for k, sh in shared if sh] == want_shared)
    cuts = [P, 0, big, 1, 29_999]
    base = synth.make_iq(rs.ceil_div(sum(cuts) * L, M) + 16, n_bursts=300, seed=17_000 + L, n_icao=20, df11_every=3)
    x = stretched(base, L, M)[: sum(cuts)]
    assert len(x) == sum(cuts)
    orc, ref = oracle_mod.Oracle(), rs.Stream(h, L, M, s)
    counts, total = [], 0
    with Context(0, max_chunks) as c, c.resampler(L, M, h, s) as res:
        c.icao_flush()
        c.set_signal_stats(True)
        at = 0
        for n in cuts:
            y = ref.run(x[at:at + n])
            counts.append(len(y))
            want, _ = orc.demod_iq(y, cap=1 << 16) if len(y) else ([], None)
            if n == big and L == 96:   # (frames behind every carried output: a carry gone wrong moves them by a sample)
                assert {k * max_chunks for k, sh in shared if sh} <= {w["chunk"] for w in want}
            assert_same(res.demod_iq(x[at:at + n], cap=1 << 16), want)
            if len(y):
                got_sig, want_sig = c.signal_stats(), ss.restated(oracle_mod.Oracle(), y, y, SIGNAL_STATS_DTYPE)
                assert len(got_sig) == len(want_sig) == rs.ceil_div(len(y), CHUNK)
                for name in want_sig.dtype.names:
                    assert np.array_equal(got_sig[name], want_sig[name]), (n, name)
            total += len(want)
            at += n
    assert counts[1] == 0 and n_big <= counts[2] <= n_big + 1
    assert total > 50 or L != 96

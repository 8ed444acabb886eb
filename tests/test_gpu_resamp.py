"""The resampler on the device (include/adsb_hip.h, "Resampling"), held bit for bit to the numpy restatement of its
definition (tests/resamp_support.py), and its frames to the reference's and the CPU oracle's.  Shapes are built from
t = adsb_resamp_selftest_tile(L, M), the outputs one workgroup takes: around one and two tiles of outputs, every residue
of the first output mod L and of P mod M at a cut, calls that produce nothing, calls shorter than the history.  Every
comparison is at tolerance 0."""
import subprocess

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import decim_support as ds
from tests import fix_support as fs
from tests import resamp_support as rs
from tests import signal_support as ss
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK = 131072
CS16, U8 = 0, 1


def t_soapy() -> np.ndarray:
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


def widen(b: np.ndarray, table: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(table[b.reshape(-1, 2)])


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msglen, m.msg.hex(), m.signal_level)


def assert_same(msgs, want):
    exp = [(w["chunk"], w["j"], w["try_phase"], w["score"], w["len"], w["msg"].hex(), w["signal_level"]) for w in want]
    assert [key(m) for m in msgs] == exp


@pytest.fixture()
def ctx(hip_lib):
    """A context whose input is ordered behind a torch stream (adsb_set_stream): run() copies in, resamples and reads
    back in that stream's order, with no other synchronisation."""
    import torch
    from dump1090_rs_amd import Context
    with Context(0, 1) as c:
        c.torch_stream = torch.cuda.Stream()
        c.set_stream(c.torch_stream.cuda_stream)
        yield c
        torch.cuda.synchronize()


def tile(hip_lib, L: int, M: int) -> int:
    t = int(hip_lib.adsb_resamp_selftest_tile(L, M))
    assert t >= L and t % L == 0
    return t


def run(res, x: np.ndarray, fmt: int = CS16, cap=None) -> np.ndarray:
    """One adsb_resamp_run_device call on x ((n, 2) int16, or uint8 for the 8-bit format) -> its outputs, (n_out, 2) int16."""
    import torch
    want_n = res.out_count(len(x))
    cap = want_n if cap is None else cap
    with torch.cuda.stream(res._ctx.torch_stream):
        d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d_out = torch.full((max(cap, 1) + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        n = res.run_device(d_in.data_ptr(), len(x), d_out.data_ptr(), cap, format=fmt)
        assert n == want_n
        y = d_out.cpu().numpy()
    assert (y[n:] == 0x5A5A).all()   # the canary: nothing written behind the call's outputs
    return y[:n]


def n_in_for(count: int, L: int, M: int) -> int:
    """The fewest inputs that give at least `count` outputs from the start of a stream: up to the newest input of output
    count - 1.  (Where L > M that input can be output count's as well: one output more.)"""
    return 0 if count == 0 else ((count - 1) * M) // L + 1


def tap_counts(L: int, M: int):
    return sorted({1, L, L + 1, 8 * max(L, M) + 1, rs.max_taps(L)})


# ----------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("L, M", [(1, 5), (6, 5), (3, 4), (24, 25), (3, 25), (15, 16), (1, 1), (24, 125)])
def test_exact_against_numpy(hip_lib, ctx, L, M):
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(1000 + 131 * L + M)
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


# ----------------------------------------------------------------------------------------------- 2. L = 1: the decimator
@pytest.mark.parametrize("M", [2, 16])
def test_equal_to_the_decimators_definition_at_l_1(hip_lib, ctx, M):
    t = tile(hip_lib, 1, M)
    rng = np.random.default_rng(1500 + M)
    for T, s in [(1, 0), (8 * M + 1, 15), (512, 16)]:
        h = ds.random_taps(rng, T)
        x = rs.random_iq(rng, (2 * t + 1) * M + 1, run=T)
        with ctx.resampler(1, M, h, s) as res:
            ref = ds.Stream(h, M, s)
            cut = T // 2 + M + 1
            parts = []
            for a, b in [(0, cut), (cut, len(x))]:
                assert res.out_count(b - a) == ref.out_count(b - a)
                parts.append(run(res, x[a:b]))
                assert np.array_equal(parts[-1], ref.run(x[a:b]))
            assert np.array_equal(np.concatenate(parts), ds.decimate(x, h, M, s))


# ----------------------------------------------------------------------------------------------- 3. cut-invariance
@pytest.mark.parametrize("L, M", [(6, 5), (24, 25), (3, 25)])
@pytest.mark.parametrize("which", ["small", "default", "maximal"])
def test_the_cut_is_invisible(hip_lib, ctx, L, M, which):
    t = tile(hip_lib, L, M)
    T, s = {"small": (L + 1, 1), "default": (8 * max(L, M) + 1, 14), "maximal": (rs.max_taps(L), 16)}[which]
    K = rs.phase_taps(L, T)
    rng = np.random.default_rng(2000 + 1000 * L + 7 * M + T)
    h = rs.random_phase_taps(rng, T, L)
    x = rs.random_iq(rng, n_in_for(3 * t, L, M) + 7, run=K)
    want = rs.resample(x, h, L, M, s)
    lengths = sorted({0, 1, M - 1, M, M + 1, max(K - 2, 0), K - 1, K, t * M // L + 1})
    plan = rs.cut_plan(rng, len(x), lengths, max(L, M))
    assert set(lengths) <= set(plan)
    ref = rs.Stream(h, L, M, s)
    with ctx.resampler(L, M, h, s) as res:
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


# ----------------------------------------------------------------------------------------------- 4. rounding, clamping
def test_rounding_and_clamping(hip_lib, ctx):
    # 2/1 with one tap per phase: y[n] = (x[n div 2] + 1) >> 1 -- a half rounds up
    with ctx.resampler(2, 1, [1, 1], 1) as res:
        x = np.array([[-3, 3], [-1, 1], [1, -1], [3, -3]], np.int16)
        assert run(res, x).tolist() == [[-1, 2], [-1, 2], [0, 1], [0, 1], [1, 0], [1, 0], [2, -1], [2, -1]]
    # 1/2: y[n] = clamp(32767 (x[2 n] + x[2 n - 1]))
    with ctx.resampler(1, 2, [32767, 32767], 0) as res:
        x = np.array([[-32768, 32767]] * 6 + [[32767, -32768]] * 6, np.int16)
        got = run(res, x)
        assert got[1:3].tolist() == [[-32768, 32767]] * 2 and got[4:].tolist() == [[32767, -32768]] * 2
        assert np.array_equal(got, rs.resample(x, [32767, 32767], 1, 2, 0))


@pytest.mark.parametrize("L, M", [(6, 5), (3, 10)])
def test_a_phase_at_the_bound_against_the_rails(hip_lib, ctx, L, M):
    """Phase p0 at sum |h| = 65534, every one of its samples at the rail of the sign that maximises |acc|, both polarities:
    the accumulator comes within 2^17 of 2^31 and does not wrap."""
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(4000 + L)
    K = 512
    T = rs.max_taps(L)
    h = rs.random_phase_taps(rng, T, L)
    h64 = h.astype(np.int64)
    for n0 in (t - 1, t + 1):
        p, q = (n0 * M) % L, (n0 * M) // L
        assert len(h64[p::L]) == K and np.abs(h64[p::L]).sum() == 65534 and q >= K - 1
        for pol in (1, -1):
            x = rs.random_iq(rng, n_in_for(t + 2, L, M), run=0)
            for j in range(K):
                x[q - j] = ds.rail_for(h64[p + j * L], pol)
            acc = sum(int(h64[p + j * L]) * int(x[q - j, 0]) for j in range(K))
            assert acc * pol > 0 and 2 ** 31 - 2 ** 17 <= abs(acc) < 2 ** 31 - 32768
            for s in (0, 16):
                r = (1 << (s - 1)) if s else 0
                with ctx.resampler(L, M, h, s) as res:
                    got = run(res, x)
                assert got[n0].tolist() == [min(max((acc + r) >> s, -32768), 32767)] * 2
                assert np.array_equal(got, rs.resample(x, h, L, M, s))


# ----------------------------------------------------------------------------------------------- 5. 8-bit
@pytest.mark.parametrize("L, M", [(3, 10), (6, 5)])
@pytest.mark.parametrize("table_name", ["soapy", "rails"])
def test_8bit_input(hip_lib, ctx, L, M, table_name):
    import torch
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(3000 + L)
    T = 8 * max(L, M) + 1
    K = rs.phase_taps(L, T)
    h, s = rs.random_phase_taps(rng, T, L), 14
    table = t_soapy() if table_name == "soapy" else rs.rail_u8_table()
    assert table[0] != 0
    b = rng.integers(0, 256, size=(n_in_for(t + 3, L, M) + 2, 2), dtype=np.uint8)
    b[: K + 5] = 0   # bytes 0 at the start: T8[0] behind the stream's start, zeros in front of it
    want = rs.resample(widen(b, table), h, L, M, s)
    # (a history of T8[0] in front of the stream would give something else in the first K - 1 outputs' reach, so the
    # comparison can tell)
    other = rs.Stream(h, L, M, s)
    other.hist[:] = table[0]
    assert not np.array_equal(other.run(widen(b, table))[: K - 1], want[: K - 1])
    ctx.set_u8_table(table)
    try:
        with ctx.resampler(L, M, h, s) as res:
            assert np.array_equal(run(res, b, U8), want)
            res.reset()
            assert np.array_equal(run(res, b, U8), want)
            # a stream that alternates CS16 calls and 8-bit calls of the same widened samples
            res.reset()
            cuts = [0, 1, K // 2 + 1, K + M, len(b) // 2, len(b)]
            parts = []
            for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
                parts.append(run(res, b[lo:hi], U8) if i % 2 else run(res, widen(b[lo:hi], table)))
            assert np.array_equal(np.concatenate(parts), want)
            # the table changed between two calls of one stream, after a stream synchronise: the history stays widened
            # through the old table, the new call's bytes go through the new one
            cs8 = (np.arange(256).astype(np.uint8).view(np.int8).astype(np.int16) << 8).astype(np.int16)
            cut = len(b) // 2 + 1
            res.reset()
            first = run(res, b[:cut], U8)
            torch.cuda.synchronize()
            ctx.set_u8_table(cs8)
            second = run(res, b[cut:], U8)
            mixed = np.concatenate([widen(b[:cut], table), widen(b[cut:], cs8)])
            assert np.array_equal(np.concatenate([first, second]), rs.resample(mixed, h, L, M, s))
    finally:
        torch.cuda.synchronize()
        ctx.set_u8_table(None)


# ----------------------------------------------------------------------------------------------- 6. capacity
def test_capacity_consumes_nothing(hip_lib, ctx):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd._lib import AdsbError
    L, M, T, s = 6, 5, 49, 14
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(5)
    h = rs.random_phase_taps(rng, T, L)
    x = rs.random_iq(rng, n_in_for(t + 5, L, M) + 1, run=9)
    want = rs.resample(x, h, L, M, s)
    with ctx.resampler(L, M, h, s) as res:
        first = run(res, x[:100])
        n = res.out_count(len(x) - 100)
        with pytest.raises(AdsbError) as e:
            run(res, x[100:], cap=n - 1)
        assert e.value.status == _lib.ADSB_ERR_CAPACITY and e.value.required == n
        assert res.out_count(len(x) - 100) == n
        assert np.array_equal(np.concatenate([first, run(res, x[100:])]), want)


# ----------------------------------------------------------------------------------------------- 7. frames, pinned
@pytest.mark.parametrize("L, M", [(2, 5), (24, 25), (3, 25)])
def test_held_golden_captures_give_the_reference_frames(hip_lib, golden, fixture_iq, L, M):
    import torch
    from dump1090_rs_amd import Context
    rng = np.random.default_rng(7000 + L)
    with Context(0, 1) as c, c.resampler(L, M, [1] * L, 0) as res:
        for fx in golden["fixtures"]:
            x = rs.hold_input(fixture_iq[fx["file"]], L, M, rng)   # x[floor(n M / L)] = capture[n], random elsewhere
            c.icao_flush()
            res.reset()
            got = res.demod_iq(x)
            assert [m.buffer().hex() for m in got] == fx["frames"] and len(got) in (5, 6)
            assert [m.j for m in got] == fx["j"] and [m.try_phase for m in got] == fx["try_phase"]
            # run_device + submit + collect, nothing in between: the pass waits for the resampler by itself
            d_in = torch.from_numpy(x).cuda()
            d_out = torch.empty((CHUNK, 2), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            c.icao_flush()
            res.reset()
            n = res.run_device(d_in.data_ptr(), len(x), d_out.data_ptr(), CHUNK)
            c.submit_iq_device(d_out.data_ptr(), n)
            again = c.collect()
            assert n == CHUNK and [key(m) for m in again] == [key(m) for m in got]


# ----------------------------------------------------------------------------------------------- 8. a real filter
@pytest.mark.parametrize("L, M", [(24, 25), (2, 5), (6, 25), (6, 5)])
def test_golden_captures_through_the_default_filter_match_the_oracle(hip_lib, oracle_mod, golden, fixture_iq, L, M):
    """Each capture as a radio at 2.4 MS/s x M / L would have delivered it -- the capture resampled by M / L -- brought
    back by the default filter, equal to the oracle on the restatement.  The share of the reference's frames that come back
    is printed, not asserted (DESIGN has the figures)."""
    from dump1090_rs_amd import Context, default_resampler_taps
    h = rs.hamming_sinc_taps(L, M)   # numpy's table of the default taps' formula: the expectation does not hang on libm
    lib_taps, shift = default_resampler_taps(L, M)
    assert shift == 14 and len(lib_taps) == len(h)
    orc = oracle_mod.Oracle()
    total = 0
    with Context(0, 1) as c, c.resampler(L, M, h, 14) as res:
        for fx in golden["fixtures"]:
            x = rs.resample(fixture_iq[fx["file"]], rs.hamming_sinc_taps(M, L), M, L, 14)
            orc.icao_flush()
            want, _ = orc.demod_iq(rs.resample(x, h, L, M, 14))
            print(f"{L}/{M} {fx['file']}: {len(want)} frames, {len(set(w['buffer'].hex() for w in want) & set(fx['frames']))} of them "
                  f"among the reference's {len(fx['frames'])}")
            total += len(want)
            c.icao_flush()
            res.reset()
            assert_same(res.demod_iq(x), want)
    assert total >= 1   # (a precondition, not a tolerance: the comparison is not empty)


# ----------------------------------------------------------------------------------------------- 9. a stream of calls
def hold_taps(L: int) -> np.ndarray:
    """Boxcar-like: mostly the newest input, a little of the one before (K = 2: the history is in play).  Shift 14."""
    return np.concatenate([np.full(L, 15000, np.int16), np.full(L, 1384, np.int16)])


def stretched(base: np.ndarray, L: int, M: int) -> np.ndarray:
    """base (at 2.4 MS/s) as a radio at 2.4 MS/s x M / L would roughly see it: held where that rate is higher, resampled
    by the numpy restatement where it is lower."""
    if L > M:
        return rs.resample(base, rs.hamming_sinc_taps(M, L), M, L, 14)
    m = np.arange(((len(base) - 1) * M) // L + 1)
    return np.ascontiguousarray(base[-((-m * L) // M)])   # x[floor(n M / L)] = base[n]: input m holds base[ceil(m L / M)]


def shared_boundaries(L: int, M: int, P: int, n_in: int, piece_out: int):
    """The piece boundaries of one blocking call -- every piece_out outputs of the call -- as (k, shared): shared where the
    outputs on both sides of boundary k have the same newest input, so that no cut of the input separates them and the
    piece in front of it produces one output more than it holds."""
    first, count = rs.out_range(L, M, P, n_in)
    edges = range(first + piece_out, first + count, piece_out)
    return [(k + 1, ((b - 1) * M) // L == (b * M) // L) for k, b in enumerate(edges)]


def test_a_stream_over_several_demod_calls(hip_lib, oracle_mod):
    from dump1090_rs_amd import Context
    total = 0
    for L, M, max_chunks, fmt in [(6, 5, 1, CS16), (3, 10, 2, CS16), (4, 5, 16, U8)]:
        h, s = hold_taps(L), 14
        # a call that spans four one-buffer pieces and a bit (6/5), two two-buffer pieces and a bit (3/10), one piece
        # (4/5), calls of no input and of one input that yields no output (3/10 and 4/5: input 50 004 is no output's
        # newest), and a rest.  At 6/5 the long call starts at P = 50 004: its first output is 60 005, so the outputs on
        # both sides of its first and of its fourth buffer boundary (191 077, 584 293: 1 mod 6) share their newest input,
        # and the surplus output is carried into a middle piece and into the last one (both have frames to show it).
        pieces = {1: 4, 2: 2, 16: 1}[max_chunks]
        piece_out = min(max_chunks, 16) * CHUNK
        big = n_in_for(pieces * min(max_chunks, 2) * CHUNK + (60_001 if L > M else 12_345), L, M)
        cuts = [50_004, 0, big, 1, 29_999] if L > M else [50_004, 0, 1, big, 29_999]
        i_big = cuts.index(big)
        shared = shared_boundaries(L, M, sum(cuts[:i_big]), big, piece_out)
        if L > M:
            assert len(shared) == 4 and [k for k, sh in shared if sh] == [1, 4]
        else:
            assert not any(sh for _, sh in shared)
        out_total = rs.ceil_div(sum(cuts) * L, M)
        base = synth.make_iq(out_total + 16, n_bursts=300, seed=900 + L, n_icao=20, df11_every=3)
        if fmt == U8:
            table = t_soapy()
            raw = np.ascontiguousarray(np.clip(np.rint(base / 256.0 + 127.4), 0, 255).astype(np.uint8))
            x = stretched(raw, L, M)[: sum(cuts)]
            xw = widen(x, table)
        else:
            x = xw = stretched(base, L, M)[: sum(cuts)]
        assert len(x) == sum(cuts)
        orc, ref = oracle_mod.Oracle(), rs.Stream(h, L, M, s)
        counts = []
        with Context(0, max_chunks) as c, c.resampler(L, M, h, s) as res:
            c.icao_flush()
            c.set_signal_stats(L > M)   # (6/5: every buffer's sum of squares, so that one wrong sample shows)
            at = 0
            for n in cuts:
                y = ref.run(xw[at:at + n])
                counts.append(len(y))
                want, _ = orc.demod_iq(y, cap=1 << 16) if len(y) else ([], None)
                if n == big:   # (frames behind every carried output: a carry gone wrong moves them by a sample)
                    assert {k for k, sh in shared if sh} <= {w["chunk"] for w in want}
                assert_same(res.demod_iq(x[at:at + n], format=fmt, cap=1 << 16), want)
                if L > M and len(y):
                    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
                    got_sig, want_sig = c.signal_stats(), ss.restated(oracle_mod.Oracle(), y, y, SIGNAL_STATS_DTYPE)
                    assert len(got_sig) == len(want_sig) == rs.ceil_div(len(y), CHUNK)
                    for name in want_sig.dtype.names:
                        assert np.array_equal(got_sig[name], want_sig[name]), (n, name)
                total += len(want)
                at += n
        assert counts[1] == 0 and counts[i_big] > pieces * min(max_chunks, 2) * CHUNK
        assert L > M or counts[2] == 0   # (the single input 50 004 reaches no output)
    assert total > 50


# ----------------------------------------------------------------------------------------------- 10. context modes
EDGE = CHUNK + 50_001


@pytest.mark.parametrize("L, M, max_chunks", [(3, 10, 1), (4, 5, 2)])
def test_carry_over_through_the_resampler(hip_lib, oracle_mod, L, M, max_chunks):
    """A DF17 planted across output sample CHUNK (a buffer boundary inside the first call) and one across EDGE (the edge
    between two calls): found with carry-over, lost without, exactly as the oracle's carry path says."""
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    n_base = 2 * CHUNK + 70_001
    edges = (CHUNK, EDGE)
    planted = [synth.df17_frame(0xABC000 + k, 0x11223344556600 + k) for k in range(2)]
    bursts = [b for b in synth.plan_bursts(n_base, 200, 4343, n_icao=20, df11_every=3)
              if all(abs(b.tick // 5 - at) > 800 for at in edges)]
    base = synth.noise_numpy(n_base, 4343)
    synth.add_bursts(base, bursts + [synth.Burst(5 * (at - 100) + k, 20000, 3 + 2 * k, planted[k]) for k, at in enumerate(edges)])
    rng = np.random.default_rng(10_000 + L)
    x = rs.hold_input(base, L, M, rng)
    h, s = [1] * L, 0
    assert np.array_equal(rs.resample(x, h, L, M, s), base)
    cut = n_in_for(EDGE, L, M)
    calls, pieces = [x[:cut], x[cut:]], [base[:EDGE], base[EDGE:]]
    assert rs.out_count(L, M, 0, cut) == EDGE
    orc, carry = oracle_mod.Oracle(), np.zeros((326, 2), np.int16)
    with_carry = [demod_iq_carry(orc, p, carry, cap=1 << 16)[0] for p in pieces]
    orc = oracle_mod.Oracle()
    plain = [orc.demod_iq(p, cap=1 << 16)[0] for p in pieces]
    found = [bytes(w["buffer"]) for part in with_carry for w in part]
    assert all(found.count(fr) == 1 for fr in planted)
    assert not any(fr == bytes(w["buffer"]) for part in plain for w in part for fr in planted)
    with Context(0, max_chunks) as c, c.resampler(L, M, h, s) as res:
        c.set_carry_over(True)
        c.icao_flush()
        for part, want in zip(calls, with_carry):
            assert_same(res.demod_iq(part, cap=1 << 16), want)
        c.set_carry_over(False)
        c.icao_flush()
        res.reset()
        for part, want in zip(calls, plain):
            assert_same(res.demod_iq(part, cap=1 << 16), want)


def test_error_correction_through_the_resampler(hip_lib, oracle_mod):
    from dump1090_rs_amd import Context, _lib
    L, M = 2, 5
    one, _, _ = fs.damaged_capture()
    iq1 = np.concatenate([one, one])   # two buffers: the second piece starts with the first's filter
    x = rs.hold_input(iq1, L, M, np.random.default_rng(10_500))
    h, s = [1] * L, 0
    want = fs.Restated(_lib.ADSB_FIX_1BIT).demod_iq(rs.resample(x, h, L, M, s))
    assert 1200 in {k[1] for k in want} and {k[4] for k in want} == {0, 1}
    with Context(0, 1) as c, c.resampler(L, M, h, s) as res:
        c.set_error_correction(_lib.ADSB_FIX_1BIT)
        c.icao_flush()
        assert [fs.key(m) for m in res.demod_iq(x, cap=1 << 16)] == want


# ----------------------------------------------------------------------------------------------- 11. adsb_feed
def test_adsb_feed_resample(hip_lib, oracle_mod, golden, fixture_iq, tmp_path):
    from dump1090_rs_amd import default_resampler_taps
    L, M = 6, 25
    fx = golden["fixtures"][2]
    x = stretched(fixture_iq[fx["file"]], L, M)   # the capture as an Airspy at 10 MS/s would roughly have seen it
    path = tmp_path / "x10.iq"
    np.ascontiguousarray(x[:, ::-1]).astype("<i2").tofile(path)   # the capture format: im first
    h, s = default_resampler_taps(L, M)
    want, _ = oracle_mod.Oracle().demod_iq(rs.resample(x, h, L, M, s))
    assert len(want) > 0
    r = subprocess.run([str(ROOT / "dump1090_rs_amd" / "adsb_feed"), "--resample", f"{L}/{M}", "--buffers", "2", str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["*" + w["buffer"].hex() + ";" for w in want]
    assert f"resampled by {L}/{M}" in r.stderr.splitlines()[-1]
    both = subprocess.run([str(ROOT / "dump1090_rs_amd" / "adsb_feed"), "--resample", f"{L}/{M}", "--decimate", "2", str(path)],
                          capture_output=True, text=True, timeout=120)
    assert both.returncode == 2 and "usage" in both.stderr

"""The decimator held to what its header promises and tests/test_gpu_decim.py leaves unchecked (include/adsb_hip.h,
"Decimation"): every factor 2..16 against the int64 restatement, the int32 accumulator at the limit sum |h| <= 65534
allows (the tap -32768 included), pointers at odd multiples of 16 bytes and the arguments that must be refused, one call
longer than the 2^30-byte buffer resource of a tile, and the context's modes -- carry-over, signal statistics, both repair
modes, ADSB_ERR_CAPACITY and ADSB_ERR_BUSY -- through adsb_decim_demod_iq and the asynchronous form.  Tolerance 0;
expectations come from tests/decim_support.py, the CPU oracle and the suites' restatements, never from the library.
tests/test_decim_cpu.py proves on the restatement alone that the inputs reach what they are meant to reach."""
import ctypes as C

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import decim_support as ds
from tests import fix2_support as f2
from tests import fix_support as fs
from tests import signal_support as ss
from tests.test_gpu_decim import CHUNK, CS16, U8, assert_same, ctx, key, n_in_for, run, t_soapy, tile, widen  # noqa: F401

pytestmark = pytest.mark.gpu


def run_split(dec, x, cuts, fmt=CS16):
    """The stream x from reset in calls cut at `cuts` -> all outputs."""
    dec.reset()
    edges = [0, *cuts, len(x)]
    return np.concatenate([run(dec, x[a:b], fmt) for a, b in zip(edges, edges[1:])])


# ----------------------------------------------------------------------------------------------- 1. every factor
@pytest.mark.parametrize("D", range(2, 17))
def test_every_factor_is_exact(hip_lib, ctx, D):
    t = tile(hip_lib)
    rng = np.random.default_rng(6000 + D)
    n_in = n_in_for(2 * t + 1, D)
    for T in ds.grid_taps(D):
        h = ds.random_taps(rng, T)
        x = ds.random_iq(rng, n_in, run=min(T, n_in // 3))
        with ctx.decimator(D, h, 15) as dec:
            dec.reset()
            got = run(dec, x)
            assert len(got) == 2 * t + 1
            assert np.array_equal(got, ds.decimate(x, h, D, 15)), (D, T)


@pytest.mark.parametrize("D", range(2, 17))
def test_every_factor_hides_the_cut(hip_lib, ctx, D):
    t = tile(hip_lib)
    rng = np.random.default_rng(6100 + D)
    T, s = 8 * D + 1, 15
    h = ds.random_taps(rng, T)
    x = ds.random_iq(rng, 2 * t * D + 7, run=T)
    want = ds.decimate(x, h, D, s)
    lengths = sorted({0, 1, D - 1, D, D + 1, T - 2, T - 1, T, t * D // 2 + 1})
    plan = ds.cut_plan(rng, len(x), lengths, D)
    assert set(lengths) <= set(plan) and any(0 < n < T - 1 for n in plan)
    ref = ds.Stream(h, D, s)
    with ctx.decimator(D, h, s) as dec:
        got, at, residues = [], 0, set()
        for n in plan:
            residues.add(ref.P % D)
            assert dec.out_count(n) == ref.out_count(n)
            y = run(dec, x[at:at + n])
            assert np.array_equal(y, ref.run(x[at:at + n])), (D, at, n)
            got.append(y)
            at += n
        assert at == len(x) and residues == set(range(D))
        assert np.array_equal(np.concatenate(got), want)


def test_the_grid_meets_both_cases_of_the_row_length(hip_lib):
    """decim_row_len's `| 1` bumps an even ceil((tile D + T + 15) / D) and leaves an odd one: both are run."""
    t = tile(hip_lib)
    parities = {ds.row_ceiling(D, T, t) % 2 for D in range(2, 17) for T in ds.grid_taps(D)}
    assert parities == {0, 1}


# ----------------------------------------------------------------------------------------------- 2. the accumulator
def clamp_shift(acc: int, s: int) -> int:
    return min(max((acc + ((1 << (s - 1)) if s else 0)) >> s, -32768), 32767)


@pytest.mark.parametrize("D", ds.WORST_D)
@pytest.mark.parametrize("which", range(8))
def test_the_accumulator_at_its_limit(hip_lib, ctx, D, which):
    """Output n0's window holds the rail of its tap's sign (times the polarity) at every tap: the largest accumulator
    these taps allow, |acc| up to 65534 * 32768 = 2^31 - 2^16, in lanes 0 and tile - 1 of the first tile, lane 0 of the
    second and the ragged third; in one call, with the window half in the history buffer, and with the output in a
    call shorter than the history."""
    t = tile(hip_lib)
    name, h, shifts = ds.worst_case_sets()[which]
    T = len(h)
    outputs, n = ds.worst_case_outputs(D, t)
    assert outputs == (0, t - 1, t, 2 * t + 20)
    from_history = short_calls = 0
    for s in shifts:
        with ctx.decimator(D, h, s) as dec:
            for pol in (1, -1):
                for n0 in outputs:
                    x = ds.worst_case_iq(h, D, n0, n, pol)
                    want = ds.decimate(x, h, D, s)
                    v = clamp_shift(ds.worst_case_acc(h, D, n0, pol), s)
                    assert want[n0].tolist() == [v, v]
                    what = (name, D, s, pol, n0)
                    assert np.array_equal(run_split(dec, x, []), want), what
                    cut = n0 * D - T // 2
                    if cut > 0 and T > 1:
                        assert np.array_equal(run_split(dec, x, [cut]), want), what
                        from_history += 1
                    # ... and output n0 from a call of T - 2 inputs: all but one of its taps read the history
                    end = n0 * D + 2
                    if T >= 3 and end - (T - 2) > 0:
                        assert np.array_equal(run_split(dec, x, [end - (T - 2), end]), want), what
                        short_calls += 1
    assert from_history >= (2 * len(shifts) * 3 if T > 1 else 0)
    assert short_calls >= (2 * len(shifts) * 2 if T >= 3 else 0)   # (T = 512 at D = 2 starts behind output tile - 1)


@pytest.mark.parametrize("D", ds.WORST_D)
def test_the_accumulator_at_its_limit_through_bytes(hip_lib, ctx, D):
    """T_soapy stops short of the rails, so a table with T8[0] = -32768 and T8[255] = 32767 takes the bytes there."""
    import torch
    t = tile(hip_lib)
    table = ds.rail_u8_table()
    outputs, n = ds.worst_case_outputs(D, t)
    sets = [x for x in ds.worst_case_sets() if x[0] in ("positive", "negative", "random 512")]
    assert len(sets) == 3
    ctx.set_u8_table(table)
    try:
        assert np.array_equal(ctx.u8_table(), table)
        for name, h, shifts in sets:
            T = len(h)
            for s in shifts:
                with ctx.decimator(D, h, s) as dec:
                    for pol in (1, -1):
                        for n0 in outputs:
                            b = ds.worst_case_iq(h, D, n0, n, pol, lo=0, hi=255, dtype=np.uint8)
                            want = ds.decimate(widen(b, table), h, D, s)
                            v = clamp_shift(ds.worst_case_acc(h, D, n0, pol), s)
                            assert want[n0].tolist() == [v, v]
                            assert np.array_equal(run_split(dec, b, [], U8), want), (name, D, s, pol, n0)
                            cut = n0 * D - T // 2
                            if cut > 0:
                                assert np.array_equal(run_split(dec, b, [cut], U8), want), (name, D, s, pol, n0)
    finally:
        torch.cuda.synchronize()
        ctx.set_u8_table(None)


# ----------------------------------------------------------------------------------------------- 3. alignment, arguments
JUNK = 0xA5


def run_at(dec, x: np.ndarray, fmt: int, in_off: int, out_off: int) -> np.ndarray:
    """run() with the input at `in_off` bytes and the outputs at `out_off` bytes into larger allocations: junk around the
    input, a guard in front of and behind the outputs."""
    import torch
    want_n = dec.out_count(len(x))
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    lead = out_off // 2
    with torch.cuda.stream(dec._ctx.torch_stream):
        d_in = torch.full((len(raw) + 256,), JUNK, dtype=torch.uint8, device="cuda")
        d_in[in_off:in_off + len(raw)] = torch.from_numpy(raw).cuda()
        d_out = torch.full((lead + 2 * (want_n + 8),), 0x5A5A, dtype=torch.int16, device="cuda")
        assert d_in.data_ptr() % 64 == 0 and d_out.data_ptr() % 64 == 0
        n = dec.run_device(d_in.data_ptr() + in_off, len(x), d_out.data_ptr() + out_off, want_n, format=fmt)
        assert n == want_n
        y = d_out.cpu().numpy()
    assert (y[:lead] == 0x5A5A).all() and (y[lead + 2 * n:] == 0x5A5A).all()   # nothing around the call's outputs
    return y[lead:lead + 2 * n].reshape(-1, 2)


@pytest.mark.parametrize("fmt", [CS16, U8])
@pytest.mark.parametrize("D", [2, 16])
def test_pointers_at_odd_multiples_of_16_bytes(hip_lib, ctx, D, fmt):
    """The ABI asks for 16 bytes, torch hands out hundreds: here the input sits at 16 and 48 bytes past such a boundary
    and the outputs at 16.  Two tiles and one output, from reset (the first tile's origin in front of the call, the
    others' behind its start) and behind a first call of 3 D + 1 inputs (an odd phase)."""
    t = tile(hip_lib)
    rng = np.random.default_rng(7000 + 2 * D + fmt)
    T, s = 8 * D + 1, 15
    h = ds.random_taps(rng, T)
    n_in = n_in_for(2 * t + 1, D)
    if fmt == U8:
        x = rng.integers(0, 256, size=(n_in, 2), dtype=np.uint8)
        want = ds.decimate(widen(x, t_soapy()), h, D, s)
    else:
        x = ds.random_iq(rng, n_in, run=T)
        want = ds.decimate(x, h, D, s)
    first = 3 * D + 1
    with ctx.decimator(D, h, s) as dec:
        for in_off, out_off in [(16, 16), (48, 16), (48, 0), (0, 16)]:
            dec.reset()
            assert np.array_equal(run_at(dec, x, fmt, in_off, out_off), want), (in_off, out_off)
            dec.reset()
            parts = [run_at(dec, x[:first], fmt, in_off, out_off), run_at(dec, x[first:], fmt, in_off, out_off)]
            assert [len(p) for p in parts] == [4, 2 * t + 1 - 4]
            assert np.array_equal(np.concatenate(parts), want), (in_off, out_off)


@pytest.mark.parametrize("fmt", [CS16, U8])
def test_misaligned_pointers_are_refused_and_consume_nothing(hip_lib, ctx, fmt):
    import torch
    from dump1090_rs_amd import _lib
    t = tile(hip_lib)
    rng = np.random.default_rng(7100 + fmt)
    D, T, s = 3, 25, 15
    h = ds.random_taps(rng, T)
    if fmt == U8:
        x = rng.integers(0, 256, size=((t + 5) * D + 1, 2), dtype=np.uint8)
        want = ds.decimate(widen(x, t_soapy()), h, D, s)
    else:
        x = ds.random_iq(rng, (t + 5) * D + 1, run=T)
        want = ds.decimate(x, h, D, s)
    with ctx.decimator(D, h, s) as dec:
        head = run(dec, x[:100], fmt)
        rest = np.ascontiguousarray(x[100:])
        probes = [dec.out_count(k) for k in range(1, 2 * D + 1)]
        cap = dec.out_count(len(rest))
        with torch.cuda.stream(ctx.torch_stream):
            d_in = torch.zeros(rest.nbytes + 64, dtype=torch.uint8, device="cuda")
            d_out = torch.full((cap + 16, 2), 0x5A5A, dtype=torch.int16, device="cuda")
            for off in (2, 4, 8):
                for in_off, out_off in ((off, 0), (0, off), (off, off)):
                    n = C.c_size_t()
                    st = dec._L.adsb_decim_run_device(dec._h, fmt, C.c_void_p(d_in.data_ptr() + in_off), len(rest),
                                                      C.c_void_p(d_out.data_ptr() + out_off), cap, C.byref(n))
                    assert st == _lib.ADSB_ERR_INVALID, (off, in_off, out_off)
                    assert [dec.out_count(k) for k in range(1, 2 * D + 1)] == probes and dec.out_count(len(rest)) == cap
            assert (d_out.cpu().numpy() == 0x5A5A).all()
        assert np.array_equal(np.concatenate([head, run(dec, rest, fmt)]), want)   # the stream goes on where it was


def test_create_refuses_what_the_header_excludes(hip_lib, ctx):
    from dump1090_rs_amd import _lib

    def create(factor, taps, shift, n_taps=None):
        a = np.ascontiguousarray(taps, dtype=np.int16)
        handle = C.c_void_p(0x1234)
        st = hip_lib.adsb_decim_create(ctx._h, factor, a.ctypes.data, len(a) if n_taps is None else n_taps, shift, C.byref(handle))
        if st == _lib.ADSB_OK:
            assert handle.value not in (None, 0x1234)
            hip_lib.adsb_decim_destroy(handle)
        else:
            assert handle.value is None
        return st

    ok = [1, -1]
    for factor in (1, 17, 0):
        assert create(factor, ok, 0) == _lib.ADSB_ERR_INVALID
    assert create(2, ok, 0, n_taps=0) == _lib.ADSB_ERR_INVALID
    assert create(2, np.ones(513, np.int16), 0) == _lib.ADSB_ERR_INVALID
    assert create(2, ok, 17) == _lib.ADSB_ERR_INVALID
    for taps in ([32767, 32767, 1], [-32768, 32767], [-32768, -32767], [128] * 511 + [127]):
        assert np.abs(np.asarray(taps, dtype=np.int64)).sum() == 65535
        assert create(2, taps, 15) == _lib.ADSB_ERR_INVALID, taps
    # the limits themselves are taken
    assert create(2, [-32768, 32766], 15) == _lib.ADSB_OK
    assert create(16, np.r_[np.full(511, 128), 126], 16) == _lib.ADSB_OK
    assert create(2, [-32768], 0) == _lib.ADSB_OK
    # ... and the tap -32768 computes (test_the_accumulator_at_its_limit runs it at the rails)
    x = np.array([[-32768, 32767], [5, -7], [1, -1], [0, 3]], np.int16)
    with ctx.decimator(2, [-32768, 32766], 15) as dec:
        assert np.array_equal(run(dec, x), ds.decimate(x, [-32768, 32766], 2, 15))


# ----------------------------------------------------------------------------------------------- 4. past the resource cap
def test_one_call_longer_than_a_tiles_buffer_resource(hip_lib, ctx):
    """k_decim gives a tile a buffer resource of the bytes left behind its origin, 2^30 at most.  2^28 + 3 tile D + 5
    CS16 samples leave more than that behind the first tiles: outputs are checked in the first two tiles, the two on
    either side of the tile where the bytes left fall below 2^30, and the last two, the ragged one included.  1.1 GiB
    of device memory; only the windows come back."""
    import torch
    t = tile(hip_lib)
    D, T, s = 16, 17, 15
    h = ds.random_taps(np.random.default_rng(8000), T)
    n_in = 2 ** 28 + 3 * t * D + 5
    n_out = -(-n_in // D)
    blocks = -(-n_out // t)

    def left(blk):
        return (n_in - ds.tile_base(blk, 0, D, T, t)) * 4

    switch = next(b for b in range(blocks) if left(b) < 2 ** 30)
    assert left(0) > 2 ** 30 and left(switch - 1) >= 2 ** 30 and 2 <= switch <= blocks - 4 and n_out % t
    windows = [(0, 2 * t), ((switch - 2) * t, 4 * t), ((blocks - 2) * t, n_out - (blocks - 2) * t)]
    with ctx.decimator(D, h, s) as dec:
        assert dec.out_count(n_in) == n_out
        with torch.cuda.stream(ctx.torch_stream):
            d_in = torch.randint(-32768, 32768, (n_in, 2), dtype=torch.int16, device="cuda")
            d_out = torch.full((n_out + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
            assert dec.run_device(d_in.data_ptr(), n_in, d_out.data_ptr(), n_out) == n_out
            for first, count in windows:
                lo, hi = ds.window_inputs(first, count, T, D)
                xw = d_in[lo:hi].cpu().numpy()
                assert xw.min() < -30000 and xw.max() > 30000
                got = d_out[first:first + count].cpu().numpy()
                assert np.array_equal(got, ds.decimate_window(xw, first, count, h, D, s)), (first, count)
            assert (d_out[n_out:].cpu().numpy() == 0x5A5A).all()
            del d_in, d_out
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------- 5. the context's modes
EDGE = CHUNK + 50_001        # outputs of the first of two calls: its input ends one sample behind a multiple of D
N_BASE = 2 * CHUNK + 70_001  # two buffers and a ragged third


def boxcar(D: int) -> np.ndarray:
    return np.full(D, 65534 // D, np.int16)


@pytest.fixture(scope="module")
def capture():
    """(base, planted): a synthetic capture at 2.4 MS/s and three DF17s planted across output sample CHUNK (a buffer
    edge of the first call), EDGE (the edge between the calls) and EDGE + CHUNK (a buffer edge of the second call).
    The tests repeat every sample D times and decimate by a boxcar."""
    edges = (CHUNK, EDGE, EDGE + CHUNK)
    planted = [synth.df17_frame(0xABC000 + k, 0x11223344556600 + k) for k in range(3)]
    # (the random bursts keep clear of the planted ones)
    bursts = [b for b in synth.plan_bursts(N_BASE, 300, 4242, n_icao=20, df11_every=3)
              if all(abs(b.tick // 5 - at) > 800 for at in edges)]
    assert len(bursts) > 290
    base = synth.noise_numpy(N_BASE, 4242)
    synth.add_bursts(base, bursts + [synth.Burst(5 * (at - 100) + k, 20000, 3 + 2 * k, planted[k]) for k, at in enumerate(edges)])
    return base, planted


def calls_of(x: np.ndarray, D: int):
    """x cut into a call that ends at an input index that is no multiple of D, one of a single input that reaches no
    output, and the rest."""
    cut = (EDGE - 1) * D + 1
    assert cut % D == 1
    return [x[:cut], x[cut:cut + 1], x[cut + 1:]]


def pieces_of(y: np.ndarray):
    return [y[:EDGE], y[EDGE:EDGE], y[EDGE:]]


def buffers(msgs):
    return [bytes(w["buffer"]) for w in msgs]


@pytest.mark.parametrize("D, max_chunks", [(2, 1), (2, 2), (5, 1), (5, 2)])
def test_carry_over_through_the_decimator(hip_lib, oracle_mod, capture, D, max_chunks):
    """A context of one buffer takes every output buffer as a piece of its own, one of two takes them in pairs: the DF17
    across output sample CHUNK straddles a piece edge or lies inside a piece, the one across EDGE straddles two calls
    with a call of no output between them."""
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    base, planted = capture
    h, s = boxcar(D), 16
    x = np.repeat(base, D, axis=0)
    y = ds.decimate(x, h, D, s)
    assert len(y) == N_BASE
    calls, pieces = calls_of(x, D), pieces_of(y)
    ref = ds.Stream(h, D, s)
    assert [len(ref.run(part)) for part in calls] == [EDGE, 0, N_BASE - EDGE] and len(calls[1]) == 1 < D
    orc, carry = oracle_mod.Oracle(), np.zeros((326, 2), np.int16)
    with_carry = [demod_iq_carry(orc, p, carry, cap=1 << 16)[0] if len(p) else [] for p in pieces]
    orc = oracle_mod.Oracle()
    plain = [orc.demod_iq(p, cap=1 << 16)[0] if len(p) else [] for p in pieces]
    # the planted frames are found at every edge with carry-over and at none without
    found = [b for w in with_carry for b in buffers(w)]
    assert all(found.count(fr) == 1 for fr in planted)
    assert not any(fr in buffers(w) for w in plain for fr in planted)
    assert planted[0] in buffers(with_carry[0]) and planted[1] in buffers(with_carry[2]) and planted[2] in buffers(with_carry[2])
    with Context(0, max_chunks) as c, c.decimator(D, h, s) as dec:
        c.icao_flush()
        for part, want in zip(calls, plain):
            assert_same(dec.demod_iq(part, cap=1 << 16), want)
        c.set_carry_over(True)   # (restarts the context's stream)
        c.icao_flush()
        dec.reset()
        for part, want in zip(calls, with_carry):
            assert_same(dec.demod_iq(part, cap=1 << 16), want)
        c.set_carry_over(False)
        c.icao_flush()
        dec.reset()
        for part, want in zip(calls, plain):
            assert_same(dec.demod_iq(part, cap=1 << 16), want)


def stats_dtype():
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
    return SIGNAL_STATS_DTYPE


def assert_records(got, want, what=""):
    assert got.dtype == want.dtype and len(got) == len(want), what
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), (what, name, got[name], want[name])


@pytest.mark.parametrize("D, max_chunks", [(2, 1), (2, 2), (5, 1), (5, 2)])
def test_signal_statistics_through_the_decimator(hip_lib, oracle_mod, capture, D, max_chunks):
    """One record per OUTPUT buffer, `chunk` counting over the call across its pieces.  The boxcar at shift 15 doubles
    the samples, so the strong bursts clamp to the rails and n_clipped counts them."""
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    base, _ = capture
    h, s = boxcar(D), 15
    x = np.repeat(base, D, axis=0)
    y = ds.decimate(x, h, D, s)
    orc = oracle_mod.Oracle()
    whole = ss.restated(orc, y, y, stats_dtype())
    assert len(whole) == 3 and list(whole["chunk"]) == [0, 1, 2] and (whole["n_clipped"] > 0).all()
    assert whole["n_samples"][2] == 70_001
    want_msgs, _ = oracle_mod.Oracle().demod_iq(y, cap=1 << 16)
    with Context(0, max_chunks) as c, c.decimator(D, h, s) as dec:
        c.icao_flush()
        assert_same(dec.demod_iq(x, cap=1 << 16), want_msgs)
        assert len(c.signal_stats()) == 0   # the mode is off
        c.set_signal_stats(True)
        c.icao_flush()
        dec.reset()
        assert_same(dec.demod_iq(x, cap=1 << 16), want_msgs)
        assert_records(c.signal_stats(), whole, "one call")
        # together with carry-over, in calls: carried samples are not counted, a call without output has no record
        c.set_carry_over(True)
        c.icao_flush()
        dec.reset()
        orc, carry = oracle_mod.Oracle(), np.zeros((326, 2), np.int16)
        for k, (part, piece) in enumerate(zip(calls_of(x, D), pieces_of(y))):
            want = demod_iq_carry(orc, piece, carry, cap=1 << 16)[0] if len(piece) else []
            assert_same(dec.demod_iq(part, cap=1 << 16), want)
            assert_records(c.signal_stats(), ss.restated(orc, piece, piece, stats_dtype()), k)
            assert len(c.signal_stats()) == (2, 0, 2)[k]


@pytest.mark.parametrize("D, max_chunks", [(2, 1), (5, 2)])
def test_error_correction_through_the_decimator(hip_lib, oracle_mod, D, max_chunks):
    from dump1090_rs_amd import Context, _lib
    h, s = boxcar(D), 16
    one, _, _ = fs.damaged_capture()
    iq1 = np.concatenate([one, one])   # two buffers: the second piece starts with the first's filter
    iq2, _ = f2.pair_stream(pairs=f2.PAIRS[::100])
    assert len(iq1) == len(iq2) == 2 * CHUNK
    with Context(0, max_chunks) as c, c.decimator(D, h, s) as dec:
        for mode, iq, restated, scores in ((_lib.ADSB_FIX_1BIT, iq1, fs.Restated, {1200}),
                                           (_lib.ADSB_FIX_2BIT, iq2, f2.Restated, {1100, 1200})):
            x = np.repeat(iq, D, axis=0)
            want = restated(mode).demod_iq(ds.decimate(x, h, D, s))
            assert scores <= {k[1] for k in want} and {k[4] for k in want} == {0, 1}
            c.set_error_correction(mode)
            c.icao_flush()
            dec.reset()
            assert [fs.key(m) for m in dec.demod_iq(x, cap=1 << 16)] == want, mode


def raw_keys(buf, n):
    return [(int(m.chunk), int(m.j), int(m.try_phase), int(m.score), int(m.len), bytes(m.msg).hex(), float(m.signal_level))
            for m in buf[:n]]


def want_keys(want):
    return [(w["chunk"], w["j"], w["try_phase"], w["score"], w["len"], w["msg"].hex(), w["signal_level"]) for w in want]


@pytest.mark.parametrize("D", [2, 5])
def test_capacity_and_busy_are_the_contexts(hip_lib, oracle_mod, capture, D):
    import torch
    from dump1090_rs_amd import Context, _lib
    from dump1090_rs_amd._lib import AdsbMsg
    base, _ = capture
    h, s = boxcar(D), 16
    x = np.repeat(base, D, axis=0)
    cuts = [0, CHUNK * D + 12_345, (CHUNK + 30_000) * D + 1, (2 * CHUNK + 1000) * D + 3, len(x)]
    parts = [np.ascontiguousarray(x[a:z]) for a, z in zip(cuts, cuts[1:])]
    ref, orc = ds.Stream(h, D, s), oracle_mod.Oracle()
    with Context(0, 1) as c, c.decimator(D, h, s) as dec:
        L = c._L
        c.icao_flush()
        # 1. the list does not fit: the full count, the list through adsb_fetch_messages, the stream advanced once
        want, _ = orc.demod_iq(ref.run(parts[0]), cap=1 << 16)
        assert len(want) > 4
        out, n = (AdsbMsg * 4)(), C.c_size_t()
        st = L.adsb_decim_demod_iq(dec._h, CS16, parts[0].ctypes.data, len(parts[0]), out, 4, C.byref(n))
        assert st == _lib.ADSB_ERR_CAPACITY and n.value == len(want)
        assert raw_keys(out, 4) == want_keys(want)[:4]
        full, m = (AdsbMsg * n.value)(), C.c_size_t()
        assert L.adsb_fetch_messages(c._h, full, n.value, C.byref(m)) == _lib.ADSB_OK and m.value == n.value
        assert raw_keys(full, m.value) == want_keys(want)
        assert dec.out_count(len(parts[1])) == ref.out_count(len(parts[1]))
        want, _ = orc.demod_iq(ref.run(parts[1]), cap=1 << 16)
        assert_same(dec.demod_iq(parts[1], cap=1 << 16), want)
        # 2. a pass submitted and not collected: adsb_decim_demod_iq is BUSY and consumes nothing, run_device is not
        y2 = ref.run(parts[2])
        d_in = torch.from_numpy(parts[2]).cuda()
        d_y = torch.full((len(y2) + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        d_other = torch.from_numpy(np.ascontiguousarray(base[:CHUNK])).cuda()
        torch.cuda.synchronize()
        c.submit_iq_device(d_other.data_ptr(), CHUNK)
        want_other, _ = orc.demod_iq(base[:CHUNK], cap=1 << 16)
        probes = [dec.out_count(k) for k in range(1, 2 * D + 1)]
        n = C.c_size_t()
        out = (AdsbMsg * 4096)()
        st = L.adsb_decim_demod_iq(dec._h, CS16, parts[2].ctypes.data, len(parts[2]), out, 4096, C.byref(n))
        assert st == _lib.ADSB_ERR_BUSY
        assert [dec.out_count(k) for k in range(1, 2 * D + 1)] == probes and c.pending() == 1
        assert dec.run_device(d_in.data_ptr(), len(parts[2]), d_y.data_ptr(), len(y2)) == len(y2)
        assert c.pending() == 1
        assert_same(c.collect(), want_other)
        torch.cuda.synchronize()
        got = d_y.cpu().numpy()
        assert np.array_equal(got[:len(y2)], y2) and (got[len(y2):] == 0x5A5A).all()
        # 3. and the stream goes on behind it
        want, _ = orc.demod_iq(ref.run(parts[3]), cap=1 << 16)
        assert len(want) > 0
        assert_same(dec.demod_iq(parts[3], cap=1 << 16), want)


@pytest.mark.parametrize("D", [2, 5])
def test_the_asynchronous_form_under_carry_over_and_statistics(hip_lib, oracle_mod, capture, D):
    """adsb_decim_run_device + adsb_submit_iq_device with nothing in between, twice, both passes in flight: the
    messages and records of the blocking form, which are the oracle's."""
    import torch
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    base, planted = capture
    h, s = boxcar(D), 15
    x = np.repeat(base, D, axis=0)
    y = ds.decimate(x, h, D, s)
    cut = (EDGE - 1) * D + 1
    calls, pieces = [np.ascontiguousarray(x[:cut]), np.ascontiguousarray(x[cut:])], [y[:EDGE], y[EDGE:]]
    orc, carry = oracle_mod.Oracle(), np.zeros((326, 2), np.int16)
    wants = [demod_iq_carry(orc, p, carry, cap=1 << 16)[0] for p in pieces]
    recs = [ss.restated(orc, p, p, stats_dtype()) for p in pieces]
    assert [len(r) for r in recs] == [2, 2] and sum(len(w) for w in wants) > 50
    with Context(0, 2) as c, c.decimator(D, h, s) as dec:
        c.set_carry_over(True)
        c.set_signal_stats(True)
        c.icao_flush()
        blocking = []
        for part, want, rec in zip(calls, wants, recs):
            got = dec.demod_iq(part, cap=1 << 16)
            assert_same(got, want)
            assert_records(c.signal_stats(), rec)
            blocking.append([key(m) for m in got])
        d_in = [torch.from_numpy(p).cuda() for p in calls]
        d_y = [torch.empty((len(p), 2), dtype=torch.int16, device="cuda") for p in pieces]
        torch.cuda.synchronize()
        c.set_carry_over(True)   # (restarts the context's stream)
        c.icao_flush()
        dec.reset()
        for k in range(2):
            n = dec.run_device(d_in[k].data_ptr(), len(calls[k]), d_y[k].data_ptr(), len(pieces[k]))
            assert n == len(pieces[k])
            c.submit_iq_device(d_y[k].data_ptr(), n)
        assert c.pending() == 2
        for k in range(2):
            got = c.collect()
            assert [key(m) for m in got] == blocking[k]
            assert_same(got, wants[k])
            assert_records(c.signal_stats(), recs[k], k)
        torch.cuda.synchronize()
        for k in range(2):
            assert np.array_equal(d_y[k].cpu().numpy(), pieces[k])

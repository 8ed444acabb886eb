"""Resampler banks on the device (include/adsb_hip.h, "Resampler banks"): every stream of a bank held bit for bit and
count for count to the numpy restatement of ONE resampler fed that stream's calls (tests/resamp_support.py, with
tests/mix_support.py and tests/formats_in_support.py for the mixer and the conversion), and, where stated, to real
Resampler handles in the same context -- never to the bank itself.  Tolerance 0 everywhere.

Every test uploads its inputs and reserves its outputs first, makes its calls back to back with nothing between them, and
reads back afterwards: the calls' order on the stream is all that holds them together."""
import numpy as np
import pytest

from tests import formats_in_support as fi
from tests import mix_support as ms
from tests import resamp_support as rs

pytestmark = pytest.mark.gpu

CHUNK = 131072
CS16, U8, CF32, REAL16 = fi.CS16, fi.U8, fi.CF32, fi.REAL16
CANARY = 0x5A5A
TAIL = 8   # canary samples behind every output


def t_soapy() -> np.ndarray:
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


@pytest.fixture()
def ctx(hip_lib):
    """A context whose input is ordered behind a torch stream (adsb_set_stream): uploads, bank calls and read-backs run in
    that stream's order, with no other synchronisation."""
    import torch
    from dump1090_rs_amd import Context
    with Context(0, 3) as c:
        c.torch_stream = torch.cuda.Stream()
        c.set_stream(c.torch_stream.cuda_stream)
        yield c
        torch.cuda.synchronize()


def tile(hip_lib, L: int, M: int) -> int:
    t = int(hip_lib.adsb_resamp_selftest_tile(L, M))
    assert t >= L and t % L == 0
    return t


def taps_of(which: str, L: int, M: int, rng):
    T, s = {"small": (L + 1, 1), "default": (8 * max(L, M) + 1, 14), "maximal": (rs.max_taps(L), 16)}[which]
    return rs.random_phase_taps(rng, T, L), s


def play(ctx, bank, calls, want, fmts=None, before=None, caps=None):
    """calls[i] = [(stream, input array), ...] and want[i] = [expected output (n, 2) int16, ...]: uploads every input,
    reserves every output (canary-filled, TAIL samples more than expected), makes the calls back to back -- before[i](), if
    any, on the host in front of call i -- and only then reads back.  Asserts the counts and the canaries; returns the
    outputs as got[i][r]."""
    import torch
    fmts = fmts or [CS16] * len(calls)
    with torch.cuda.stream(ctx.torch_stream):
        d_in = [[torch.from_numpy(np.ascontiguousarray(x)).cuda() if len(x) else None for _, x in call] for call in calls]
        d_out = [[torch.full((len(w) + TAIL, 2), CANARY, dtype=torch.int16, device="cuda") for w in ws] for ws in want]
        counts = []
        for i, call in enumerate(calls):
            if before and before.get(i):
                before[i]()
            n = bank.run_device([s for s, _ in call], [t.data_ptr() if t is not None else 0 for t in d_in[i]],
                                [len(x) for _, x in call], [t.data_ptr() for t in d_out[i]],
                                [len(w) for w in want[i]] if caps is None else caps[i], format=fmts[i])
            counts.append(n.tolist())
        got = [[t.cpu().numpy() for t in outs] for outs in d_out]
    for i, ws in enumerate(want):
        assert counts[i] == [len(w) for w in ws], (i, counts[i])
        for r, w in enumerate(ws):
            assert (got[i][r][len(w):] == CANARY).all(), (i, r)   # nothing written behind the run's outputs
            got[i][r] = got[i][r][: len(w)]
    return got


def assert_equal(got, want):
    for i, ws in enumerate(want):
        for r, w in enumerate(ws):
            assert np.array_equal(got[i][r], w), (i, r)


# ----------------------------------------------------------------------------------------------- 1. ragged streams
@pytest.mark.parametrize("L, M", [(1, 5), (6, 5), (3, 25), (33, 17)])
@pytest.mark.parametrize("which", ["small", "default", "maximal"])
def test_ragged_streams(hip_lib, ctx, L, M, which):
    """Five streams, five calls in a row: per-call output counts from {0, 1, t - 1, t, t + 1, 2 t + 3}, a run shorter than
    K - 1, a run of no input, a stream left out of a call.  Every stream equals its rs.Stream, every n_out its out_count,
    consumed the sum of the stream's inputs -- and inputs_for / out_count of the bank the restatement's at every P met."""
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(9000 + 1000 * L + 7 * M + len(which))
    h, s = taps_of(which, L, M, rng)
    K = rs.phase_taps(L, len(h))
    N, n_calls = 5, 5
    choices = [0, 1, t - 1, t, t + 1, 2 * t + 3]
    refs = [rs.Stream(h, L, M, s) for _ in range(N)]
    P = [0] * N
    # what each call asks of each stream: ("out", count), ("in", inputs) or None (left out)
    asks = [[("out", choices[(N * i + k) % 6]) for k in range(N)] for i in range(n_calls)]   # every count four times
    asks[0][4] = ("out", 2 * t + 3)
    asks[1][0] = ("in", max(K - 2, 0))   # shorter than the history (small taps: no input at all)
    asks[2][1] = ("in", 0)               # a run of no input
    asks[3][2] = None                    # a stream left out
    asks[1][3] = ("in", 1)
    asks[4][0] = ("out", t + 1)          # ... and the short run's stream goes on
    seen = set()
    calls, want, planned = [], [], []
    for i in range(n_calls):
        call, ws = [], []
        order = [int(k) for k in rng.permutation(N)]   # the runs name the streams in any order
        for k in order:
            if asks[i][k] is None:
                continue
            kind, v = asks[i][k]
            n_in = rs.inputs_for(L, M, P[k], v) if kind == "out" else v
            n_out = rs.out_count(L, M, P[k], n_in)
            if kind == "out":
                assert v <= n_out <= v + (L > M)
                seen.add(v)
            planned.append((i, k, P[k], v if kind == "out" else None, n_in, n_out))
            x = rs.random_iq(rng, n_in, run=min(K, n_in // 3))
            y = refs[k].run(x)
            assert len(y) == n_out
            P[k] += n_in
            call.append((k, x))
            ws.append(y)
        calls.append(call)
        want.append(ws)
    assert seen == set(choices)
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        assert bank.streams == N
        # the host arithmetic, per stream, in front of each call (the calls themselves are made back to back below: these
        # queries wait for nothing)
        done = {"i": 0}

        def check_counts(i):
            def f():
                for (ci, k, Pk, v, n_in, n_out) in planned:
                    if ci != i:
                        continue
                    assert bank.consumed(k) == Pk
                    assert bank.out_count(k, n_in) == n_out
                    if v is not None:
                        assert bank.inputs_for(k, v) == ((n_in, n_out) if v else (0, 0)), (k, Pk, v)
                done["i"] += 1
            return f

        got = play(ctx, bank, calls, want, before={i: check_counts(i) for i in range(n_calls)})
        assert done["i"] == n_calls
        assert_equal(got, want)
        assert [bank.consumed(k) for k in range(N)] == P == [r.P for r in refs]


# ----------------------------------------------------------------------------------------------- 2. a bank of one
@pytest.mark.parametrize("L, M", [(24, 25), (1, 16)])
def test_a_bank_of_one_is_a_resampler(hip_lib, ctx, L, M):
    import torch
    from dump1090_rs_amd import default_resampler_taps
    t = tile(hip_lib, L, M)
    h, s = default_resampler_taps(L, M)
    K = rs.phase_taps(L, len(h))
    rng = np.random.default_rng(9100 + L)
    x = rs.random_iq(rng, rs.inputs_for(L, M, 0, 2 * t + 5) + 11, run=K)
    cuts = [0, 1, K - 2, K + M, rs.inputs_for(L, M, 0, t) + 3, len(x) - 1, len(x)]
    pieces = [x[a:b] for a, b in zip(cuts, cuts[1:])]
    ref = rs.Stream(h, L, M, s)
    want = [[ref.run(p)] for p in pieces]
    with ctx.resampler_bank(1, L, M, h, s) as bank, ctx.resampler(L, M, h, s) as res:
        got = play(ctx, bank, [[(0, p)] for p in pieces], want)
        with torch.cuda.stream(ctx.torch_stream):
            d_in = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pieces]
            d_out = [torch.full((len(w[0]) + TAIL, 2), CANARY, dtype=torch.int16, device="cuda") for w in want]
            ns = [res.run_device(a.data_ptr(), len(p), o.data_ptr(), len(w[0])) for a, p, o, w in zip(d_in, pieces, d_out, want)]
            single = [o.cpu().numpy() for o in d_out]
        assert ns == [len(w[0]) for w in want]
        for i, w in enumerate(want):
            assert got[i][0].tobytes() == single[i][: ns[i]].tobytes()   # the handle's bytes ...
            assert np.array_equal(got[i][0], w[0])                       # ... which are the restatement's
        assert bank.consumed(0) == len(x)


# ----------------------------------------------------------------------------------------------- 3. formats and mixer
def in_format(rng, fmt: int, n: int, g: float):
    """n samples of random input in `fmt` (CF32: with the edge values of q among them)."""
    if fmt == CS16:
        return rs.random_iq(rng, n, run=3)
    if fmt == U8:
        return rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    if fmt == REAL16:
        return rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
    x = (rng.standard_normal((n, 2)) * (20000.0 / g)).astype(np.float32)
    e = fi.edge_values()
    k = min(len(e), x.size)
    x.reshape(-1)[rng.permutation(x.size)[:k]] = e[:k]
    return x


@pytest.mark.parametrize("L, M", [(3, 25), (6, 5)])
def test_formats_and_mixer(hip_lib, ctx, L, M):
    """All four formats alternate from call to call on three streams whose P -- hence whose mixer phase -- differ; the
    mixer (N = 7) is set, changed and cleared between calls; CF32 at a scale that is no power of two, with NaN, the
    infinities and the ties; an odd REAL16 length.  Output = conversion, then mixer, then filter, per stream."""
    import torch
    from dump1090_rs_amd import default_resampler_taps
    t = tile(hip_lib, L, M)
    h, s = default_resampler_taps(L, M)
    rng = np.random.default_rng(9200 + L)
    w1, w2 = ms.random_table(rng, 7), ms.random_table(rng, 7)
    assert not np.array_equal(w1, w2)
    table = t_soapy()
    N = 3
    refs = [ms.ResampStream(h, L, M, s) for _ in range(N)]
    base = rs.inputs_for(L, M, 0, t + 3)
    # (format, mixer in front of the call -- "keep": unchanged --, scale in front of the call, the three lengths)
    script = [(CS16, "keep", None, [base, 5, base // 2 + 1]),
              (CF32, w1, fi.G2, [base + 3, base // 3, 7]),
              (REAL16, "keep", None, [2 * M + 1, base | 1, 1]),
              (U8, w2, None, [base // 2, 9, base + 1]),
              (CF32, None, fi.DEFAULT_SCALE, [11, base, 0]),
              (CS16, w1, None, [base, base + 2, 3])]
    assert any(n % 2 for n in script[2][3])
    calls, want, fmts, before = [], [], [], {}
    g, phases = fi.DEFAULT_SCALE, []
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        assert bank.mixer_period == 0 and bank.scale == fi.DEFAULT_SCALE
        for i, (fmt, w, scale, lens) in enumerate(script):
            if scale is not None:
                g = scale

            def setter(w=w, scale=scale):
                if scale is not None:
                    bank.set_scale(scale)
                if not isinstance(w, str):
                    bank.set_mixer(w)
            before[i] = setter
            if not isinstance(w, str):
                for r in refs:
                    r.set_mixer(w)
            if refs[0].w is not None:
                phases.append(tuple(r.P % len(r.w) for r in refs))
            call, ws = [], []
            for k, n in enumerate(lens):
                x = in_format(rng, fmt, n, g)
                ws.append(refs[k].run(fi.to_cs16(x, fmt, g, table)))
                call.append((k, x))
            calls.append(call)
            want.append(ws)
            fmts.append(fmt)
        assert any(len(set(p)) == N for p in phases)   # the streams stood at three different table entries
        ctx.set_u8_table(table)   # (nothing is running yet)
        try:
            got = play(ctx, bank, calls, want, fmts=fmts, before=before)
        finally:
            torch.cuda.synchronize()
            ctx.set_u8_table(None)
        assert_equal(got, want)
        assert bank.mixer_period == 7 and bank.scale == fi.DEFAULT_SCALE
        assert [bank.consumed(k) for k in range(N)] == [r.P for r in refs]


# ----------------------------------------------------------------------------------------------- 4. width
IN_SLOT, OUT_SLOT = 304, 64   # samples per stream: 16-byte multiples that hold 300 inputs and 60 outputs + canary


def wide_call(ctx, bank, order, x_all, n_in):
    """One call over the streams of `order`, stream k's inputs at slot k of x_all's device copy -> (counts, outputs)."""
    import torch
    N = len(n_in)
    with torch.cuda.stream(ctx.torch_stream):
        d_in = torch.from_numpy(x_all).cuda()
        d_out = torch.full((N * OUT_SLOT, 2), CANARY, dtype=torch.int16, device="cuda")
        order = np.asarray(order, dtype=np.int64)
        n = bank.run_device(order, d_in.data_ptr() + order * (IN_SLOT * 4), n_in[order], d_out.data_ptr() + order * (OUT_SLOT * 4),
                            np.full(len(order), OUT_SLOT - 4))
        y = d_out.cpu().numpy().reshape(N, OUT_SLOT, 2)
    counts = np.zeros(N, dtype=np.int64)
    counts[order] = n
    return counts, y


@pytest.mark.parametrize("N", [16384, 67])
def test_width(hip_lib, ctx, N):
    """Every stream of the widest bank there is, 37 .. 300 inputs by index, in one call; at N = 67 a second call names the
    streams in reverse order."""
    from dump1090_rs_amd import default_resampler_taps
    L, M = 1, 5
    h, s = default_resampler_taps(L, M)
    rng = np.random.default_rng(9300 + N)
    n_in = 37 + (np.arange(N) % 264 if N >= 264 else np.arange(N) * 263 // (N - 1))
    assert n_in.min() == 37 and n_in.max() == 300
    rounds = 1 if N > 67 else 2
    xs = [rng.integers(-32768, 32768, size=(N, IN_SLOT, 2), dtype=np.int64).astype(np.int16) for _ in range(rounds)]
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        orders = [np.arange(N), np.arange(N)[::-1]][:rounds]
        results = [wide_call(ctx, bank, o, x.reshape(-1, 2), n_in) for o, x in zip(orders, xs)]
        checked = sorted({0, N - 1, *rng.integers(0, N, size=64).tolist()})
        for k in range(N):
            P = 0
            for counts, y in results:
                c = rs.out_count(L, M, P, int(n_in[k]))
                assert counts[k] == c and (y[k, c:] == CANARY).all(), k
                P += int(n_in[k])
        for k in checked:
            ref = rs.Stream(h, L, M, s)
            for x, (counts, y) in zip(xs, results):
                assert np.array_equal(y[k, : counts[k]], ref.run(x[k, : n_in[k]])), k
        assert bank.consumed(N - 1) == rounds * int(n_in[N - 1])


# ----------------------------------------------------------------------------------------------- 5. descriptor rotation
def test_descriptor_rotation(hip_lib, ctx):
    """Three times as many calls as there are descriptor blocks, back to back: a call that finds its block in flight
    waits for it, and no call reads another's descriptors."""
    L, M = 6, 5
    depth = int(hip_lib.adsb_bank_selftest_depth())
    assert depth >= 2
    t = tile(hip_lib, L, M)
    rng = np.random.default_rng(9400)
    h, s = taps_of("default", L, M, rng)
    N = 3
    refs = [rs.Stream(h, L, M, s) for _ in range(N)]
    calls, want = [], []
    for i in range(3 * depth):
        call, ws = [], []
        for k in [int(v) for v in rng.permutation(N)]:
            n = int(rng.choice([1, 7, 40 + i, t // 2 + 5 * i + k, rs.inputs_for(L, M, refs[k].P, t + 2 + i)]))
            x = rs.random_iq(rng, n, run=3)
            ws.append(refs[k].run(x))
            call.append((k, x))
        calls.append(call)
        want.append(ws)
    assert len({(len(x), len(w)) for call, ws in zip(calls, want) for (_, x), w in zip(call, ws)}) > 2 * depth
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        assert_equal(play(ctx, bank, calls, want), want)
        assert [bank.consumed(k) for k in range(N)] == [r.P for r in refs]


# ----------------------------------------------------------------------------------------------- 6. reset
def test_reset_of_one_stream_and_of_all(hip_lib, ctx):
    L, M = 3, 25
    rng = np.random.default_rng(9500)
    h, s = taps_of("default", L, M, rng)
    K = rs.phase_taps(L, len(h))
    N = 3
    refs = [rs.Stream(h, L, M, s) for _ in range(N)]
    lens = [[5 * M + 3, K + 40, 2 * M + 1], [K + 7, 3 * M + 2, K // 2], [K + 1, K + 2, K + 3]]
    calls, want = [], []
    for i, row in enumerate(lens):
        if i == 1:
            refs[1].reset()
        if i == 2:
            for r in refs:
                r.reset()
        call = [(k, rs.random_iq(rng, n, run=K // 2)) for k, n in enumerate(row)]
        calls.append(call)
        want.append([refs[k].run(x) for k, x in call])
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        got = play(ctx, bank, calls, want, before={1: lambda: bank.reset(1), 2: lambda: bank.reset()})
        assert_equal(got, want)
        # (a stream that was not reset would have answered with its history: the comparison can tell)
        stale = rs.Stream(h, L, M, s)
        stale.run(calls[0][1][1])
        assert not np.array_equal(stale.run(calls[1][1][1]), want[1][1])
        assert [bank.consumed(k) for k in range(N)] == lens[2]


# ----------------------------------------------------------------------------------------------- 7. errors
def test_errors_change_nothing(hip_lib, ctx):
    import torch
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd._lib import AdsbError
    L, M = 6, 5
    rng = np.random.default_rng(9600)
    h, s = taps_of("default", L, M, rng)
    N = 3
    refs = [rs.Stream(h, L, M, s) for _ in range(N)]
    first = [(k, rs.random_iq(rng, 50 + 13 * k, run=3)) for k in range(N)]
    second = [(k, rs.random_iq(rng, 200 + 31 * k, run=3)) for k in range(N)]
    want = [[refs[k].run(x) for k, x in first], [refs[k].run(x) for k, x in second]]
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        got0 = play(ctx, bank, [first], want[:1])
        P = [bank.consumed(k) for k in range(N)]
        assert P == [len(x) for _, x in first]
        need = [len(w) for w in want[1]]
        # capacity short on one run of three: every count comes back, nothing moves
        short = list(need)
        short[1] -= 1
        with pytest.raises(AdsbError) as e:
            play(ctx, bank, [second], want[1:], caps=[short])
        assert e.value.status == _lib.ADSB_ERR_CAPACITY and e.value.required.tolist() == need
        assert [bank.consumed(k) for k in range(N)] == P
        with torch.cuda.stream(ctx.torch_stream):
            d_in = [torch.from_numpy(x).cuda() for _, x in second]
            d_out = [torch.full((n + TAIL, 2), CANARY, dtype=torch.int16, device="cuda") for n in need]
        pin, pout = [t.data_ptr() for t in d_in], [t.data_ptr() for t in d_out]
        lens = [len(x) for _, x in second]
        for what, args in [("a stream named twice", ([0, 1, 0], pin, lens, pout, need)),
                           ("a stream past N", ([0, 1, N], pin, lens, pout, need)),
                           ("more runs than streams", ([0, 1, 2, 1], pin + pin[:1], lens + lens[:1], pout + pout[:1], need + need[:1])),
                           ("a misaligned input", ([0, 1, 2], [pin[0], pin[1] + 4, pin[2]], lens, pout, need)),
                           ("a misaligned output", ([0, 1, 2], pin, lens, [pout[0], pout[1], pout[2] + 8], need)),
                           ("no input", ([0, 1, 2], [pin[0], 0, pin[2]], lens, pout, need)),
                           ("no output", ([0, 1, 2], pin, lens, [0, pout[1], pout[2]], need)),
                           ("a format there is not", None)]:
            with pytest.raises(AdsbError) as e:
                if args is None:
                    bank.run_device([0, 1, 2], pin, lens, pout, need, format=4)
                else:
                    bank.run_device(*args)
            assert e.value.status == _lib.ADSB_ERR_INVALID, what
            assert [bank.consumed(k) for k in range(N)] == P, what
        with pytest.raises(AdsbError):
            bank.reset(N)
        with pytest.raises(AdsbError):
            bank.consumed(N)
        with torch.cuda.stream(ctx.torch_stream):
            assert all((t.cpu().numpy() == CANARY).all() for t in d_out)   # nothing was enqueued
        # a call of no runs, and then the refused call again: the right bytes
        assert bank.run_device([], [], [], [], []).tolist() == []
        got1 = play(ctx, bank, [second], want[1:])
        assert_equal(got0 + got1, want)
        assert [bank.consumed(k) for k in range(N)] == [r.P for r in refs]


# ----------------------------------------------------------------------------------------------- 8. with receivers
def frames_by_chunk(msgs):
    out = {}
    for m in msgs:
        out.setdefault(m.chunk, []).append((m.buffer().hex(), m.j, m.try_phase))
    return out


def test_end_to_end_with_receivers(hip_lib, golden, fixture_iq):
    """The aggregator's loop: one bank call resamples one buffer per receiver into consecutive slots of one allocation,
    and the _rx pass behind it -- nothing in between -- finds each capture's reference frames under its receiver."""
    import torch
    from dump1090_rs_amd import Context
    L, M = 2, 5
    fixtures = golden["fixtures"]
    assert len(fixtures) == 3
    rng = np.random.default_rng(9700)
    xs = [rs.hold_input(fixture_iq[fx["file"]], L, M, rng) for fx in fixtures]   # x[floor(n M / L)] = capture[n]
    expect = [list(zip(fx["frames"], fx["j"], fx["try_phase"])) for fx in fixtures]
    with Context(0, 3) as c, c.resampler_bank(3, L, M, [1, 1], 0) as bank:
        c.set_receivers(3)
        d_in = [torch.from_numpy(x).cuda() for x in xs]
        slots = torch.empty((3 * CHUNK, 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        for streams in ([0, 1, 2], [0, 2]):
            for r in streams:
                c.icao_flush_receiver(r)
            bank.reset()
            for r in streams:
                assert bank.inputs_for(r, CHUNK) == (len(xs[r]), CHUNK)
            n = bank.run_device(streams, [d_in[r].data_ptr() for r in streams], [len(xs[r]) for r in streams],
                                [slots.data_ptr() + 4 * CHUNK * k for k in range(len(streams))], [CHUNK] * len(streams))
            assert n.tolist() == [CHUNK] * len(streams)
            msgs = c.demod_iq_device_rx(slots.data_ptr(), len(streams) * CHUNK, streams)
            got = frames_by_chunk(msgs)
            assert sorted(got) == list(range(len(streams)))
            for k, r in enumerate(streams):
                assert got[k] == expect[r] and len(got[k]) in (5, 6), (streams, r)


def test_golden_captures_through_the_default_filter_equal_three_handles(hip_lib, ctx, golden, fixture_iq):
    import torch
    from dump1090_rs_amd import default_resampler_taps
    L, M = 6, 25
    h, s = default_resampler_taps(L, M)
    # each capture as a radio at 10 MS/s would have delivered it: interpolated by 25/6
    xs = [rs.resample(fixture_iq[fx["file"]], rs.hamming_sinc_taps(M, L), M, L, 14) for fx in golden["fixtures"]]
    xs = [np.ascontiguousarray(x[: rs.inputs_for(L, M, 0, CHUNK)]) for x in xs]
    want = [[np.empty((CHUNK, 2), np.int16)] * 3]
    with ctx.resampler_bank(3, L, M, h, s) as bank:
        got = play(ctx, bank, [[(k, x) for k, x in enumerate(xs)]], want)
        for k, x in enumerate(xs):
            with ctx.resampler(L, M, h, s) as res, torch.cuda.stream(ctx.torch_stream):
                d_in = torch.from_numpy(x).cuda()
                d_out = torch.empty((CHUNK, 2), dtype=torch.int16, device="cuda")
                assert res.run_device(d_in.data_ptr(), len(x), d_out.data_ptr(), CHUNK) == CHUNK
                single = d_out.cpu().numpy()
            assert got[0][k].tobytes() == single.tobytes(), k
            assert got[0][k].any()

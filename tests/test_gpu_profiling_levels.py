"""adsb_set_profiling chooses the code a pass runs through, not only what is timed: at level 2 no pass is one launch
(three launches with an inline tail, two scan streams instead of four, a reset launch of its own behind an icao_flush, the
fresh_q edge, never a ring slot read in place, never a rematch, classic event records on up to three streams that
adsb_collect reads back), at level 0 nothing is timed at all.  The rest of the suite runs at the default level 1; the
benchmark and the measuring tools quote numbers from levels 0 and 2.  So here every entry point runs at levels 0 and 2
against the CPU oracle -- tolerance 0 on (chunk, j, try_phase, score, msg, signal_level), in count and order, never
against the library at another level -- and proves that the level took effect: the timing fields of adsb_get_stats after
every call (tests/profiling_support.py: assert_level) and adsb_host_rematches, which cannot grow at level 2.

The streams and their oracle answers are built once (tests/profiling_support.py; every builder asserts its scenario is
not vacuous and can be checked without a GPU)."""
import numpy as np
import pytest

from tests import profiling_support as P
from tests.profiling_support import CHUNK, assert_level, rematches, replays, run_pipeline
from tests.test_gpu_small_pass import key, ring_stream

pytestmark = pytest.mark.gpu
LEVELS = (0, 2)


def keys(msgs):
    return [key(m) for m in msgs]


def on_device(a):
    import torch
    d = torch.from_numpy(np.array(a)).cuda()   # (a copy: the streams are shared between the tests and kept read-only)
    torch.cuda.synchronize()
    return d


def opened(max_chunks, level):
    from dump1090_rs_amd import Context
    c = Context(0, max_chunks)
    try:
        c.set_profiling(level)
    except BaseException:
        c.close()
        raise
    return c


def soapy_table(c):
    """the CU8 wants were widened through T_soapy: a new context's table"""
    from tests.test_gpu_u8 import T
    assert np.array_equal(c.u8_table(), T)


@pytest.fixture(scope="module")
def streams(oracle_mod):
    """tests/profiling_support.py with the oracle built: its builders keep what they made for the module's other tests."""
    return P


# ------------------------------------------------------------------------------------------------- 1. blocking calls
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("max_chunks", [1, 16, 17])
def test_blocking_calls_host_and_resident_in_both_formats(hip_lib, streams, max_chunks, level):
    """max_chunks buffers and a ragged one: a call cut into two passes (18 one-buffer passes in a context of 1)."""
    iq, want, raw, want8 = streams.blocking(max_chunks)
    d, d8 = on_device(iq), on_device(raw)
    with opened(max_chunks, level) as c:
        soapy_table(c)
        calls = [(lambda: c.demod_iq(iq, cap=1 << 17), want), (lambda: c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 17), want),
                 (lambda: c.demod_iq_u8(raw, cap=1 << 17), want8), (lambda: c.demod_iq_device_u8(d8.data_ptr(), len(raw), cap=1 << 17), want8)]
        for k, (call, w) in enumerate(calls):
            c.icao_flush()
            assert keys(call()) == w, k
            assert_level(c, level, k)
            assert c.stats()["n_chunks"] == max_chunks + 1 and c.stats()["retries"] == 0
        assert rematches(c) == 0


# ------------------------------------------------------------------------------------------------- 2. the pipeline full
@pytest.mark.parametrize("level", [2, 1, 0])
@pytest.mark.parametrize("max_chunks,per_pass", [(1, 1), (16, 3)])
def test_pipeline_full_over_folded_bitmaps_teach_then_need(hip_lib, streams, max_chunks, per_pass, level):
    """24 passes eight deep: the pass that needs an address is submitted while the pass that teaches it is in flight.  At
    level 2 the stream edges alone must order them (no rematch); levels 1 and 0 are one-launch passes that the host
    matches again -- the contrast that shows the stream exercises the ordering."""
    iq, wants = streams.planted(per_pass)
    d = on_device(iq)
    per = per_pass * CHUNK
    with opened(max_chunks, level) as c:
        assert c.max_in_flight() == 8
        c.icao_flush()
        got = run_pipeline(c, P.N_PIPE, lambda k: c.submit_iq_device(d.data_ptr() + 4 * k * per, min(per, len(iq) - k * per)), 8, level)
        assert got == wants, [k for k, (g, w) in enumerate(zip(got, wants)) if g != w]
        P.check_planted(got)
        if level == 2:
            assert rematches(c) == 0
        else:
            assert rematches(c) >= 1


# ------------------------------------------------------------------------------------------------- 3. flushes
@pytest.mark.parametrize("flushes", [P.FLUSH_EVERY, P.FLUSH_SOME], ids=["every", "some"])
@pytest.mark.parametrize("max_chunks,per_pass", [(1, 1), (16, 2)])
def test_flushes_in_a_full_pipeline_of_three_launch_passes(hip_lib, streams, max_chunks, per_pass, flushes):
    """Level 2, eight deep: the pass behind an icao_flush clears the next folded bitmap with a launch of its own, and the
    passes behind it -- which need what it teaches -- are put behind it while it is in flight; what was known only before
    the flush must not decode.  Twice over on one context: 40 passes, the nine bitmaps of the rotation wrap."""
    iq, wants = streams.flushed(per_pass, flushes)
    d = on_device(iq)
    per = per_pass * CHUNK
    with opened(max_chunks, 2) as c:
        for rep in range(2):
            got = run_pipeline(c, P.N_FLUSH, lambda k: c.submit_iq_device(d.data_ptr() + 4 * k * per, min(per, len(iq) - k * per)), 8, 2,
                               flushes)
            assert got == wants[rep], (rep, [k for k, (g, w) in enumerate(zip(got, wants[rep])) if g != w])
        assert rematches(c) == 0


# ------------------------------------------------------------------------------------------------- 4. the ring
@pytest.mark.parametrize("u8", [False, True], ids=["cs16", "cu8"])
@pytest.mark.parametrize("level,per_slot,depth", [(0, 1, 8), (2, 1, 8), (2, 2, 8), (2, 3, 8), (2, 16, 8), (2, 20, 4)])
def test_the_ring_in_both_formats(hip_lib, streams, level, per_slot, depth, u8):
    """13 slots, the last ragged, flushes before slots 0 and 7, twice over.  At level 2 no slot is read in place: every
    one goes through the copy engine on its pass's scan stream, of which there are two."""
    raw, want = streams.ring(per_slot, u8)
    with opened(per_slot, level) as c:
        soapy_table(c)
        (c.ring_create_u8 if u8 else c.ring_create)(per_slot * CHUNK)
        fed = P.Probed(c, level, u8)
        for rep in range(2):
            got = ring_stream(fed, raw, per_slot * CHUNK, depth, set(P.RING_FLUSH))
            assert [(s,) + key(m) for s, m in got] == want, rep
        if level == 2:
            assert rematches(c) == 0


# ------------------------------------------------------------------------------------------------- 5. magnitudes, carry-over
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("max_chunks", [1, 16])
def test_caller_magnitudes_with_a_lead_in(hip_lib, streams, max_chunks, level):
    from dump1090_rs_amd import MagnitudeBuffer
    with opened(max_chunks, level) as c:
        for rep in range(2):
            c.icao_flush()
            for data, n, want in streams.magnitudes():
                mb = MagnitudeBuffer()
                mb.data[:] = data
                mb.length = n
                assert keys(c.demodulate2400(mb)) == want, n
                assert_level(c, level, n)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("max_chunks", [1, 16])
def test_carry_over_blocking_and_with_the_pipeline_full(hip_lib, streams, max_chunks, level):
    """One stream in ten calls cut at awkward places (two shorter than the lead-in), frames across the calls' ends and
    across the buffer ends inside them, against oracle.binding.demod_iq_carry."""
    iq, wants = streams.carry(max_chunks)
    b = P.carry_bounds(max_chunks)
    d = on_device(iq)
    with opened(max_chunks, level) as c:
        c.set_carry_over(True)
        c.icao_flush()
        for k, (a, z) in enumerate(zip(b[:-1], b[1:])):
            assert keys(c.demod_iq(iq[a:z], cap=1 << 17)) == wants[k], k
            assert_level(c, level, k)
        c.set_carry_over(True)      # restarts the stream
        c.icao_flush()
        got = run_pipeline(c, len(wants), lambda k: c.submit_iq_device(d.data_ptr() + 4 * b[k], b[k + 1] - b[k]), c.max_in_flight(), level)
        assert got == wants, [k for k, (g, w) in enumerate(zip(got, wants)) if g != w]
        assert rematches(c) == 0    # (carry-over passes share one scan stream: nothing to redo at any level)


# ------------------------------------------------------------------------------------------------- 6. dense, on the device
@pytest.mark.parametrize("level", LEVELS)
def test_dense_stream_ordered_and_scored_on_the_device(hip_lib, streams, level):
    """Passes of 17 buffers, four in flight, an icao_flush before the fourth: scan, tail and score streams, and at level 2
    an event on each that adsb_collect reads back.  Once the stream is known dense the host replays nothing."""
    caps, prime, wants = streams.dense()
    devs = [on_device(x) for x in caps]
    n = P.DENSE_N * CHUNK
    with opened(P.DENSE_N, level) as c:
        c.icao_flush()
        assert keys(c.demod_iq_device(devs[2].data_ptr(), n, cap=1 << 17)) == prime     # (tells the context how dense the stream is)
        assert_level(c, level, "priming call")
        assert replays(c) == 1
        got = run_pipeline(c, len(wants), lambda k: c.submit_iq_device(devs[P.DENSE_ORDER[k]].data_ptr(), n), 4, level, (0, 3))
        assert got == wants, [k for k, (g, w) in enumerate(zip(got, wants)) if g != w]
        assert replays(c) == 1 and c.stats()["n_records"] >= 8 * P.DENSE_N


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("mode", [1, 3])
def test_dense_stream_repaired_and_scored_on_the_device(hip_lib, streams, mode, level):
    """The same under error correction, on fix_scored_support.order_stream (its first 17 buffers) against that module's
    restatement."""
    from tests import fix_support as fs
    iq, wants = streams.dense_fix(mode)
    d = on_device(iq)
    fkeys = lambda msgs: [fs.key(m) for m in msgs]   # noqa: E731
    with opened(P.DENSE_N, level) as c:
        c.set_error_correction(mode)
        c.icao_flush()
        assert fkeys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 17)) == wants[0]
        assert_level(c, level, "priming call")
        assert replays(c) == 1
        got = run_pipeline(c, 4, lambda k: c.submit_iq_device(d.data_ptr(), len(iq)), 4, level, (0, 2), keys=fkeys)
        assert got == wants[1:], [k for k, (g, w) in enumerate(zip(got, wants[1:])) if g != w]
        assert replays(c) == 1


# ------------------------------------------------------------------------------------------------- 7. the fallbacks
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("u8", [False, True], ids=["cs16", "cu8"])
@pytest.mark.parametrize("n_buf", [1, 4])
def test_overflow_fallback_and_the_context_after_it(hip_lib, streams, n_buf, u8, level):
    """A pass whose address/parity list overflows is redone buffer by buffer through the reference-shaped kernel, on the
    context's two redo events and a temporary slot: at level 2 adsb_collect reads five events of it back and must return
    ADSB_OK (an error status raises here).  An ordinary pipelined stream on the same context afterwards."""
    raw, want = streams.overflowing(n_buf, u8)
    per_pass = 1 if n_buf == 1 else 2
    iq2, wants2 = streams.aftermath(per_pass)
    d, d2 = on_device(raw), on_device(iq2)
    per = per_pass * CHUNK
    with opened(n_buf, level) as c:
        soapy_table(c)
        for how in ("host", "device", "submit"):
            c.icao_flush()
            if how == "host":
                got = (c.demod_iq_u8 if u8 else c.demod_iq)(raw, cap=1 << 17)
            elif how == "device":
                got = (c.demod_iq_device_u8 if u8 else c.demod_iq_device)(d.data_ptr(), len(raw), cap=1 << 17)
            else:
                (c.submit_iq_device_u8 if u8 else c.submit_iq_device)(d.data_ptr(), len(raw))
                got = c.collect(cap=1 << 17)
            assert c.stats()["retries"] >= 1, how
            assert keys(got) == want, how
            assert_level(c, level, how)
        got = run_pipeline(c, len(wants2), lambda k: c.submit_iq_device(d2.data_ptr() + 4 * k * per, per), c.max_in_flight(), level, (0,))
        assert got == wants2, [k for k, (g, w) in enumerate(zip(got, wants2)) if g != w]
        assert c.stats()["retries"] == 0


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("max_chunks", [1, 4])
def test_caller_magnitudes_that_overflow(hip_lib, streams, max_chunks, level):
    from dump1090_rs_amd import MagnitudeBuffer
    data, n, want = streams.overflowing_magnitudes()
    per_pass = 1 if max_chunks == 1 else 2
    iq2, wants2 = streams.aftermath(per_pass)
    d2 = on_device(iq2)
    per = per_pass * CHUNK
    mb = MagnitudeBuffer()
    mb.data[:] = data
    mb.length = n
    with opened(max_chunks, level) as c:
        for rep in range(2):
            c.icao_flush()
            assert keys(c.demodulate2400(mb, cap=1 << 17)) == want
            assert c.stats()["retries"] >= 1
            assert_level(c, level, rep)
        got = run_pipeline(c, len(wants2), lambda k: c.submit_iq_device(d2.data_ptr() + 4 * k * per, per), c.max_in_flight(), level, (0,))
        assert got == wants2


# ------------------------------------------------------------------------------------------------- 8. receivers
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("max_chunks,n", [(1, 1), (16, 5)])
def test_receivers_with_the_pipeline_full(hip_lib, streams, max_chunks, n, level):
    """Five receivers, a map of its own per pass, eight passes in flight, one receiver flushed in the middle; one oracle
    per receiver (tests/receivers_support.py)."""
    from tests import receivers_support as RS
    from tests.test_gpu_receivers import tables_equal
    n_receivers = 5
    iq, passes, flushed, wants, model = streams.receivers_pipeline(n)
    d = on_device(iq)
    with opened(max_chunks, level) as c:
        c.set_receivers(n_receivers)

        def submit(k):
            a, z, mp, cut = passes[k]
            if k == P.RX_FLUSH_AT:
                c.icao_flush_receiver(flushed)
            c.submit_iq_device_rx(d.data_ptr() + 4 * a * CHUNK, (z - a) * CHUNK - cut, mp)

        got = run_pipeline(c, P.RX_PASSES, submit, c.max_in_flight(), level, keys=RS.keys)
        assert got == wants, [k for k, (g, w) in enumerate(zip(got, wants)) if g != w]
        tables_equal(c, model, n_receivers)
        if level == 2:
            assert rematches(c) == 0


@pytest.mark.parametrize("level", LEVELS)
def test_receivers_scored_on_the_device(hip_lib, streams, level):
    """A context of 17, three receivers, dense 17-buffer passes four deep through the keyed scoring kernels."""
    from tests import receivers_support as RS
    from tests.test_gpu_receivers import tables_equal
    n_receivers, n = 3, P.DENSE_N
    iq, maps, prime, wants, model = streams.receivers_dense()
    zeros = np.zeros(n, dtype=np.uint32)
    d = on_device(iq)
    with opened(n, level) as c:
        c.set_receivers(n_receivers)
        c.set_receiver_scoring(True)
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), n * CHUNK, zeros, cap=1 << 17)) == prime
        assert_level(c, level, "priming call")
        c.icao_flush()
        before = replays(c)
        got = run_pipeline(c, 4, lambda k: c.submit_iq_device_rx(d.data_ptr(), n * CHUNK, maps[k]), 4, level, keys=RS.keys)
        assert got == wants, [k for k, (g, w) in enumerate(zip(got, wants)) if g != w]
        tables_equal(c, model, n_receivers)
        counters = c.selftest_rx_score_counters()
        assert counters["taken"] >= 1 and counters["taken"] + (replays(c) - before) == 4, counters


# ------------------------------------------------------------------------------------------------- 9. signal statistics
def assert_records(got, want, what):
    assert len(got) == len(want), what
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), (what, name)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("max_chunks", [1, 16, 17])
def test_signal_statistics_of_every_kind_of_call(hip_lib, streams, max_chunks, level):
    """The blocking calls (cut into passes), submit / collect with the pipeline full, the ring at one buffer per slot:
    the records are signal_support's restatement field for field, the frames of the same run the oracle's."""
    iq, want = streams.stats_stream()
    exp = streams.stats_expect(max_chunks)
    d = on_device(iq)
    with opened(max_chunks, level) as c:
        c.set_signal_stats(True)
        for how in ("host", "device"):
            c.icao_flush()
            got = c.demod_iq(iq, cap=1 << 17) if how == "host" else c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 17)
            assert keys(got) == want, how
            assert_records(c.signal_stats(), exp["call"], how)
            assert_level(c, level, how)
        depth = c.max_in_flight()
        pieces, wants, records = exp["submit"]
        devs = [on_device(p) for p in pieces]
        done = 0
        for k in range(len(pieces) + depth):
            if c.pending() == depth or (k >= len(pieces) and c.pending()):
                assert keys(c.collect(cap=1 << 17)) == wants[done], done
                assert_records(c.signal_stats(), records[done], ("submit", done))
                assert_level(c, level, ("submit", done))
                done += 1
            if k < len(pieces):
                if k == 0:
                    c.icao_flush()
                c.submit_iq_device(devs[k].data_ptr(), len(pieces[k]))
        assert done == len(pieces)
        slots, wants, records = exp["ring"]
        c.ring_create(CHUNK)
        done = 0
        for k in range(len(slots) + depth):
            if c.pending() == depth or (k >= len(slots) and c.pending()):
                assert keys(c.collect(cap=1 << 17)) == wants[done], done
                assert_records(c.signal_stats(), records[done], ("ring", done))
                assert_level(c, level, ("ring", done))
                done += 1
            if k < len(slots):
                if k == 0:
                    c.icao_flush()
                buf = c.ring_acquire()
                buf[: len(slots[k])] = slots[k]
                c.ring_submit(len(slots[k]))
        assert done == len(slots)


# ------------------------------------------------------------------------------------------------- 10. shards
@pytest.mark.parametrize("level", LEVELS)
def test_sharded_capture_and_the_level_parked_between_its_phases(hip_lib, oracle_mod, streams, level):
    """A 34-buffer capture cut in two over two contexts of 17: scan, union, finish, one ordered replay -- the single
    oracle stream.  Between the phases the level cannot change."""
    from dump1090_rs_amd import sharding
    from dump1090_rs_amd._lib import ADSB_ERR_BUSY, AdsbError
    from dump1090_rs_amd.context import replay_records
    from tests.test_gpu_small_pass import want_key
    iq, want, reply = streams.sharded()
    d = on_device(iq)
    half = 17 * CHUNK
    ctxs = [opened(17, level), opened(17, level)]
    try:
        learned = [c.shard_scan(d.data_ptr() + 4 * k * half, half) for k, c in enumerate(ctxs)]
        assert P.SHARD_ICAO in learned[0].tolist() and P.SHARD_ICAO not in learned[1].tolist()
        for c in ctxs:
            with pytest.raises(AdsbError) as busy:
                c.set_profiling(1)
            assert busy.value.status == ADSB_ERR_BUSY
        union = np.unique(np.concatenate(learned))
        records = [c.shard_finish(union) for c in ctxs]
        got = replay_records(sharding.merge_records(records, [0, 17]), cap=1 << 17)
        assert keys(got) == want
        assert sorted({m.chunk for m in got if m.buffer() == reply}) == [10, 20, 30]
        # the refused call changed nothing: an ordinary pass on each context still runs at the level it was given
        first = [want_key(w) for w in oracle_mod.Oracle().demod_iq(iq[:2 * CHUNK])[0]]
        for c in ctxs:
            c.icao_flush()
            assert keys(c.demod_iq_device(d.data_ptr(), 2 * CHUNK)) == first
            assert_level(c, level, "after the shard")
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------------------------------------- 11. the level changing
@pytest.mark.parametrize("how", ["blocking", "submit", "ring"])
@pytest.mark.parametrize("max_chunks", [1, 16, 17])
def test_levels_changing_along_one_stream(hip_lib, streams, max_chunks, how):
    """24 passes of one oracle stream, the level changing every four in the order 1, 2, 0, 2, 1, 0: one-launch and three-
    launch passes take turns on the same slots, bitmaps and streams.  An address taught under one level is needed under
    the next; flushes land right before a change, right after one, and pending across one."""
    from dump1090_rs_amd import Context
    pieces, wants = streams.changing(max_chunks)
    devs = [on_device(p) for p in pieces] if how != "ring" else None
    got = []
    with Context(0, max_chunks) as c:
        if how == "ring":
            c.ring_create(max_chunks * CHUNK)
        for g in range(P.N_CHANGE // 4):
            level = P.LEVEL_CYCLE[g]
            pending_flush = 4 * g in P.CHANGE_FLUSH and g % 2 == 1
            if pending_flush:
                c.icao_flush()          # ... stays pending across the change
            c.set_profiling(level)
            for p in range(4 * g, 4 * g + 4):
                if p in P.CHANGE_FLUSH and not (pending_flush and p == 4 * g):
                    c.icao_flush()
                n = len(pieces[p])
                if how == "blocking":
                    got.append(keys(c.demod_iq_device(devs[p].data_ptr(), n, cap=1 << 17)))
                    assert_level(c, level, p)
                elif how == "submit":
                    c.submit_iq_device(devs[p].data_ptr(), n)
                else:
                    buf = c.ring_acquire()
                    buf[:n] = pieces[p]
                    c.ring_submit(n)
            while c.pending():
                got.append(keys(c.collect(cap=1 << 17)))
                assert_level(c, level, len(got) - 1)
        assert got == wants, [k for k, (g_, w) in enumerate(zip(got, wants)) if g_ != w]
        if how == "blocking":
            assert rematches(c) == 0


# ------------------------------------------------------------------------------------------------- 12. the call itself
def test_the_call_itself(hip_lib, streams):
    """NULL, busy, clamping, the default -- the level seen through the timing fields and adsb_host_rematches only."""
    from dump1090_rs_amd import Context
    from dump1090_rs_amd._lib import ADSB_ERR_BUSY, ADSB_ERR_INVALID, AdsbError
    assert hip_lib.adsb_set_profiling(None, 1) == ADSB_ERR_INVALID
    iq, wants = streams.planted(1)
    d = on_device(iq)
    submit = lambda c: (lambda k: c.submit_iq_device(d.data_ptr() + 4 * k * CHUNK, min(CHUNK, len(iq) - k * CHUNK)))   # noqa: E731
    with Context(0, 1) as c:
        # a fresh context is at level 1
        c.icao_flush()
        assert keys(c.demod_iq_device(d.data_ptr(), CHUNK)) == wants[0]
        assert_level(c, 1, "fresh")
        # refused while a pass is pending, and nothing changes
        c.submit_iq_device(d.data_ptr() + 4 * CHUNK, CHUNK)
        with pytest.raises(AdsbError) as busy:
            c.set_profiling(2)
        assert busy.value.status == ADSB_ERR_BUSY
        assert keys(c.collect()) == wants[1]
        assert_level(c, 1, "after the refusal")
        # ... and while a shard is parked between its phases
        c.icao_flush()
        c.shard_scan(d.data_ptr(), CHUNK)
        with pytest.raises(AdsbError) as busy:
            c.set_profiling(0)
        assert busy.value.status == ADSB_ERR_BUSY
        c.shard_finish(np.zeros(0, np.uint32))
        # -5 is level 0: nothing timed, one-launch passes that the host matches again
        c.set_profiling(-5)
        c.icao_flush()
        before = rematches(c)
        assert run_pipeline(c, P.N_PIPE, submit(c), 8, 0) == wants
        assert rematches(c) >= before + 1
        # 9 is level 2: every kernel timed, no pass is one launch, nothing is matched again
        c.set_profiling(9)
        c.icao_flush()
        before = rematches(c)
        assert run_pipeline(c, P.N_PIPE, submit(c), 8, 2) == wants
        assert rematches(c) == before

"""Many receivers, one pass, scored on the device (include/adsb_hip.h: adsb_set_receiver_scoring): dense passes of a large
context with one ICAO filter per receiver go through k_rx_adders / k_score_rx / k_emit_rx instead of the host's replay.
Every list is compared with tests/receivers_support.py's Model -- one CPU oracle (or fix restatement) per receiver -- at
tolerance 0, and every parity test first asserts that one shared filter would give a different list for its input.

The shape is the smallest at which any of this can go wrong: Context(0, 20), passes of 20 buffers, four in flight,
F.fill_capture(seed, 20, per_buffer=60) as the dense input.  A context enters dense mode only when a dense pass has been
collected, so every test primes with one blocking dense pass and a flush; that pass is the host's, so the first judged
pass rebuilds the keyed set once (counter "rebuilds" + 1, from empty filters)."""
from functools import lru_cache

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS
from tests.test_gpu_receivers import expect_passes, on_device, quantise, random_maps, tables_equal, widen

pytestmark = pytest.mark.gpu
CHUNK = RS.CHUNK
N = 20


@lru_cache(maxsize=None)
def dense(seed=900, n=N, per_buffer=60):
    iq = F.fill_capture(seed, n, per_buffer=per_buffer)
    iq.setflags(write=False)
    return iq


def replays(c):
    return int(c._L.adsb_host_replays(c._h))


class Scored:
    """A Context(0, 20) with receivers and scoring on, primed into dense mode; `since()` is what the counters and
    adsb_host_replays have moved by since the priming (or the last mark())."""

    def __init__(self, n_receivers, mode=0, scoring=True, max_chunks=N):
        from dump1090_rs_amd import Context
        self.c = Context(0, max_chunks)
        self.n_receivers = n_receivers

        def opened():
            c = self.c
            c.set_receivers(n_receivers)
            if mode:
                c.set_error_correction(mode)
            if scoring:
                c.set_receiver_scoring(True)
            if max_chunks > 16:
                d = on_device(dense())
                c.demod_iq_device_rx(d.data_ptr(), N * CHUNK, np.zeros(N, dtype=np.uint32), cap=1 << 17)
                assert c.stats()["n_records"] >= 8 * N
                c.icao_flush()
            self.mark()
        try:
            opened()
        except BaseException:
            self.c.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.close()

    def mark(self):
        self.base = dict(self.c.selftest_rx_score_counters(), replays=replays(self.c))

    def since(self):
        now = dict(self.c.selftest_rx_score_counters(), replays=replays(self.c))
        return {k: now[k] - self.base[k] for k in now}


def collect_dense(c, n=N):
    got = RS.keys(c.collect(cap=1 << 17))
    assert c.stats()["n_records"] >= 8 * n
    return got


def run_pipeline(c, passes, submit, depth=4, before=None):
    """tests.test_gpu_receivers.pipeline, asserting of every pass collected that it was dense"""
    got = []
    for k, p in enumerate(passes):
        if c.pending() == depth:
            got.append(collect_dense(c, p[1] - p[0]))
        for r in (before or {}).get(k, []):
            c.icao_flush() if r is None else c.icao_flush_receiver(r)
        submit(k, p)
    while c.pending():
        got.append(collect_dense(c, passes[len(got)][1] - passes[len(got)][0]))
    return got


# ------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
def test_parity_with_the_pipeline_full(hip_lib, oracle_mod, fmt):
    """Four receivers, four passes of 20 buffers with a different random map each, submitted four deep: the lists and the
    tables equal the model's, no pass is replayed by the host, four device results are taken."""
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 9)
    passes = [(0, N, mp, 0) for mp in maps]
    with Scored(n_receivers) as s:
        c = s.c
        raw = quantise(dense()) if fmt == "cu8" else dense()
        meant = widen(c, raw) if fmt == "cu8" else dense()
        wants, shareds, model = expect_passes(n_receivers, meant, passes)
        RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
        d = on_device(raw)
        call = c.submit_iq_device_rx_u8 if fmt == "cu8" else c.submit_iq_device_rx
        for p in passes:
            call(d.data_ptr(), N * CHUNK, p[2])
        assert c.pending() == 4
        got = [collect_dense(c) for _ in passes]
        assert got == wants
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 4, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}
        # once more without a flush: every address is in the keyed set now, nothing is rebuilt
        again = [model.feed(meant, p[2]) for p in passes]
        assert again != wants
        assert run_pipeline(c, passes, lambda k, p: call(d.data_ptr(), N * CHUNK, p[2])) == again
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 8, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}


def test_blocking_call_cut_into_passes_and_the_plain_calls(hip_lib, oracle_mod):
    """adsb_demod_iq_device_rx over 45 buffers is cut into 20 + 20 + 5: two scored passes and a small one the host scores;
    the scored passes of the next call rebuild the keyed set from filters that are no longer empty.  Then the plain call
    on the same context: every buffer is receiver 0, scored on the device all the same."""
    n_receivers, n = 3, 45
    iq = dense(901, n)
    (m1, m2) = random_maps(n_receivers, [n, n], 11)
    own, shared = RS.Model(n_receivers), RS.Model(n_receivers, shared=True)
    want = [own.feed(iq, m1), own.feed(iq, m2)]
    RS.assert_tells_apart(n_receivers, sum(want, []), shared.feed(iq, m1) + shared.feed(iq, m2))
    d = on_device(iq)
    with Scored(n_receivers) as s:
        c = s.c
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), n * CHUNK, m1, cap=1 << 18)) == want[0]
        assert c.stats()["n_records"] >= 8 * n
        assert s.since() == {"taken": 2, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 1}
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), n * CHUNK, m2, cap=1 << 18)) == want[1]
        assert s.since() == {"taken": 4, "refused": 0, "rebuilds": 2, "no_room": 0, "replays": 2}
        tables_equal(c, own, n_receivers)
        plain = own.feed(iq[:N * CHUNK], np.zeros(N, dtype=np.uint32))
        assert RS.keys(c.demod_iq_device(d.data_ptr(), N * CHUNK, cap=1 << 17)) == plain
        assert s.since() == {"taken": 5, "refused": 0, "rebuilds": 3, "no_room": 0, "replays": 2}
        tables_equal(c, own, n_receivers)


def test_the_ring_on_a_large_context(hip_lib, oracle_mod):
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 13)
    passes = [(0, N, mp, 0) for mp in maps]
    wants, shareds, model = expect_passes(n_receivers, dense(), passes)
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    with Scored(n_receivers) as s:
        c = s.c
        c.ring_create(N * CHUNK)

        def submit(k, p):
            buf = c.ring_acquire()
            buf[:N * CHUNK] = dense()
            c.ring_submit_rx(N * CHUNK, p[2])

        assert run_pipeline(c, passes, submit, depth=3) == wants
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 4, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}


def test_scored_passes_of_either_kind_leave_the_tables_empty_for_the_other(hip_lib, oracle_mod):
    """One context: two pipelined dense passes with receivers and scoring on (k_score_rx / k_emit_rx), adsb_set_receivers(0)
    and two plain ones (k_score / k_emit), receivers on again and two more.  Each kind of pass scores against first-adder
    tables that the kind before it has to have left empty (an entry left behind makes a later trial of that address look
    like one that comes after its first adder: 1000 for -1); every list equals the model's, which restarts from empty
    filters at each switch, as adsb_set_receivers documents.
    The counts of which passes the device scored are those of this test body on the commit that gave k_emit and k_emit_rx
    one shared body, run against its parent's library, not this build's own."""
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd._lib import AdsbError
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 29)
    zeros = np.zeros(N, dtype=np.uint32)
    d = on_device(dense())

    def empty_restart(c, n):
        assert c.receivers() == n
        if n:
            assert not any(c.receiver_filter_table(r).any() for r in range(n))
        else:
            with pytest.raises(AdsbError) as e:
                c.receiver_filter_table(0)
            assert e.value.status == _lib.ADSB_ERR_INVALID

    with Scored(n_receivers) as s:
        c = s.c
        rx = lambda k, p: c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, p[2])   # noqa: E731
        plain = lambda k, p: c.submit_iq_device(d.data_ptr(), N * CHUNK)         # noqa: E731
        # receivers on, scoring on
        passes = [(0, N, mp, 0) for mp in maps[:2]]
        wants, shareds, model = expect_passes(n_receivers, dense(), passes)
        RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
        assert run_pipeline(c, passes, rx) == wants
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 2, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}
        # receivers off: a plain context, from an empty filter
        c.set_receivers(0)
        empty_restart(c, 0)
        one = RS.Model(1)
        want_plain = [one.feed(dense(), zeros) for _ in range(2)]
        assert want_plain[0] != want_plain[1]
        assert run_pipeline(c, [(0, N, zeros, 0)] * 2, plain) == want_plain
        assert s.since() == {"taken": 2, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}   # (k_score / k_emit)
        # receivers on again: every receiver from an empty filter, the keyed set rebuilt
        c.set_receivers(n_receivers)
        empty_restart(c, n_receivers)
        passes = [(0, N, mp, 0) for mp in maps[2:]]
        wants, shareds, model = expect_passes(n_receivers, dense(), passes)
        RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
        assert run_pipeline(c, passes, rx) == wants
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 4, "refused": 0, "rebuilds": 2, "no_room": 0, "replays": 0}


# ------------------------------------------------------------------------------------------------- 2. isolation
X = 0x4B1A2C
DF17_X = synth.df17_frame(X, 0x58B986D0B3BD25)
REPLY_X = F.ap_frame(4, X, 0x1234567)[:7]
DF18_X = F.es_frame(18, X, 0x58B986D0B3BD25)
A, B = 0, 1


def spiked(items, seed=900):
    """The dense input with frames of our own: (buffer, frame) in a stretch of that buffer made quiet first."""
    iq = dense(seed).copy()
    bursts = []
    for k, (b, frame) in enumerate(items):
        j = 40000 + 977 * k
        a = b * CHUNK + j
        iq[a - 100:a + 500] = synth.noise_numpy(600, seed=4242 + k)
        bursts.append(synth.Burst(5 * a + 1 + k, 24000, 1 + k, frame))
    synth.add_bursts(iq, bursts)
    return iq


def where(ks, frame):
    return sorted({(k[0], k[3]) for k in ks if k[4] == frame})


def map_ab(**receiver_of):
    """every buffer receiver 2 or 3 (bystanders), but for the named ones: map_ab(b3=A, b5=B)"""
    m = np.array([2 + b % 2 for b in range(N)], dtype=np.uint32)
    for name, r in receiver_of.items():
        m[int(name[1:])] = r
    return m


def test_isolation_spelled_out(hip_lib, oracle_mod):
    """In ONE pass receiver A hears a clean DF17 of X in buffer 3, B gets an address/parity reply of X in buffer 5 and A
    one in buffer 7: A's is emitted with score 1000, B's is not (the keyed first-adder table).  The same across two passes
    (the keyed set).  With the order reversed A's reply in front of its DF17 is not emitted either; and an aircraft known
    from DF18 alone never makes a later reply score 1000."""
    n_receivers = 4
    one = spiked([(3, DF17_X), (5, REPLY_X), (7, REPLY_X)])
    first, second = spiked([(3, DF17_X)]), spiked([(5, REPLY_X), (7, REPLY_X)])
    reverse = spiked([(3, REPLY_X), (7, DF17_X)])
    only18 = spiked([(3, DF18_X), (7, REPLY_X)])
    m = map_ab(b3=A, b5=B, b7=A)
    with Scored(n_receivers) as s:
        c = s.c

        def judged(inputs, expect_where):
            """a flush, then the inputs as consecutive scored passes: equal to the model, which says `expect_where`"""
            c.icao_flush()
            own, shared = RS.Model(n_receivers), RS.Model(n_receivers, shared=True)
            wants = [own.feed(iq, m) for iq in inputs]
            shareds = [shared.feed(iq, m) for iq in inputs]
            RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
            assert [where(w, REPLY_X) for w in wants] == expect_where
            devs = [on_device(iq) for iq in inputs]
            passes = [(0, N, m, 0)] * len(inputs)
            got = run_pipeline(c, passes, lambda k, p: c.submit_iq_device_rx(devs[k].data_ptr(), N * CHUNK, m))
            assert got == wants
            assert [where(g, REPLY_X) for g in got] == expect_where
            tables_equal(c, own, n_receivers)
            return shareds

        shared = judged([one], [[(7, 1000)]])
        assert where(shared[0], REPLY_X) == [(5, 1000), (7, 1000)]
        judged([first, second], [[], [(7, 1000)]])
        judged([reverse], [[]])
        judged([only18], [[]])
        judged([only18, second], [[], []])
        since = s.since()
        assert since["taken"] == 7 and since["replays"] == 0 and since["refused"] == 0, since


# ------------------------------------------------------------------------------------------------- 3. flushes
def test_flush_of_all_rotates_the_set_and_flush_of_one_receiver_rebuilds_it(hip_lib, oracle_mod):
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 17)
    passes = [(0, N, mp, 0) for mp in maps]
    d = on_device(dense())
    with Scored(n_receivers) as s:
        c = s.c
        submit = lambda k, p: c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, p[2])   # noqa: E731
        # adsb_icao_flush between pipelined scored passes: nothing is drained or rebuilt
        before = {2: [None]}
        wants, shareds, model = expect_passes(n_receivers, dense(), passes, before=before)
        RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
        assert wants[2] != wants[0] or maps[2].tolist() != maps[0].tolist()
        assert run_pipeline(c, passes, submit, before=before) == wants
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 4, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}
        # adsb_icao_flush_receiver(1) with three passes in flight: the next scored pass drains and rebuilds
        c.icao_flush()
        s.mark()
        before = {3: [1]}
        wants, shareds, model = expect_passes(n_receivers, dense(), passes, before=before)
        unflushed = expect_passes(n_receivers, dense(), passes)[0]
        assert wants[3] != unflushed[3]
        assert run_pipeline(c, passes, submit, before=before) == wants
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 4, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}


# ------------------------------------------------------------------------------------------------- 4. error correction
@pytest.mark.parametrize("mode", [1, 3])
def test_error_correction_repairs_for_the_receiver_that_knows_the_aircraft(hip_lib, oracle_mod, mode):
    """A dense pass of 12 buffers of every format with damaged copies (three receivers' captures) and 8 fill buffers; in
    the fill buffers a clean DF17 of X for A (13), a damaged DF17 of X for B (15) and for A (17): repaired -- 1200, or 1100
    for two bits -- for A alone, by the device."""
    n_receivers = 3
    bits = (40,) if mode == 1 else (40, 77)
    score = 1200 if mode == 1 else 1100
    repaired = synth.df17_frame(X, 0x99AA5511223344)
    damaged = F.flip(repaired, *bits)
    fix_iq, fix_map = RS.batch(n_receivers, 4, fix=True)
    iq = np.concatenate([fix_iq, dense(902, 8)])
    for k, b in enumerate((13, 15, 17)):
        a = b * CHUNK + 40000 + 977 * k
        iq[a - 100:a + 500] = synth.noise_numpy(600, seed=777 + k)
    at = lambda k, b: 5 * (b * CHUNK + 40000 + 977 * k) + 1 + k   # noqa: E731
    synth.add_bursts(iq, [synth.Burst(at(0, 13), 24000, 1, DF17_X), synth.Burst(at(1, 15), 24000, 2, damaged),
                          synth.Burst(at(2, 17), 24000, 3, damaged)])
    m = np.concatenate([fix_map, np.array([2, A, 2, B, 2, A, 1, 0], dtype=np.uint32)])
    m2 = np.concatenate([fix_map[::-1], np.array([0, 1, 2, A, 2, A, 1, B], dtype=np.uint32)])
    own, shared = RS.Model(n_receivers, mode), RS.Model(n_receivers, mode, shared=True)
    wants = [own.feed(iq, m), own.feed(iq, m2)]
    shareds = [shared.feed(iq, m), shared.feed(iq, m2)]
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    assert where(wants[0], repaired) == [(17, score)] and where(shareds[0], repaired) == [(15, score), (17, score)]
    # (the second pass, no flush: buffers 15 and 17 are both A's now, and A knows X from the keyed set)
    assert where(wants[1], repaired) == [(15, score), (17, score)]
    assert sum(k[3] == 1200 for k in wants[0]) >= 5 * 12
    d = on_device(iq)
    with Scored(n_receivers, mode=mode) as s:
        c = s.c
        passes = [(0, N, m, 0), (0, N, m2, 0)]
        got = run_pipeline(c, passes, lambda k, p: c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, p[2]))
        assert got == wants
        tables_equal(c, own, n_receivers)
        assert s.since() == {"taken": 2, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}


# ------------------------------------------------------------------------------------------------- 5. a filter near full
def test_a_receiver_whose_table_fills_up_is_left_to_the_host(hip_lib, oracle_mod):
    """Two receivers; receiver 0 gets 18 of every 20 buffers of a stream of new aircraft (80 frames a buffer) until its
    table is past 4096 - 64 and then full.  While it is far from that the device's results are taken; once it is within 64
    of full every pass that adds to it is refused and replayed by the host, which reproduces the reference on a full table."""
    n_receivers, n_passes = 2, 6
    iq = dense(903, n_passes * N, 80)
    m = np.array([0] * 18 + [1] * 2, dtype=np.uint32)
    own, shared = RS.Model(n_receivers), RS.Model(n_receivers, shared=True)
    d = on_device(iq)
    held = lambda r: sum(a != 0 for a in own.table(r))   # noqa: E731
    wants, shareds = [], []
    with Scored(n_receivers) as s:
        c = s.c
        refused_when_near_full = 0
        for k in range(n_passes):
            before, counters = held(0), s.since()
            part = iq[k * N * CHUNK:(k + 1) * N * CHUNK]
            wants.append(own.feed(part, m))
            shareds.append(shared.feed(part, m))
            c.submit_iq_device_rx(d.data_ptr() + 4 * k * N * CHUNK, N * CHUNK, m)
            assert RS.keys(c.collect(cap=1 << 17)) == wants[-1], k
            assert c.stats()["n_records"] >= 8 * N
            now = s.since()
            if k < 2:   # (about 900 addresses a pass: nowhere near)
                assert held(0) < 2500 and now["taken"] == counters["taken"] + 1, (k, now)
            if before + 64 >= 4096:
                assert held(0) >= before and now["refused"] == counters["refused"] + 1 and now["replays"] == counters["replays"] + 1, (k, now)
                refused_when_near_full += 1
            tables_equal(c, own, n_receivers)
        RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
        assert held(0) == 4096 and held(1) < 1000 and refused_when_near_full >= 1
        assert s.since()["no_room"] == 0


# ------------------------------------------------------------------------------------------------- 6. out of probes
def test_out_of_probes_is_a_flag_and_a_host_replay(hip_lib, oracle_mod):
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 19)
    passes = [(0, N, mp, 0) for mp in maps]
    wants, shareds, model = expect_passes(n_receivers, dense(), passes)
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    d = on_device(dense())
    with Scored(n_receivers) as s:
        c = s.c
        submit = lambda k, p: c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, p[2])   # noqa: E731
        # 64 slots, 4 probes: the first pass's several hundred additions cannot all be placed
        c.selftest_rx_score_tune(6, 4)
        assert run_pipeline(c, passes, submit) == wants
        tables_equal(c, model, n_receivers)
        since = s.since()
        assert since["no_room"] >= 1 and since["taken"] == 0 and since["replays"] == 4, since
        # back to the defaults, from empty filters: scored on the device again
        c.selftest_rx_score_tune(0, 0)
        c.icao_flush()
        s.mark()
        assert run_pipeline(c, passes, submit) == wants
        tables_equal(c, model, n_receivers)
        assert s.since() == {"taken": 4, "refused": 0, "rebuilds": 1, "no_room": 0, "replays": 0}


# ------------------------------------------------------------------------------------------------- 7. the overflow fallback
def test_overflow_fallback_with_scoring_on(hip_lib, oracle_mod):
    """A periodic stretch inside one receiver's buffer overflows the lists of the second of three pipelined passes: it is
    redone buffer by buffer by the host, the pass scored behind it is disowned and replayed too, and the next one rebuilds
    the keyed set and is scored on the device again."""
    from tests.test_gpu_parity import ADVERSARIAL_PERIODS
    n_receivers = 3
    bad = dense().copy()
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 20000, CHUNK + 95000
    bad[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    bad[a:z, 1] = 0
    maps = random_maps(n_receivers, [N] * 4, 23)
    inputs = [dense(), bad, dense(), dense()]
    own, shared = RS.Model(n_receivers), RS.Model(n_receivers, shared=True)
    wants = [own.feed(iq, mp) for iq, mp in zip(inputs, maps)]
    shareds = [shared.feed(iq, mp) for iq, mp in zip(inputs, maps)]
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    devs = [on_device(dense()), on_device(bad)]
    dev_of = [devs[0], devs[1], devs[0], devs[0]]
    with Scored(n_receivers) as s:
        c = s.c
        got, retries = [], []
        for k in range(3):
            c.submit_iq_device_rx(dev_of[k].data_ptr(), N * CHUNK, maps[k])
        for k in range(3):
            got.append(RS.keys(c.collect(cap=1 << 18)))
            retries.append(c.stats()["retries"])
        assert got == wants[:3]
        assert retries[0] == 0 and retries[1] > 0 and retries[2] == 0
        since = s.since()
        assert since["taken"] == 1 and since["rebuilds"] == 1, since
        c.submit_iq_device_rx(dev_of[3].data_ptr(), N * CHUNK, maps[3])
        assert collect_dense(c) == wants[3]
        tables_equal(c, own, n_receivers)
        since = s.since()
        assert since["taken"] == 2 and since["rebuilds"] == 2, since


# ------------------------------------------------------------------------------------------------- 8. the keyed set alone
def model_set(keys, queries, lg, probe_max):
    """the table in plain Python, one insertion after the other: (found per query, insertions that ran out of probes,
    the longest run of occupied slots)"""
    from dump1090_rs_amd.context import rx_set_home
    mask, table, failed = (1 << lg) - 1, {}, 0
    for key in keys:
        h = rx_set_home(key, lg)
        for _ in range(probe_max):
            if table.get(h, key) == key:
                table[h] = key
                break
            h = (h + 1) & mask
        else:
            failed += 1
    found = []
    for q in queries:
        h, hit = rx_set_home(q, lg), False
        for _ in range(probe_max):
            if h not in table:
                break
            if table[h] == q:
                hit = True
                break
            h = (h + 1) & mask
        found.append(hit)
    run = longest = 0
    for h in range(2 << lg):   # (twice round: a run may wrap)
        run = run + 1 if (h & mask) in table else 0
        longest = max(longest, run)
    return found, failed, longest


def keys_at_home(home, lg, n, seed):
    """n distinct keys (receiver << 24 | value, value != 0) whose probes start at `home` in a set of 2^lg slots"""
    from dump1090_rs_amd.context import rx_set_home
    r = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = (r.integers(0, 16384, size=1 << 20, dtype=np.uint64) << np.uint64(24)) | r.integers(1, 1 << 24, size=1 << 20, dtype=np.uint64)
        with np.errstate(over="ignore"):
            h = (k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - lg)
        out += [int(x) for x in np.unique(k[h == np.uint64(home)]) if int(x) not in out]
    out = out[:n]
    assert all(rx_set_home(k, lg) == home for k in out)   # (the library's own word for it)
    return out


def test_the_keyed_set_alone(hip_lib):
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import rx_set_home
    key = lambda r, v: (r << 24) | v   # noqa: E731
    with Context(0, N) as c:
        c.set_receivers(4)
        c.set_receiver_scoring(True)
        lg = 15   # 2 x 4096 x 4 receivers
        # 64 keys that share one home slot (the default probe bound), and 64 absent ones with the same home
        same = keys_at_home(rx_set_home(key(1, 0x123456), lg), lg, 128, 5)
        present, absent = same[:64], same[64:]
        v = 0x4B1A2C
        edge = [key(0, v), key(1, v), key(16383, v), key(5, 0xFFFFFF), key(16383, 0xFFFFFF)]
        keys = present + edge
        queries = present + absent + edge + [key(2, v), key(16382, v), key(16383, 0xFFFFFE), key(0, 0xFFFFFF)]
        want = [True] * 64 + [False] * 64 + [True] * 5 + [False] * 4
        found, failed = c.selftest_rx_set_lookup(keys, queries)
        assert found.tolist() == want and failed == 0
        # every key twice, in another order: the same set
        found, failed = c.selftest_rx_set_lookup(keys + keys[::-1], queries)
        assert found.tolist() == want and failed == 0
        # one more key of that home than the probe bound reaches: exactly one insertion is out of probes
        found, failed = c.selftest_rx_set_lookup(same[:65], same[:65])
        assert failed == 1 and int(found.sum()) == 64
        # a run longer than a small probe bound: 64 slots, 8 probes, 40 keys of one home.  (The insertions run in
        # parallel: WHICH keys get the eight slots is not fixed, how many is, and that is what the model says too.)
        c.selftest_rx_score_tune(6, 8)
        small = keys_at_home(17, 6, 40, 6)
        far = [k for k in (key(3, 1000 + i) for i in range(400)) if (rx_set_home(k, 6) - 17) % 64 >= 8][:30]
        found, failed = c.selftest_rx_set_lookup(small, small + far)
        assert failed == 40 - 8 == model_set(small, [], 6, 8)[1]
        assert int(found[:40].sum()) == 8 and not found[40:].any()
        # keys of many homes whose runs stay shorter than the bound, in whatever order: the model's answers, slot for slot
        spread = [key(3, 1000 + i) for i in range(16)]
        want_found, want_failed, longest = model_set(spread, spread + small, 6, 8)
        assert longest <= 8 and want_failed == 0
        found, failed = c.selftest_rx_set_lookup(spread, spread + small)
        assert (found.tolist(), failed) == (want_found, want_failed)
        c.selftest_rx_score_tune(0, 0)
        assert c._L.adsb_selftest_rx_set_lookup(c._h, None, 1, None, 0, None) == -1


# ------------------------------------------------------------------------------------------------- 9. off and refusals
def test_off_by_default_and_on_then_off_again(hip_lib, oracle_mod):
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 9)
    passes = [(0, N, mp, 0) for mp in maps]
    wants, shareds, model = expect_passes(n_receivers, dense(), passes)
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    d = on_device(dense())
    with Scored(n_receivers, scoring=False) as s:
        c = s.c
        assert c.get_receiver_scoring() is False
        submit = lambda k, p: c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, p[2])   # noqa: E731
        c.set_receiver_scoring(True)
        assert c.get_receiver_scoring() is True
        c.set_receiver_scoring(False)
        assert c.get_receiver_scoring() is False
        assert run_pipeline(c, passes, submit) == wants
        assert s.since() == {"taken": 0, "refused": 0, "rebuilds": 0, "no_room": 0, "replays": 4}
        # BUSY while a pass is pending, and the setting stays what it was
        submit(0, passes[0])
        assert c._L.adsb_set_receiver_scoring(c._h, 1) == -7 and c._L.adsb_selftest_rx_score_tune(c._h, 6, 4) == -7
        c.collect(cap=1 << 17)
        assert c.get_receiver_scoring() is False
        assert c._L.adsb_set_receiver_scoring(None, 1) == -1 and c._L.adsb_get_receiver_scoring(None) == -1


def test_a_small_context_remembers_the_setting_and_the_host_scores(hip_lib, oracle_mod):
    n_receivers, n = 3, 4
    iq, m = RS.batch(n_receivers, 4)
    want, shared, model = RS.expectations(n_receivers, 4)
    RS.assert_tells_apart(n_receivers, want, shared)
    with Scored(n_receivers, max_chunks=n) as s:
        c = s.c
        assert c.get_receiver_scoring() is True
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == want
        tables_equal(c, model, n_receivers)
        since = s.since()
        assert since["replays"] == len(m) // n and since["taken"] == 0 and since["rebuilds"] == 0, since


def test_receivers_off_and_scoring_on_is_the_plain_path(hip_lib, oracle_mod):
    from dump1090_rs_amd import Context
    d = on_device(dense())
    lists = []
    for scoring in (False, True):
        with Context(0, N) as c:
            if scoring:
                c.set_receiver_scoring(True)
            got = [RS.keys(c.demod_iq_device(d.data_ptr(), N * CHUNK, cap=1 << 17))]
            before = replays(c)
            for _ in range(3):
                c.submit_iq_device(d.data_ptr(), N * CHUNK)
            got += [RS.keys(c.collect(cap=1 << 17)) for _ in range(3)]
            assert replays(c) == before   # (scored by k_score / k_emit, as always)
            assert c.selftest_rx_score_counters() == {"taken": 0, "refused": 0, "rebuilds": 0, "no_room": 0}
            lists.append(got)
    assert lists[0] == lists[1]
    model = RS.Model(1)
    assert lists[1] == [model.feed(dense(), np.zeros(N, dtype=np.uint32)) for _ in range(4)]

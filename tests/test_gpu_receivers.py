"""Many receivers, one pass (include/adsb_hip.h) through the device: a context with one ICAO filter per receiver, the
receiver of every buffer named by a map.  The reference is the header's defining equation -- one CPU oracle per receiver,
one demod_iq per buffer, relabelled with the buffer's index in the call (tests/receivers_support.py) -- with tolerance 0,
and every parity test first asserts that ONE shared filter would give a different list for its input.

Two context sizes: max_chunks = 4 (one-launch passes, folded supersets, eight in flight) and max_chunks = 20 (the
smallest whose passes of 17-20 buffers take the three launches and can be ordered on the device, four in flight)."""
import ctypes as C

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS
from tests import signal_support as ss

pytestmark = pytest.mark.gpu
CHUNK = RS.CHUNK
SIZES = [4, 20]
# receivers -> buffers per receiver: 22-25 buffers in all, so that a blocking call is cut into passes on both context
# sizes (6-7 passes of 4; one of 20 -- three launches -- and one of 2-5)
PER = {1: 22, 2: 11, 3: 8, 5: 5}


def quantise(iq):
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def widen(c, b):
    return np.ascontiguousarray(c.u8_table()[b.reshape(-1, 2)])


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


def tables_equal(c, model, n_receivers):
    for r in range(n_receivers):
        assert list(c.receiver_filter_table(r)) == model.table(r), r


def random_maps(n_receivers, lengths, seed):
    r = np.random.default_rng([0xA11, seed])
    return [r.integers(0, n_receivers, size=n).astype(np.uint32) for n in lengths]


def expect_passes(n_receivers, iq, passes, mode=0, before=None):
    """passes: (first buffer, end buffer, map, samples cut off the end).  before: {pass: [receiver or None (all)]}
    flushed in front of it.  -> (per-receiver lists, shared-filter lists, the per-receiver model)"""
    own, shared = RS.Model(n_receivers, mode), RS.Model(n_receivers, mode, shared=True)
    wants, shareds = [], []
    for k, (a, z, m, cut) in enumerate(passes):
        for r in (before or {}).get(k, []):
            own.flush(r)
            shared.flush(r)
        part = iq[a * CHUNK:z * CHUNK - cut]
        wants.append(own.feed(part, m))
        shareds.append(shared.feed(part, m))
    return wants, shareds, own


def pipeline(c, passes, submit, depth, before=None):
    """submit(k, pass) with `depth` passes in flight; the flushes of `before` issued in front of their pass."""
    got = []
    for k, p in enumerate(passes):
        if c.pending() == depth:
            got.append(RS.keys(c.collect(cap=1 << 17)))
        for r in (before or {}).get(k, []):
            c.icao_flush() if r is None else c.icao_flush_receiver(r)
        submit(k, p)
    while c.pending():
        got.append(RS.keys(c.collect(cap=1 << 17)))
    return got


# ------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("n_receivers", [1, 2, 3, 5])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_blocking_host_and_device_forms(hip_lib, oracle_mod, max_chunks, n_receivers):
    """One blocking call longer than max_chunks (cut into passes, the map indexed by the buffer's index in the call),
    from the host and resident, the resident one with a short last buffer."""
    from dump1090_rs_amd import Context
    iq, m = RS.batch(n_receivers, PER[n_receivers])
    want, shared, model = RS.expectations(n_receivers, PER[n_receivers])
    RS.assert_tells_apart(n_receivers, want, shared)
    assert len(m) > max_chunks and len(want) > 2000
    cut = 50001
    (want_cut,), (shared_cut,), model_cut = expect_passes(n_receivers, iq, [(0, len(m), m, cut)])
    RS.assert_tells_apart(n_receivers, want_cut, shared_cut)
    d = on_device(iq)
    with Context(0, max_chunks) as c:
        c.set_receivers(n_receivers)
        assert c.receivers() == n_receivers
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == want
        assert c.stats()["n_chunks"] == len(m)
        tables_equal(c, model, n_receivers)
        c.icao_flush()
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), len(iq) - cut, m, cap=1 << 17)) == want_cut
        tables_equal(c, model_cut, n_receivers)
        # a map of another integer type, and a list, are converted
        c.icao_flush()
        assert RS.keys(c.demod_iq_rx(iq, [int(x) for x in m], cap=1 << 17)) == want
        c.icao_flush()
        assert RS.keys(c.demod_iq_rx(iq, m.astype(np.int64), cap=1 << 17)) == want
        assert int(c._L.adsb_host_replays(c._h)) >= 4


@pytest.mark.parametrize("n_receivers", [2, 5])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_pipeline_full_with_a_map_that_changes_from_pass_to_pass(hip_lib, oracle_mod, max_chunks, n_receivers):
    """Submit / collect at depth 1 and with the pipeline full: nine passes over windows of one resident capture, each
    with a map of its own (a receiver hears a buffer it has heard before: by then it knows the aircraft), the last
    pass ending in a short buffer.  The map is freed as soon as the submit returns."""
    from dump1090_rs_amd import Context
    iq, _ = RS.batch(3, PER[3])
    total = len(iq) // CHUNK
    n = max_chunks if max_chunks <= 16 else 17    # (17: the smallest three-launch pass)
    starts = [(3 * k) % (total - n + 1) for k in range(9)]
    lengths = [n - (k % 3 == 2) for k in range(9)]
    maps = random_maps(n_receivers, lengths, 40 + n_receivers)
    passes = [(a, a + ln, mp, 30001 if k == 8 else 0) for k, (a, ln, mp) in enumerate(zip(starts, lengths, maps))]
    wants, shareds, model = expect_passes(n_receivers, iq, passes)
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    d = on_device(iq)
    with Context(0, max_chunks) as c:
        c.set_receivers(n_receivers)

        def submit(k, p):
            a, z, mp, cut = p
            scratch = mp.copy()
            c.submit_iq_device_rx(d.data_ptr() + 4 * a * CHUNK, (z - a) * CHUNK - cut, scratch)
            scratch[:] = 0xFFFFFFFF   # (copied by the call: what becomes of it afterwards does not matter)

        for depth in (1, c.max_in_flight()):
            c.icao_flush()
            assert pipeline(c, passes, submit, depth) == wants, depth
            tables_equal(c, model, n_receivers)


def isolation_capture(damage=()):
    """Three buffers: a DF17 of aircraft X in buffer 0; in buffers 1 and 2 an address/parity reply of X -- or, with
    `damage`, a DF17 of X with those bits flipped."""
    x = 0x4B1A2C
    clean = synth.df17_frame(x, 0x58B986D0B3BD25)
    later = F.flip(synth.df17_frame(x, 0x99AA5511223344), *damage) if damage else F.ap_frame(4, x, 0x1234567)[:7]
    iq = synth.noise_numpy(3 * CHUNK, seed=4242)
    at = lambda chunk, j: 5 * (chunk * CHUNK + j)   # noqa: E731
    synth.add_bursts(iq, [synth.Burst(at(0, 40000) + 1, 24000, 1, clean), synth.Burst(at(1, 30000) + 2, 24000, 2, later),
                          synth.Burst(at(2, 70000) + 3, 24000, 3, later)])
    emitted = synth.df17_frame(x, 0x99AA5511223344) if damage else later
    return iq, emitted


@pytest.mark.parametrize("max_chunks", SIZES)
def test_isolation_spelled_out(hip_lib, oracle_mod, max_chunks):
    """Receiver A hears a DF17 of X in buffer 0; receiver B gets only an address/parity reply of X in buffer 1; A gets
    one in buffer 2.  B's is not emitted, A's scores 1000 -- and the same IQ through a plain context emits both."""
    from dump1090_rs_amd import Context
    iq, reply = isolation_capture()
    m = np.array([0, 1, 0], dtype=np.uint32)
    (want,), (shared,), model = expect_passes(2, iq, [(0, 3, m, 0)])
    where = lambda ks: sorted({(k[0], k[3]) for k in ks if k[4] == reply})   # noqa: E731
    assert where(want) == [(2, 1000)] and where(shared) == [(1, 1000), (2, 1000)]
    with Context(0, max_chunks) as c:
        plain = RS.keys(c.demod_iq(iq))
        assert where(plain) == [(1, 1000), (2, 1000)] and plain == shared
        c.set_receivers(2)
        got = RS.keys(c.demod_iq_rx(iq, m))
        assert where(got) == [(2, 1000)] and got == want
        tables_equal(c, model, 2)
        # the other way round: B hears X first, then A's reply in buffer 1 is the one that is not emitted
        c.icao_flush()
        assert where(RS.keys(c.demod_iq_rx(iq, 1 - m))) == [(2, 1000)]
        c.icao_flush()
        assert where(RS.keys(c.demod_iq_rx(iq, np.array([0, 0, 1], dtype=np.uint32)))) == [(1, 1000)]


@pytest.mark.parametrize("max_chunks", SIZES)
def test_one_receiver_and_plain_calls_equal_a_plain_context(hip_lib, oracle_mod, max_chunks):
    from dump1090_rs_amd import Context
    iq, _ = RS.batch(3, PER[3])
    want = RS.Model(1).feed(iq, np.zeros(len(iq) // CHUNK, dtype=np.uint32))
    d = on_device(iq)
    zeros = np.zeros(len(iq) // CHUNK, dtype=np.uint32)
    with Context(0, max_chunks) as plain, Context(0, max_chunks) as c:
        ref = RS.keys(plain.demod_iq(iq, cap=1 << 17))
        assert ref == want
        c.set_receivers(1)
        assert RS.keys(c.demod_iq_rx(iq, zeros, cap=1 << 17)) == ref
        c.set_receivers(3)   # (a change of n restarts every receiver from an empty filter)
        assert not c.receiver_filter_table(0).any()
        assert RS.keys(c.demod_iq(iq, cap=1 << 17)) == ref                       # plain calls: every buffer is receiver 0
        assert not c.receiver_filter_table(1).any() and c.receiver_filter_table(0).any()
        c.icao_flush()
        assert RS.keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 17)) == ref
        c.icao_flush()
        n = min(max_chunks, 17) * CHUNK
        c.submit_iq_device(d.data_ptr(), n)
        assert RS.keys(c.collect(cap=1 << 17)) == [k for k in ref if k[0] < n // CHUNK]
        c.set_receivers(0)   # off again: a plain context
        assert c.receivers() == 0
        assert RS.keys(c.demod_iq(iq, cap=1 << 17)) == ref


# ------------------------------------------------------------------------------------------------- flushes
@pytest.mark.parametrize("max_chunks", SIZES)
def test_flush_of_one_receiver_in_a_full_pipeline_and_of_all(hip_lib, oracle_mod, max_chunks):
    """adsb_icao_flush_receiver with the pipeline full: the receiver restarts from an empty filter at the pass submitted
    next, the others are untouched; adsb_icao_flush empties all.  Against oracles flushed at the same buffer."""
    from dump1090_rs_amd import Context
    n_receivers = 3
    iq, _ = RS.batch(3, PER[3])
    total = len(iq) // CHUNK
    n = max_chunks if max_chunks <= 16 else 17
    starts = [(5 * k) % (total - n + 1) for k in range(10)]
    maps = random_maps(n_receivers, [n] * 10, 77)
    passes = [(a, a + n, mp, 0) for a, mp in zip(starts, maps)]
    before = {3: [1], 5: [0, 2], 7: [None], 8: [1, 1]}
    wants, shareds, model = expect_passes(n_receivers, iq, passes, before=before)
    plain, _, _ = expect_passes(n_receivers, iq, passes)
    assert wants != plain and wants[:3] == plain[:3]     # the flushes are visible in the results, from the first one on
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    d = on_device(iq)
    with Context(0, max_chunks) as c:
        c.set_receivers(n_receivers)
        submit = lambda k, p: c.submit_iq_device_rx(d.data_ptr() + 4 * p[0] * CHUNK, (p[1] - p[0]) * CHUNK, p[2])   # noqa: E731
        assert pipeline(c, passes, submit, c.max_in_flight(), before) == wants
        tables_equal(c, model, n_receivers)
        # with nothing in flight a receiver's flush shows at once; adsb_icao_flush empties every receiver
        assert c.receiver_filter_table(2).any()
        c.icao_flush_receiver(2)
        assert not c.receiver_filter_table(2).any() and c.receiver_filter_table(0).any()
        c.icao_flush()
        assert not any(c.receiver_filter_table(r).any() for r in range(n_receivers))
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr() + 4 * passes[0][0] * CHUNK, n * CHUNK, maps[0], cap=1 << 17)) == plain[0]


# ------------------------------------------------------------------------------------------------- the other modes
@pytest.mark.parametrize("max_chunks", SIZES)
def test_cu8_twins_equal_the_cs16_calls_on_the_widened_input(hip_lib, oracle_mod, max_chunks):
    from dump1090_rs_amd import Context
    n_receivers = 3
    iq, m = RS.batch(n_receivers, PER[n_receivers])
    b = quantise(iq)
    d8 = on_device(b)
    with Context(0, max_chunks) as c:
        c.set_receivers(n_receivers)
        wide = widen(c, b)
        (want,), (shared,), model = expect_passes(n_receivers, wide, [(0, len(m), m, 0)])
        RS.assert_tells_apart(n_receivers, want, shared)
        assert len(want) > 1500
        assert RS.keys(c.demod_iq_rx(wide, m, cap=1 << 17)) == want
        c.icao_flush()
        assert RS.keys(c.demod_iq_rx_u8(b, m, cap=1 << 17)) == want
        tables_equal(c, model, n_receivers)
        c.icao_flush()
        assert RS.keys(c.demod_iq_device_rx_u8(d8.data_ptr(), len(b), m, cap=1 << 17)) == want
        c.icao_flush()
        n = min(max_chunks, 17)
        c.submit_iq_device_rx_u8(d8.data_ptr(), n * CHUNK, m[:n])
        first = RS.Model(n_receivers).feed(wide[:n * CHUNK], m[:n])
        assert RS.keys(c.collect(cap=1 << 17)) == first


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_error_correction_consults_the_filter_of_the_trials_own_receiver(hip_lib, oracle_mod, max_chunks, mode):
    from dump1090_rs_amd import Context
    # spelled out: a damaged DF17 of X is repaired for the receiver that has heard X, not for the one that has not
    bits = (40,) if mode == 1 else (40, 77)
    score = 1200 if mode == 1 else 1100
    iso, clean = isolation_capture(damage=bits)
    m3 = np.array([0, 1, 0], dtype=np.uint32)
    (want_iso,), (shared_iso,), _ = expect_passes(2, iso, [(0, 3, m3, 0)], mode=mode)
    # (a damaged frame can be repaired at two neighbouring positions: buffers and scores, each once)
    where = lambda ks: sorted({(k[0], k[3]) for k in ks if k[4] == clean})   # noqa: E731
    assert where(want_iso) == [(2, score)] and where(shared_iso) == [(1, score), (2, score)]
    # ... and a capture of every format with damaged copies in every buffer
    n_receivers = 3
    iq, m = RS.batch(n_receivers, PER[n_receivers], fix=True)
    want, shared, model = RS.expectations(n_receivers, PER[n_receivers], fix=True, mode=mode)
    RS.assert_tells_apart(n_receivers, want, shared)
    assert sum(k[3] == 1200 for k in want) >= 5 * len(m)
    d = on_device(iq)
    with Context(0, max_chunks) as c:
        c.set_receivers(2)
        c.set_error_correction(mode)
        got = RS.keys(c.demod_iq_rx(iso, m3))
        assert where(got) == [(2, score)] and got == want_iso
        c.set_receivers(n_receivers)
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), len(iq), m, cap=1 << 17)) == want
        tables_equal(c, model, n_receivers)


@pytest.mark.parametrize("max_chunks", SIZES)
def test_signal_statistics_on(hip_lib, oracle_mod, max_chunks):
    """Frames byte-equal to the mode off, and one record per buffer equal to the plain restatement."""
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
    n_receivers = 3
    iq, m = RS.batch(n_receivers, PER[n_receivers])
    want, _, _ = RS.expectations(n_receivers, PER[n_receivers])
    records = ss.restated(oracle_mod.Oracle(), iq, iq, SIGNAL_STATS_DTYPE)
    d = on_device(iq)
    with Context(0, max_chunks) as c:
        c.set_receivers(n_receivers)
        c.set_signal_stats(True)
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), len(iq), m, cap=1 << 17)) == want
        got = c.signal_stats()
        assert len(got) == len(m)
        for name in records.dtype.names:
            assert np.array_equal(got[name], records[name]), name
        c.icao_flush()
        n = min(max_chunks, 17)
        c.submit_iq_device_rx(d.data_ptr(), n * CHUNK, m[:n])
        assert RS.keys(c.collect(cap=1 << 17)) == [k for k in want if k[0] < n]
        got = c.signal_stats()
        for name in records.dtype.names:
            assert np.array_equal(got[name], records[name][:n]), name


# ------------------------------------------------------------------------------------------------- the other paths
def test_dense_input_is_never_scored_on_the_device_and_the_pooled_replay_agrees(hip_lib, oracle_mod):
    """The large context on a dense stream (>= 8 records per buffer; from the second pass on the device hands the
    records over in replay order): four passes in flight, every one replayed by the host, per receiver; with the
    threshold of the pooled replay at one record the receivers are dealt to several threads -- the same lists."""
    from dump1090_rs_amd import Context
    n_receivers, n = 4, 20
    iq = F.fill_capture(900, n, per_buffer=60)
    maps = random_maps(n_receivers, [n] * 4, 9)
    passes = [(0, n, mp, 0) for mp in maps]
    wants, shareds, model = expect_passes(n_receivers, iq, passes)
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    d = on_device(iq)
    with Context(0, n) as c:
        c.set_receivers(n_receivers)
        submit = lambda k, p: c.submit_iq_device_rx(d.data_ptr(), n * CHUNK, p[2])   # noqa: E731
        replays = int(c._L.adsb_host_replays(c._h))
        got = []
        for k, p in enumerate(passes):
            submit(k, p)
        for k in range(4):
            got.append(RS.keys(c.collect(cap=1 << 17)))
            assert c.stats()["n_records"] >= 8 * n
            assert int(c._L.adsb_host_replays(c._h)) == replays + k + 1
        assert got == wants
        tables_equal(c, model, n_receivers)
        counters = c.selftest_rx_counters()
        assert counters["rx_passes"] == 4 and counters["pooled_passes"] == 0
        # the same passes again, behind dense ones (the device now hands the records over in replay order), pooled
        c.icao_flush()
        c.selftest_rx_tune(1)
        assert pipeline(c, passes, submit, 4) == wants
        assert int(c._L.adsb_host_replays(c._h)) == replays + 8
        counters = c.selftest_rx_counters()
        assert counters["rx_passes"] == 8 and counters["pooled_passes"] == 4
        tables_equal(c, model, n_receivers)
        c.selftest_rx_tune(0)
        c.icao_flush()
        assert pipeline(c, passes, submit, 4) == wants
        assert c.selftest_rx_counters()["pooled_passes"] == 4


def test_overflow_fallback_goes_buffer_by_buffer_per_receiver(hip_lib, oracle_mod):
    """A periodic stretch inside one receiver's buffer, dense enough to overflow the lists: the pass is redone buffer
    by buffer, each against its receiver's filter, the superset put back from the union of the filters."""
    from dump1090_rs_amd import Context
    from tests.test_gpu_parity import ADVERSARIAL_PERIODS
    n_receivers = 2
    clean, m = RS.batch(n_receivers, 2)
    iq = clean.copy()
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 20000, CHUNK + 95000
    iq[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    iq[a:z, 1] = 0
    passes = [(0, 4, m, 0), (0, 4, m[::-1].copy(), 0)]
    own = RS.Model(n_receivers)
    shared = RS.Model(n_receivers, shared=True)
    want = [own.feed(clean, m), own.feed(iq, passes[1][2])]
    shared_want = [shared.feed(clean, m), shared.feed(iq, passes[1][2])]
    RS.assert_tells_apart(n_receivers, sum(want, []), sum(shared_want, []))
    with Context(0, 4) as c:
        c.set_receivers(n_receivers)
        assert RS.keys(c.demod_iq_rx(clean, m, cap=1 << 17)) == want[0]
        assert c.stats()["retries"] == 0
        assert RS.keys(c.demod_iq_rx(iq, passes[1][2], cap=1 << 17)) == want[1]
        assert c.stats()["retries"] > 0
        assert c.selftest_rx_counters()["union_reseeds"] >= 1
        tables_equal(c, own, n_receivers)


def test_rematch_on_the_small_context_with_two_receivers(hip_lib, oracle_mod):
    """One-buffer passes, eight in flight: receiver A is taught X in one pass and gets an address/parity reply of X in
    its next one, launched while the first was in flight -- that pass is matched again (adsb_host_rematches) behind the
    union superset; receiver B's reply of X, in between, stays out."""
    from dump1090_rs_amd import Context
    x = 0x4B1A2C
    df4 = F.ap_frame(4, x, 0x7654321)[:7]
    df20 = F.ap_frame(20, x, 0x1122334455667788)
    n = 12
    iq = synth.make_iq(n * CHUNK, n_bursts=20 * n, seed=9911, n_icao=12, df11_every=5)
    at = lambda chunk, j: 5 * (chunk * CHUNK + j)   # noqa: E731
    synth.add_bursts(iq, [synth.Burst(at(3, 50000), 22000, 1, df4),                        # A, too early
                          synth.Burst(at(4, 100000) + 2, 22000, 2, synth.df17_frame(x, 7)),  # A learns X
                          synth.Burst(at(5, 300) + 1, 22000, 3, df4),                      # B: never heard X
                          synth.Burst(at(6, 300) + 1, 22000, 3, df4),                      # A: the very next pass of A
                          synth.Burst(at(7, 60000) + 3, 22000, 4, df20),                   # B again
                          synth.Burst(at(8, 1000), 22000, 5, df20)])                       # A
    m = np.array([0, 1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1], dtype=np.uint32)
    passes = [(b, b + 1, m[b:b + 1], 0) for b in range(n)]
    wants, shareds, model = expect_passes(2, iq, passes)
    hits = lambda lists: sorted({b for b, ks in enumerate(lists) for k in ks if k[4] in (df4, df20)})   # noqa: E731
    assert hits(wants) == [6, 8] and hits(shareds) == [5, 6, 7, 8]
    d = on_device(iq)
    with Context(0, 4) as c:
        c.set_receivers(2)
        submit = lambda k, p: c.submit_iq_device_rx(d.data_ptr() + 4 * p[0] * CHUNK, CHUNK, p[2])   # noqa: E731
        assert pipeline(c, passes, submit, 8) == wants
        assert int(c._L.adsb_host_rematches(c._h)) >= 1
        tables_equal(c, model, 2)


@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_the_ring_in_both_formats(hip_lib, oracle_mod, max_chunks, fmt):
    """The aggregator's loop: a slot holds one buffer from each of several receivers, the map goes with the slot."""
    from dump1090_rs_amd import Context
    n_receivers = 5
    iq, _ = RS.batch(3, PER[3])
    total = len(iq) // CHUNK
    n = max_chunks if max_chunks <= 16 else 17
    starts = [(4 * k) % (total - n + 1) for k in range(6)]
    maps = random_maps(n_receivers, [n] * 6, 5)
    passes = [(a, a + n, mp, 20001 if k == 5 else 0) for k, (a, mp) in enumerate(zip(starts, maps))]
    with Context(0, max_chunks) as c:
        c.set_receivers(n_receivers)
        raw = quantise(iq) if fmt == "cu8" else iq
        meant = widen(c, raw) if fmt == "cu8" else iq
        wants, shareds, model = expect_passes(n_receivers, meant, passes)
        RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
        (c.ring_create_u8 if fmt == "cu8" else c.ring_create)(n * CHUNK)

        def submit(k, p):
            a, z, mp, cut = p
            buf = c.ring_acquire_u8() if fmt == "cu8" else c.ring_acquire()
            k_samples = (z - a) * CHUNK - cut
            buf[:k_samples] = raw[a * CHUNK:a * CHUNK + k_samples]
            c.ring_submit_rx(k_samples, mp)

        assert pipeline(c, passes, submit, min(3, c.max_in_flight())) == wants
        tables_equal(c, model, n_receivers)


# ------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("max_chunks", SIZES)
def test_refusals_leave_the_results_unchanged(hip_lib, oracle_mod, max_chunks):
    from dump1090_rs_amd import Context, _lib
    from dump1090_rs_amd._lib import AdsbError
    n_receivers = 2
    iq, m = RS.batch(n_receivers, 2)
    want, shared, model = RS.expectations(n_receivers, 2)
    RS.assert_tells_apart(n_receivers, want, shared)
    d = on_device(iq)
    L = hip_lib

    def refused(status, call):
        with pytest.raises(AdsbError) as e:
            call()
        assert e.value.status == status

    with Context(0, max_chunks) as c:
        h, n_out = c._h, C.c_size_t()
        # receivers off: every _rx call and the two per-receiver calls
        refused(_lib.ADSB_ERR_INVALID, lambda: c.demod_iq_rx(iq, m))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.demod_iq_device_rx(d.data_ptr(), len(iq), m))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.submit_iq_device_rx(d.data_ptr(), len(iq), m))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.demod_iq_rx_u8(quantise(iq), m))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.demod_iq_device_rx_u8(d.data_ptr(), len(iq), m))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.submit_iq_device_rx_u8(d.data_ptr(), len(iq), m))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.icao_flush_receiver(0))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.receiver_filter_table(0))
        c.ring_create(4 * CHUNK)
        c.ring_acquire()
        refused(_lib.ADSB_ERR_INVALID, lambda: c.ring_submit_rx(4 * CHUNK, m))
        assert c.pending() == 0
        # n > ADSB_MAX_RECEIVERS; carry-over in either order
        refused(_lib.ADSB_ERR_INVALID, lambda: c.set_receivers(_lib.ADSB_MAX_RECEIVERS + 1))
        c.set_carry_over(True)
        refused(_lib.ADSB_ERR_INVALID, lambda: c.set_receivers(n_receivers))
        c.set_carry_over(False)
        c.set_receivers(n_receivers)
        refused(_lib.ADSB_ERR_INVALID, lambda: c.set_carry_over(True))
        c.set_carry_over(False)   # (off is what it is: accepted)
        # the results are what they would have been
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == want
        tables_equal(c, model, n_receivers)
        before = [c.receiver_filter_table(r) for r in range(n_receivers)]
        # a map entry out of range or a null map: nothing enqueued, no filter touched
        bad = m.copy()
        bad[-1] = n_receivers
        refused(_lib.ADSB_ERR_INVALID, lambda: c.demod_iq_rx(iq, bad))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.demod_iq_device_rx(d.data_ptr(), len(iq), bad))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.submit_iq_device_rx(d.data_ptr(), len(iq), bad))
        c.ring_acquire()
        refused(_lib.ADSB_ERR_INVALID, lambda: c.ring_submit_rx(4 * CHUNK, bad))
        assert L.adsb_demod_iq_device_rx(h, C.c_void_p(d.data_ptr()), len(iq), None, None, 0, C.byref(n_out)) == -1
        assert L.adsb_submit_iq_device_rx(h, C.c_void_p(d.data_ptr()), len(iq), None) == -1
        assert c.pending() == 0
        refused(_lib.ADSB_ERR_INVALID, lambda: c.icao_flush_receiver(n_receivers))
        refused(_lib.ADSB_ERR_INVALID, lambda: c.receiver_filter_table(n_receivers))
        # the shard calls
        out, cnt = np.zeros(16, dtype=np.uint32), C.c_size_t()
        assert L.adsb_shard_scan(h, C.c_void_p(d.data_ptr()), len(iq), out.ctypes.data, 16, C.byref(cnt)) == _lib.ADSB_ERR_INVALID
        # with a pass pending: adsb_set_receivers and the filter tables are busy
        c.submit_iq_device_rx(d.data_ptr(), len(iq), m)
        refused(_lib.ADSB_ERR_BUSY, lambda: c.set_receivers(3))
        refused(_lib.ADSB_ERR_BUSY, lambda: c.set_receivers(0))
        refused(_lib.ADSB_ERR_BUSY, lambda: c.receiver_filter_table(0))
        assert L.adsb_selftest_rx_tune(h, 1) == _lib.ADSB_ERR_BUSY
        model2 = RS.Model(n_receivers)
        model2.feed(iq, m)
        assert RS.keys(c.collect(cap=1 << 17)) == model2.feed(iq, m)
        for r in range(n_receivers):
            assert np.array_equal(c.receiver_filter_table(r), before[r])   # (the second time nothing new was learned)
        assert c.receivers() == n_receivers


@pytest.mark.parametrize("max_chunks", SIZES)
def test_capacity_from_an_rx_call_then_fetch_messages(hip_lib, oracle_mod, max_chunks):
    from dump1090_rs_amd import _lib, Context
    from dump1090_rs_amd._lib import AdsbMsg
    n_receivers = 2
    iq, m = RS.batch(n_receivers, 2)
    want, _, model = RS.expectations(n_receivers, 2)
    with Context(0, max_chunks) as c:
        c.set_receivers(n_receivers)
        out, n = (AdsbMsg * 7)(), C.c_size_t()
        st = c._L.adsb_demod_iq_rx(c._h, iq.ctypes.data, len(iq), m.ctypes.data, out, 7, C.byref(n))
        assert st == _lib.ADSB_ERR_CAPACITY and n.value == len(want)
        assert [(o.chunk, o.j, o.score) for o in out] == [(k[0], k[1], k[3]) for k in want[:7]]
        full = (AdsbMsg * n.value)()
        assert c._L.adsb_fetch_messages(c._h, full, n.value, C.byref(n)) == 0
        assert [(o.chunk, o.j, o.try_phase, o.score, bytes(o.msg[:o.len])) for o in full] == [k[:5] for k in want]
        tables_equal(c, model, n_receivers)      # the pass was done: the filters have advanced, once

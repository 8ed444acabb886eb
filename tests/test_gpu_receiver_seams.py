"""Receiver seams (include/adsb_hip.h, "Receiver seams") through the device: carry-over with receivers on.  The reference
is the header's defining sentence -- one CPU oracle WITH CARRY-OVER per receiver, one call per buffer, relabelled with the
buffer's index (tests/seam_support.py) -- with tolerance 0, and every test first asserts on the CPU that its planted seam
frames are found with carry and not without.

Two context sizes: max_chunks = 8 (one-launch passes, folded supersets, eight in flight) and max_chunks = 64 (passes of
17 and more buffers take the three launches, four in flight).

Rates are not this file's business: tools/seam_rate.py, profiles/seam_rate.jsonl."""
from functools import lru_cache

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS
from tests import seam_support as S

pytestmark = pytest.mark.gpu
CHUNK, LEAD = S.CHUNK, S.LEAD
SIZES = [8, 64]
THREE_LAUNCH = 17   # the smallest pass that takes the three launches


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


def quantise(iq):
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def seam_context(max_chunks, n_receivers, mode=0):
    from dump1090_rs_amd import Context
    c = Context(0, max_chunks)
    c.set_receivers(n_receivers)
    if mode:
        c.set_error_correction(mode)
    c.set_receiver_carry(True)
    assert c.get_receiver_carry()
    return c


def padded(max_chunks, streams, m, seed=7700):
    """(streams, map) as they are for the small context; for the large one with buffers of noise from one more receiver
    appended, so that the pass takes the three launches.  -> (iq, map, receivers)"""
    streams, m = list(streams), [int(x) for x in m]
    extra = THREE_LAUNCH - len(m) if max_chunks > 16 else 0
    if extra > 0:
        streams.append(synth.noise_numpy(extra * CHUNK, seed))
        m += [len(streams) - 1] * extra
    m = np.array(m, dtype=np.uint32)
    return S.interleave(streams, m), m, len(streams)


def pipeline(c, n_passes, submit, depth, between=None):
    got = []
    for k in range(n_passes):
        if c.pending() == depth:
            got.append(RS.keys(c.collect(cap=1 << 17)))
        if between:
            between(k)
        submit(k)
    while c.pending():
        got.append(RS.keys(c.collect(cap=1 << 17)))
    return got


# ------------------------------------------------------------------------------------------------- 1. the catalogue
@lru_cache(maxsize=None)
def catalogue_case(n_receivers=5, per=4, blocked=False):
    streams, planted = S.catalogue(n_receivers, per)
    m = np.repeat(np.arange(n_receivers, dtype=np.uint32), per) if blocked else S.round_robin(n_receivers, per)
    iq = S.interleave(streams, m)
    (want,), model = S.expect_calls(n_receivers, [(iq, m)])
    (without,), _ = S.expect_calls(n_receivers, [(iq, m)], carry=False)
    # on the CPU: what the input is for
    S.assert_seams_matter(want, without, [f for kind in ("straddle", "inside") for _, f in planted[kind]])
    for _, f in planted["last"]:   # (its preamble is at j = 324, which only a real lead-in reaches; some are found at 325 too)
        assert S.found(want, f)
    assert sum(any(j == LEAD - 2 for _, j, _ in S.found(want, f)) for _, f in planted["last"]) >= len(planted["last"]) - 1
    assert not any(j == LEAD - 2 for _, f in planted["last"] for _, j, _ in S.found(without, f))
    for _, f in planted["edge"]:
        assert not S.found(want, f) and [j for _, j, _ in S.found(without, f)] == [LEAD - 1]
    assert all(len(v) >= n_receivers - 1 for v in planted.values())
    iq.setflags(write=False)
    return iq, m, want, without, model, planted


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_the_seam_catalogue(hip_lib, oracle_mod, max_chunks, blocked):
    """20 buffers of 5 receivers, round robin or every receiver's buffers in a row (the lead-in then comes from the pass's
    own input): one three-launch pass in the large context, a blocking call cut into three passes in the small one."""
    iq, m, want, without, model, planted = catalogue_case(blocked=blocked)
    d = on_device(iq)
    with seam_context(max_chunks, 5) as c:
        got = RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17))
        assert got == want and got != without
        S.tables_equal(c, model, 5)
        k = c.selftest_rx_seam_counters()
        assert k["passes"] == (1 if max_chunks > 16 else 3) and k["records"] > 0 and k["redone"] == 0
        assert k["dropped"] >= len(planted["edge"])      # found at j = 325 by the pass itself, against its zero lead-in
        for _, f in planted["edge"]:
            assert not S.found(got, f)
        for _, f in planted["straddle"] + planted["inside"]:
            assert all(j < LEAD for _, j, _ in S.found(got, f))
        # resident, from empty filters and restarted streams
        c.icao_flush()
        c.receiver_carry_reset()
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), len(iq), m, cap=1 << 17)) == want
        S.tables_equal(c, model, 5)


# ------------------------------------------------------------------------------------------------- 2. the filter across the seam
@lru_cache(maxsize=None)
def filter_case():
    x1, x2, x3, y = 0x4B1A2C, 0x3C6589, 0xA1B2C3, 0x06A0AF
    a = [(CHUNK - 321, synth.df11_frame(x1), 1), (CHUNK - 126, F.ap_frame(4, x1, 0x1234567)[:7], 2),          # learned inside the same seam
         (CHUNK + 40000, synth.df17_frame(x3, 0x58B986D0B3BD25), 3),                                        # learned in the first pass
         (2 * CHUNK - 100, synth.df17_frame(x2, 0x99AA5511223344), 0), (2 * CHUNK + 1000, F.ap_frame(5, x2, 0x7654321)[:7], 4),
         (3 * CHUNK - 150, F.ap_frame(4, y, 0x0F0F0F0)[:7], 1),                                             # known only to B
         (4 * CHUNK - 130, F.ap_frame(20, x3, 0x1122334), 2), (5 * CHUNK - 120, F.ap_frame(20, x3, 0x5566778), 3)]
    b = [(50000, synth.df17_frame(y, 0x2233445566778), 2)]
    frames = [p[1] for p in a]
    return (S.stream(811, 6, a), S.stream(812, 6, b)), frames


@pytest.mark.parametrize("max_chunks", SIZES)
def test_the_filter_across_the_seam(hip_lib, oracle_mod, max_chunks):
    """On receiver A while B sees none of it: an address learned inside the same seam, a seam DF17 that lets a reply at
    j >= 326 of the same buffer through, an address of an earlier pass asked for in a seam (lead-in from the carry, and
    from the pass's own input), and an address only B knows, which must not let A's seam reply through."""
    (sa, sb), fr = filter_case()
    calls = []
    for lo, hi in ((0, 4), (4, 6)):
        iq, m, n = padded(max_chunks, [sa[lo * CHUNK:hi * CHUNK], sb[lo * CHUNK:hi * CHUNK]], [0, 1] * (hi - lo), seed=7700 + lo)
        calls.append((iq, m))
    wants, model = S.expect_calls(n, calls)
    withouts, _ = S.expect_calls(n, calls, carry=False)
    df11, df4, _, df17, df5, df4_y, df20_carry, df20_own = fr
    w0, w1 = wants
    assert [s for _, _, s in S.found(w0, df4)] == [1000] and S.found(w0, df4)[0][1] < LEAD and S.found(w0, df11)[0][1] < 10
    assert S.found(w0, df17)[0][1] < LEAD and [(j >= LEAD, s) for _, j, s in S.found(w0, df5)] == [(True, 1000)]
    assert not S.found(w0, df4_y)
    assert {s for _, _, s in S.found(w1, df20_carry)} == {1000} and {s for _, _, s in S.found(w1, df20_own)} == {1000}
    assert S.found(w1, df20_carry)[0][0] == 0 and S.found(w1, df20_own)[0][0] == 2
    for f in (df11, df4, df17, df5, df20_carry, df20_own):
        assert not S.found(withouts[0] + withouts[1], f), f.hex()
    with seam_context(max_chunks, n) as c:
        for (iq, m), want in zip(calls, wants):
            assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == want
        S.tables_equal(c, model, n)
        assert c.receiver_filter_table(1).any() and c.selftest_rx_seam_counters()["records"] >= 6


# ------------------------------------------------------------------------------------------------- 3. every entry point
@lru_cache(maxsize=None)
def long_case():
    """70 buffers of 5 receivers, round robin, the catalogue at every seam."""
    streams, planted = S.catalogue(5, 14, seed=930)
    m = S.round_robin(5, 14)
    iq = S.interleave(streams, m)
    iq.setflags(write=False)
    return iq, m, planted


def pass_bounds(max_chunks, total):
    n = 7 if max_chunks <= 16 else THREE_LAUNCH
    cuts = list(range(0, total - n + 1, n))
    return [(a, (a + n if k + 1 < len(cuts) else total)) for k, a in enumerate(cuts)]


@pytest.mark.parametrize("max_chunks", SIZES)
def test_submit_collect_ring_and_a_blocking_call_cut_into_passes(hip_lib, oracle_mod, max_chunks):
    iq, m, planted = long_case()
    bounds = pass_bounds(max_chunks, len(m))
    assert len(bounds) >= 4 and bounds[-1][1] - bounds[-1][0] <= max_chunks
    calls = [(iq[a * CHUNK:z * CHUNK], m[a:z]) for a, z in bounds]
    wants, model = S.expect_calls(5, calls)
    withouts, _ = S.expect_calls(5, calls, carry=False)
    seam = [f for kind in ("straddle", "inside") for _, f in planted[kind]]
    S.assert_seams_matter(sum(wants, []), sum(withouts, []), seam)
    (whole,), model_whole = S.expect_calls(5, [(iq, m)])
    d = on_device(iq)
    with seam_context(max_chunks, 5) as c:
        depth = c.max_in_flight()
        assert depth >= 4
        submit = lambda k: c.submit_iq_device_rx(d.data_ptr() + 4 * bounds[k][0] * CHUNK, len(calls[k][0]), calls[k][1])   # noqa: E731
        assert pipeline(c, len(calls), submit, min(depth, len(calls))) == wants
        S.tables_equal(c, model, 5)
        # the ring, full as well
        c.icao_flush()
        c.receiver_carry_reset()
        c.ring_create(max(len(x[0]) for x in calls))

        def ring_submit(k):
            buf = c.ring_acquire()
            buf[:len(calls[k][0])] = calls[k][0]
            c.ring_submit_rx(len(calls[k][0]), calls[k][1])

        assert pipeline(c, len(calls), ring_submit, min(depth, len(calls))) == wants
        S.tables_equal(c, model, 5)
        # one blocking call over all 70 buffers: cut into passes of max_chunks
        c.icao_flush()
        c.receiver_carry_reset()
        assert RS.keys(c.demod_iq_device_rx(d.data_ptr(), len(iq), m, cap=1 << 17)) == whole
        S.tables_equal(c, model_whole, 5)
        assert c.selftest_rx_seam_counters()["redone"] == 0


@pytest.mark.parametrize("max_chunks", SIZES)
def test_cu8_twins_and_formats_alternating_on_one_receiver(hip_lib, oracle_mod, max_chunks):
    """The _u8 twins on the quantised catalogue, and then CS16 and CU8 calls in turn: a receiver's carry is CS16 whatever
    format its previous buffer came in."""
    iq, m, *_ = catalogue_case()
    b = quantise(iq)
    d8 = on_device(b)
    with seam_context(max_chunks, 5) as c:
        wide = np.ascontiguousarray(c.u8_table()[b.reshape(-1, 2)])
        (want,), model = S.expect_calls(5, [(wide, m)])
        (without,), _ = S.expect_calls(5, [(wide, m)], carry=False)
        assert want != without and sum(k[1] < LEAD for k in want) >= 8
        assert RS.keys(c.demod_iq_rx_u8(b, m, cap=1 << 17)) == want
        S.tables_equal(c, model, 5)
        c.icao_flush()
        c.receiver_carry_reset()
        assert RS.keys(c.demod_iq_device_rx_u8(d8.data_ptr(), len(b), m, cap=1 << 17)) == want
        # five buffers a call (one of every receiver), CS16 and CU8 in turn
        c.icao_flush()
        c.receiver_carry_reset()
        calls = [(wide[a * CHUNK:(a + 5) * CHUNK], m[a:a + 5]) for a in range(0, 20, 5)]
        wants, model = S.expect_calls(5, calls)
        for k, (part, mp) in enumerate(calls):
            got = c.demod_iq_rx(part, mp) if k % 2 == 0 else c.demod_iq_rx_u8(b[5 * k * CHUNK:5 * (k + 1) * CHUNK], mp)
            assert RS.keys(got) == wants[k], k
        S.tables_equal(c, model, 5)


@pytest.mark.parametrize("short", [100, 327])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_a_short_last_buffer_followed_by_more_of_that_receiver(hip_lib, oracle_mod, max_chunks, short):
    """Receiver 0's stream is cut at CHUNK, CHUNK + short, 2 CHUNK + short, ...: the short buffer is the last of its call,
    and a DF17 that begins 50 samples before it straddles all three pieces."""
    x = synth.df17_frame(0x4840D6, 0x58C382D690C8AC)
    y = synth.df17_frame(0x4840D7, 0x58C382D690C8AD)
    s0 = S.stream(841, 3, [(CHUNK - 50, x, 2), (2 * CHUNK + short - 90, y, 3)])
    s1 = S.stream(842, 3, [(CHUNK - 100, synth.df17_frame(0x4840D8, 0x58C382D690C8AE), 1)])
    cuts = [0, CHUNK, CHUNK + short, 2 * CHUNK + short, 3 * CHUNK]
    p0 = [s0[a:z] for a, z in zip(cuts, cuts[1:])]
    p1 = [s1[k * CHUNK:(k + 1) * CHUNK] for k in range(3)]
    calls = [(np.concatenate([p0[0], p1[0], p0[1]]), [0, 1, 0]), (np.concatenate([p0[2], p1[1]]), [0, 1]),
             (np.concatenate([p1[2], p0[3]]), [1, 0])]
    calls = [(np.ascontiguousarray(iq), np.array(m, dtype=np.uint32)) for iq, m in calls]
    wants, model = S.expect_calls(2, calls)
    withouts, _ = S.expect_calls(2, calls, carry=False)
    S.assert_seams_matter(sum(wants, []), sum(withouts, []), [x, y])
    # (100 samples: the short buffer's positions end before the frame, the next call's first buffer finds it; 327: the
    # short buffer itself does, at j = 275)
    at = S.found(wants[1] if short == 100 else wants[0], x)
    assert at and at[0][0] == (0 if short == 100 else 2) and at[0][1] < LEAD
    assert S.found(wants[2], y)[0][:2][0] == 1 and S.found(wants[2], y)[0][1] < LEAD
    with seam_context(max_chunks, 2) as c:
        for k, ((iq, m), want) in enumerate(zip(calls, wants)):
            assert RS.keys(c.demod_iq_rx(iq, m)) == want, k
        S.tables_equal(c, model, 2)


# ------------------------------------------------------------------------------------------------- 4. one receiver, the plain calls
@pytest.mark.parametrize("max_chunks", SIZES)
def test_one_receiver_fed_by_the_plain_calls_equals_carry_over(hip_lib, oracle_mod, max_chunks):
    from dump1090_rs_amd import Context
    streams, planted = S.catalogue(1, 7, seed=950)
    iq = streams[0]
    pieces = [(0, 1), (1, 3), (3, 4), (4, 7)]
    calls = [(iq[a * CHUNK:z * CHUNK], np.zeros(z - a, dtype=np.uint32)) for a, z in pieces]
    wants, model = S.expect_calls(1, calls)
    withouts, _ = S.expect_calls(1, calls, carry=False)
    S.assert_seams_matter(sum(wants, []), sum(withouts, []), [f for kind in ("straddle", "inside") for _, f in planted[kind]])
    d = on_device(iq)
    with seam_context(max_chunks, 1) as c, Context(0, max_chunks) as plain:
        plain.set_carry_over(True)
        for k, ((part, _), want) in enumerate(zip(calls, wants)):
            a = pieces[k][0]
            got = c.demod_iq(part) if k % 2 == 0 else c.demod_iq_device(d.data_ptr() + 4 * a * CHUNK, len(part))
            ref = plain.demod_iq(part)
            assert RS.keys(got) == want and RS.keys(ref) == want, k
        S.tables_equal(c, model, 1)


# ------------------------------------------------------------------------------------------------- 5. both repair modes
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_repair_across_a_seam(hip_lib, oracle_mod, max_chunks, mode):
    """A one-bit and a two-bit damaged DF17 of an aircraft receiver 0 has heard, each across the end of one of its
    buffers; receiver 1 gets the same damaged frames without ever having heard it."""
    x = 0x4B1A2C
    clean = synth.df17_frame(x, 0x58B986D0B3BD25)
    one, two = synth.df17_frame(x, 0x99AA5511223344), synth.df17_frame(x, 0x99AA5511223355)
    damaged = [(CHUNK - 100, F.flip(one, 40), 1), (2 * CHUNK - 200, F.flip(two, 40, 77), 2)]
    s0 = S.stream(861, 3, [(30000, clean, 3)] + damaged)
    s1 = S.stream(862, 3, damaged)
    iq, m, n = padded(max_chunks, [s0, s1], [0, 1] * 3)
    (want,), model = S.expect_calls(n, [(iq, m)], mode=mode)
    (without,), _ = S.expect_calls(n, [(iq, m)], mode=mode, carry=False)
    where = lambda ks, f: sorted({(k[0], k[3]) for k in ks if k[4] == f})   # noqa: E731
    assert where(want, one) == [(2, 1200)] and where(without, one) == []
    assert where(want, two) == ([(4, 1100)] if mode == 3 else []) and where(without, two) == []
    with seam_context(max_chunks, n, mode) as c:
        got = RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17))
        assert got == want
        S.tables_equal(c, model, n)


# ------------------------------------------------------------------------------------------------- 6. a receiver that reconnected
@pytest.mark.parametrize("who", [2, None])
@pytest.mark.parametrize("max_chunks", SIZES)
def test_carry_reset_with_passes_in_flight(hip_lib, oracle_mod, max_chunks, who):
    """adsb_receiver_carry_reset(r) between two submissions, the pipeline full: r's next buffer behaves as a first
    buffer, the others' do not; ADSB_RX_ALL restarts every receiver."""
    iq, m, planted = long_case()
    bounds = pass_bounds(max_chunks, len(m))[:4]
    calls = [(iq[a * CHUNK:z * CHUNK], m[a:z]) for a, z in bounds]
    before = {2: [("reset", who)]}
    wants, model = S.expect_calls(5, calls, before=before)
    plain, _ = S.expect_calls(5, calls)
    assert wants[:2] == plain[:2] and wants[2] != plain[2]
    changed = set(plain[2]) ^ set(wants[2])   # (frames lost, and a frame at j = 325 that only a zero lead-in finds)
    assert changed and all(k[1] < LEAD for k in changed)
    if who is not None:   # the others' seams of that pass are still found
        assert any(k[1] < LEAD and int(calls[2][1][k[0]]) != who for k in wants[2])
        assert all(int(calls[2][1][k[0]]) == who for k in changed)
    d = on_device(iq)
    with seam_context(max_chunks, 5) as c:
        submit = lambda k: c.submit_iq_device_rx(d.data_ptr() + 4 * bounds[k][0] * CHUNK, len(calls[k][0]), calls[k][1])   # noqa: E731
        between = lambda k: (c.receiver_carry_reset() if who is None else c.receiver_carry_reset(who)) if k == 2 else None   # noqa: E731
        assert pipeline(c, 4, submit, 4, between) == wants
        S.tables_equal(c, model, 5)


# ------------------------------------------------------------------------------------------------- 7. overflow
@pytest.mark.parametrize("max_chunks", SIZES)
def test_a_full_seam_list_is_redone_in_pieces(hip_lib, oracle_mod, max_chunks):
    iq, m, want, without, model, planted = catalogue_case()
    with seam_context(max_chunks, 5) as c:
        c.selftest_rx_seam_tune(4)
        got = RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17))
        k = c.selftest_rx_seam_counters()
        assert k["redone"] > 0 and got == want
        S.tables_equal(c, model, 5)
        c.selftest_rx_seam_tune(0)
        c.icao_flush()
        c.receiver_carry_reset()
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == want
        assert c.selftest_rx_seam_counters()["redone"] == k["redone"]


def test_the_list_overflow_fallback_of_the_pass_itself(hip_lib, oracle_mod):
    """The dense input of tests/test_gpu_edges.py (a periodic stretch that overflows a one-buffer context's lists) with the
    mode on: the pass goes buffer by buffer through the reference-shaped kernel, the seam's records join each buffer."""
    from tests import edges_support as E
    from tests.test_gpu_parity import ADVERSARIAL_PERIODS
    cat = E.iq_stream("planted")
    iq = np.concatenate([cat, cat, cat])
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 66000, 2 * CHUNK + 500   # (across the end of the second buffer: the seam of the third is dense too)
    iq[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    iq[a:z, 1] = 0
    x = synth.df17_frame(0x4840D6, 0x58C382D690C8AC)
    synth.add_bursts(iq, [synth.Burst(5 * (CHUNK - 100) + 2, 26000, 3, x)])
    m = np.zeros(3, dtype=np.uint32)
    (want,), model = S.expect_calls(1, [(iq, m)])
    (without,), _ = S.expect_calls(1, [(iq, m)], carry=False)
    S.assert_seams_matter(want, without, [x])
    with seam_context(1, 1) as c:
        got = RS.keys(c.demod_iq_rx(iq, m, cap=1 << 20))
        assert c.stats()["retries"] > 0 and got == want
        S.tables_equal(c, model, 1)


def test_the_fallback_behind_a_flush_still_knows_what_the_seam_learned(hip_lib, oracle_mod):
    """The overflowing pass holds a DF17 across its buffer's start -- validated only in the seam -- and a reply to it at
    j >= 326 of the same buffer; an icao_flush and another pass are submitted before it is collected, so the fallback
    matches against a bitmap the first seam scan never wrote into."""
    from tests.test_gpu_parity import ADVERSARIAL_PERIODS
    x = 0x4840D6
    df17, df4 = synth.df17_frame(x, 0x58C382D690C8AC), F.ap_frame(4, x, 0x1234567)[:7]
    iq = S.stream(871, 3, [(CHUNK - 100, df17, 2), (CHUNK + 1000, df4, 3)])
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 66000, 2 * CHUNK - 1000
    iq[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    iq[a:z, 1] = 0
    one = np.zeros(1, dtype=np.uint32)
    calls = [(iq[k * CHUNK:(k + 1) * CHUNK], one) for k in range(3)]
    wants, model = S.expect_calls(1, calls, before={2: [("flush", None)]})
    withouts, _ = S.expect_calls(1, calls, carry=False, before={2: [("flush", None)]})
    assert S.found(wants[1], df17)[0][1] < LEAD and {(j >= LEAD, s) for _, j, s in S.found(wants[1], df4)} == {(True, 1000)}
    assert not S.found(withouts[1], df17) and not S.found(withouts[1], df4)
    d = on_device(iq)
    with seam_context(1, 1) as c:
        got, retries = [], 0
        for k in range(3):
            if k == 2:
                c.icao_flush()
            c.submit_iq_device_rx(d.data_ptr() + 4 * k * CHUNK, CHUNK, one)
        while c.pending():
            got.append(RS.keys(c.collect(cap=1 << 20)))
            retries += c.stats()["retries"]
        assert retries > 0 and got == wants
        S.tables_equal(c, model, 1)


# ------------------------------------------------------------------------------------------------- 8. many receivers
def test_forty_receivers_two_rounds(hip_lib, oracle_mod):
    n = 40
    streams = [S.stream(1000 + r, 2, [(CHUNK - 40 - 7 * r, synth.df17_frame(S.aircraft(r, 0), 0x58B986D0B3BD25 + r), r % 5)])
               for r in range(n)]
    m = np.arange(n, dtype=np.uint32)
    calls = [(S.interleave([s[k * CHUNK:(k + 1) * CHUNK] for s in streams], m), m) for k in range(2)]
    wants, model = S.expect_calls(n, calls)
    withouts, _ = S.expect_calls(n, calls, carry=False)
    frames = [synth.df17_frame(S.aircraft(r, 0), 0x58B986D0B3BD25 + r) for r in range(n)]
    S.assert_seams_matter(wants[1], withouts[1], frames)
    with seam_context(64, n) as c:
        for (iq, mp), want in zip(calls, wants):
            assert RS.keys(c.demod_iq_rx(iq, mp, cap=1 << 17)) == want
        S.tables_equal(c, model, n)
        assert c.selftest_rx_seam_counters()["records"] >= n


# ------------------------------------------------------------------------------------------------- 9. mode off
@pytest.mark.parametrize("max_chunks", SIZES)
def test_mode_off_is_the_behaviour_it_was_and_the_refusals(hip_lib, oracle_mod, max_chunks):
    from dump1090_rs_amd import Context, _lib
    from dump1090_rs_amd.context import AdsbError
    iq, m, want, without, *_ = catalogue_case()
    d = on_device(iq)

    def status(call):
        try:
            call()
        except AdsbError as e:
            return e.status
        return _lib.ADSB_OK

    with Context(0, max_chunks) as c:
        assert not c.get_receiver_carry()
        assert status(lambda: c.set_receiver_carry(True)) == _lib.ADSB_ERR_INVALID      # receivers off
        assert status(lambda: c.receiver_carry_reset(0)) == _lib.ADSB_ERR_INVALID
        c.set_receivers(5)
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == without                    # off: every buffer from a zero lead-in
        assert c.selftest_rx_seam_counters() == {"passes": 0, "records": 0, "dropped": 0, "redone": 0}
        assert status(lambda: c.receiver_carry_reset(0)) == _lib.ADSB_ERR_INVALID       # the mode is off
        assert status(lambda: c.set_carry_over(True)) == _lib.ADSB_ERR_INVALID          # as it always was
        # both orders against adsb_set_receiver_scoring
        c.set_receiver_scoring(True)
        assert status(lambda: c.set_receiver_carry(True)) == _lib.ADSB_ERR_INVALID
        c.set_receiver_scoring(False)
        c.set_receiver_carry(True)
        assert status(lambda: c.set_receiver_scoring(True)) == _lib.ADSB_ERR_INVALID
        assert status(lambda: c.set_carry_over(True)) == _lib.ADSB_ERR_INVALID
        assert status(lambda: c.receiver_carry_reset(5)) == _lib.ADSB_ERR_INVALID       # r >= n
        # busy while passes are pending; the reset never is
        c.icao_flush()
        n = min(max_chunks, 20)
        c.submit_iq_device_rx(d.data_ptr(), n * CHUNK, m[:n])
        assert status(lambda: c.set_receiver_carry(False)) == _lib.ADSB_ERR_BUSY
        c.receiver_carry_reset(1)
        c.receiver_carry_reset()
        (first,), _ = S.expect_calls(5, [(iq[:n * CHUNK], m[:n])])
        assert RS.keys(c.collect(cap=1 << 17)) == first
        # off again, and adsb_set_receivers(0) turns it off
        c.set_receiver_carry(False)
        c.icao_flush()
        before = c.selftest_rx_seam_counters()
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == without
        assert c.selftest_rx_seam_counters() == before
        c.set_receiver_carry(True)
        c.set_receivers(0)
        assert not c.get_receiver_carry()
        c.set_receivers(3)
        assert not c.get_receiver_carry()
        # a change of the number of receivers with the mode on restarts every stream
        c.set_receiver_carry(True)
        half = 10 * CHUNK
        c.demod_iq_rx(iq[:half], m[:10] % 3, cap=1 << 17)
        c.set_receivers(5)
        assert c.get_receiver_carry()
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == want

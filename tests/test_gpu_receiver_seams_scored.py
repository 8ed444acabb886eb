"""Receiver seams scored on the device (include/adsb_hip.h, "Receiver seams, scored on the device";
adsb_set_receiver_carry_scoring): dense passes of a large context whose buffers belong to several receivers, each with
carry-over and a filter of its own, take their result from the device -- the seam records merged into the ordered hits by
adsb_seam_score.hip, the merged pass scored by the keyed kernels.  Every list is compared with tests/seam_support.py's
SeamModel (one CPU oracle with carry-over per receiver) at tolerance 0, every filter table slot for slot, and every parity
test first asserts on the CPU that its planted seam frames are found with carry and not without, that one shared filter
would give a different list, and that every judged pass holds at least 8 records per buffer.

The shape is tests/test_gpu_receivers_scored.py's: Context(0, 20), passes of 20 buffers, four in flight, primed into dense
mode by one blocking dense pass and a flush (that pass is the host's: the first judged pass rebuilds the keyed set once).
Every judged pass is asserted to have been taken from the device -- "taken" and "merged_passes" advance, "refused" and
adsb_host_replays do not -- unless the case is about a refusal."""
from functools import lru_cache

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS
from tests import seam_support as S
from tests import seam_scored_support as SS

pytestmark = pytest.mark.gpu
CHUNK, LEAD, N = SS.CHUNK, SS.LEAD, SS.N


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


def quantise(iq):
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def soapy_widen(b):
    """the CS16 samples a context's default table (T_soapy) makes of CU8 bytes"""
    t = ((np.arange(256, dtype=np.float32) - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)
    return np.ascontiguousarray(t[b.reshape(-1, 2)])


def random_maps(n_receivers, lengths, seed):
    r = np.random.default_rng([0x5EA3, seed])
    return [r.integers(0, n_receivers, size=n).astype(np.uint32) for n in lengths]


def replays(c):
    return int(c._L.adsb_host_replays(c._h))


ZERO = {"taken": 0, "refused": 0, "rebuilds": 0, "no_room": 0, "replays": 0, "merged_passes": 0, "unscored": 0}


class Combined:
    """A Context(0, 20) with receivers on and `mode` of ("both", "carry", "scoring", "neither"), primed into dense mode by
    one blocking dense pass; filters flushed and every receiver's stream restarted afterwards.  since(): what the counters
    have moved by since then (or the last mark())."""

    def __init__(self, n_receivers, fix=0, mode="both", max_chunks=N):
        from dump1090_rs_amd import Context
        self.c = Context(0, max_chunks)
        self.n_receivers = n_receivers

        def opened():
            c = self.c
            c.set_receivers(n_receivers)
            if fix:
                c.set_error_correction(fix)
            if mode == "both":
                c.set_receiver_carry_scoring(True)
                assert c.get_receiver_carry_scoring() and c.get_receiver_carry() and c.get_receiver_scoring()
            elif mode == "carry":
                c.set_receiver_carry(True)
            elif mode == "scoring":
                c.set_receiver_scoring(True)
            if max_chunks > 16:
                d = on_device(SS.dense())
                c.demod_iq_device_rx(d.data_ptr(), N * CHUNK, np.zeros(N, dtype=np.uint32), cap=1 << 17)
                assert c.stats()["n_records"] >= 8 * N
                c.icao_flush()
                if mode in ("both", "carry"):
                    c.receiver_carry_reset()
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

    def now(self):
        c = self.c
        return dict(c.selftest_rx_score_counters(), replays=replays(c), **c.selftest_rx_seam_score_counters(),
                    redone=c.selftest_rx_seam_counters()["redone"], host_seam_records=c.selftest_rx_seam_counters()["records"])

    def mark(self):
        self.base = self.now()

    def since(self):
        now = self.now()
        return {k: now[k] - self.base[k] for k in now}

    def since_core(self):
        s = self.since()
        return {k: s[k] for k in ZERO}


def collect_dense(c, n=N):
    got = RS.keys(c.collect(cap=1 << 17))
    assert c.stats()["n_records"] >= 8 * n
    return got


def run_pipeline(c, n_passes, submit, depth=4, between=None):
    got = []
    for k in range(n_passes):
        if c.pending() == depth:
            got.append(collect_dense(c))
        if between:
            between(k)
        submit(k)
    while c.pending():
        got.append(collect_dense(c))
    return got


def all_taken(s, n, rebuilds=1):
    """every one of n judged passes came from the device, merged there; nothing was refused or replayed"""
    since = s.since()
    assert since_core(since) == dict(ZERO, taken=n, rebuilds=rebuilds, merged_passes=n), since
    assert since["seam_records"] > 0 and since["redone"] == 0 and since["host_seam_records"] == 0, since
    return since


def since_core(since):
    return {k: since[k] for k in ZERO}


# ------------------------------------------------------------------------------------------------- 1. parity
@lru_cache(maxsize=None)
def parity_case(fmt):
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 9)
    raw, planted = SS.seam_passes(maps)
    if fmt == "cu8":
        raw = [quantise(x) for x in raw]
    meant = [soapy_widen(x) for x in raw] if fmt == "cu8" else raw
    calls = [(iq, m) for iq, m in zip(meant, maps)]
    wants, withouts, shareds, model = SS.expect(n_receivers, calls)
    SS.assert_input_is_for_this(n_receivers, calls, wants, withouts, shareds, SS.seam_frames_of(planted))
    again = [model.feed(iq, m) for iq, m in calls]   # once more without a flush: the model has moved on
    assert again != wants and all(len(a) >= 8 * N for a in again)
    return n_receivers, maps, raw, wants, again, model, planted


@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
def test_parity_with_the_pipeline_full(hip_lib, oracle_mod, fmt):
    """Four receivers, four passes of 20 buffers with a different random map each and a planted frame at every third seam,
    submitted four deep: the lists and every filter table equal the model's, every pass is taken from the device with its
    seam records merged there.  A second round without a flush shows different scores and rebuilds nothing."""
    n_receivers, maps, raw, wants, again, model, planted = parity_case(fmt)
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers) as s:
        c = s.c
        call = c.submit_iq_device_rx_u8 if fmt == "cu8" else c.submit_iq_device_rx
        for d, m in zip(devs, maps):
            call(d.data_ptr(), N * CHUNK, m)
        assert c.pending() == 4
        got = [collect_dense(c) for _ in maps]
        assert got == wants
        since = all_taken(s, 4)
        if planted["edge"]:   # found at j = 325 by the pass itself against its zero lead-in: dropped on the device
            assert since["dropped"] >= 1
        assert run_pipeline(c, 4, lambda k: call(devs[k].data_ptr(), N * CHUNK, maps[k])) == again
        S.tables_equal(c, model, n_receivers)
        all_taken(s, 8)


# ------------------------------------------------------------------------------------------------- 2. order across the seam
X = 0x4B1A2C
DF17_X = synth.df17_frame(X, 0x58B986D0B3BD25)
REPLY_X = F.ap_frame(4, X, 0x1234567)[:7]
A, B = 0, 1


def map_ab(**receiver_of):
    """every buffer receiver 2 or 3 (bystanders), but for the named ones: map_ab(b3=A, b5=B)"""
    m = np.array([2 + b % 2 for b in range(N)], dtype=np.uint32)
    for name, r in receiver_of.items():
        m[int(name[1:])] = r
    return m


def quiet(iq, b, j, k=0):
    a = b * CHUNK + j
    iq[a - 100:a + 500] = synth.noise_numpy(600, seed=4242 + k)
    return a


def where(ks, frame):
    """(buffer, found across the seam, score) of every emission of `frame`; a frame that adds its address (DF17, DF11) is
    told by its place alone, score None: a later trial phase of the same position finds the address its first one added"""
    adder = frame[0] >> 3 in (11, 17)
    return sorted({(k[0], k[1] < LEAD, None if adder else k[3]) for k in ks if k[4] == frame})


@lru_cache(maxsize=None)
def order_case(which):
    """-> (iq, map, {frame: where the model emits it}, what must NOT be emitted)"""
    iq = SS.dense().copy()
    if which == "a":   # a seam DF17 of X, then X's reply later in the same buffer
        m = map_ab(b3=A, b7=A)
        SS.plant(iq, 3, iq, 7, -100, DF17_X)
        a = quiet(iq, 7, 40000)
        synth.add_bursts(iq, [synth.Burst(5 * a + 1, 24000, 2, REPLY_X)])
        expect_where = {DF17_X: [(7, True, None)], REPLY_X: [(7, False, 1000)]}
    elif which == "b":   # an own DF17 in A's buffer 3 makes a seam reply of its buffer 7 valid
        m = map_ab(b3=A, b7=A)
        a = quiet(iq, 3, 40000)
        synth.add_bursts(iq, [synth.Burst(5 * a + 1, 24000, 2, DF17_X)])
        SS.plant(iq, 3, iq, 7, -100, REPLY_X)
        expect_where = {DF17_X: [(3, False, None)], REPLY_X: [(7, True, 1000)]}
    elif which == "c":   # the same address through B's buffers does not
        m = map_ab(b3=B, b5=A, b7=A)
        a = quiet(iq, 3, 40000)
        synth.add_bursts(iq, [synth.Burst(5 * a + 1, 24000, 2, DF17_X)])
        SS.plant(iq, 5, iq, 7, -100, REPLY_X)
        expect_where = {DF17_X: [(3, False, None)], REPLY_X: []}
    elif which == "d":   # the edge plant: the pass's own hit at j = 325 is dropped, its address never learned
        m = map_ab(b3=A, b7=A)
        SS.plant(iq, 3, iq, 7, 0, DF17_X, loud=True)
        expect_where = {DF17_X: []}
    else:                # e: one seam position whose frame is a record at two or more trial phases
        m = map_ab(b3=A, b7=A)
        SS.plant(iq, 3, iq, 7, -100, DF17_X, tick=2, amplitude=28500)
        expect_where = {DF17_X: [(7, True, None)]}
    calls = [(iq, m)]
    wants, withouts, shareds, model = SS.expect(4, calls)
    assert len(wants[0]) >= 8 * N
    for f, w in expect_where.items():
        assert where(wants[0], f) == w, (which, f.hex(), where(wants[0], f))
    if which == "c":
        assert where(shareds[0], REPLY_X) == [(7, True, 1000)]        # one shared filter would let it through
    elif which == "d":
        assert [(b, j) for b, j, _ in S.found(withouts[0], DF17_X)] == [(7, LEAD - 1)]   # a zero lead-in finds it at 325
        assert X not in model.table(A)
    else:
        assert wants[0] != withouts[0]
    if which == "e":
        # The seam trials of buffer 7 restated on the CPU: a trial at seam position j reads data[j .. j + 290] of (the last
        # 326 samples of A's buffer 3 ++ buffer 7), which is what a buffer that BEGINS with those 326 samples holds at
        # j + 326 behind its own zero lead-in.  The frame is sliced clean -- a self-validating record -- at two or more of
        # the five trial phases of ONE position; X is unknown before, so the first of them scores 1400 and adds X, the
        # second finds it and scores 1800, strictly more: the message emitted is the second record of the group, at 1800,
        # which no scoring of the group's records one by one, or of one of them alone, gives.
        from oracle import binding
        window = np.ascontiguousarray(np.concatenate([iq[4 * CHUNK - LEAD:4 * CHUNK], iq[7 * CHUNK:7 * CHUNK + 2000]]))
        trials = binding.all_trials(window)[1]
        (emitted,) = [k for k in wants[0] if k[4] == DF17_X]
        phases = [int(t["j_tp"]) >> 24 for t in trials if (int(t["j_tp"]) & 0xFFFFFF) == emitted[1] + LEAD and bytes(t["msg"]) == DF17_X]
        assert len(phases) >= 2 and phases == sorted(phases), phases
        assert emitted[1] < LEAD and emitted[3] == 1800 and emitted[2] == phases[1], (emitted[:4], phases)
        assert not [k for k in wants[0] if k[4][1:4] == DF17_X[1:4] and k[:2] < emitted[:2]]   # nothing of X in front of it
    return iq, m, wants[0], model


@pytest.mark.parametrize("which", ["a", "b", "c", "d", "e"])
def test_order_across_the_seam(hip_lib, oracle_mod, which):
    iq, m, want, model = order_case(which)
    d = on_device(iq)
    with Combined(4) as s:
        c = s.c
        c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, m)
        assert collect_dense(c) == want
        S.tables_equal(c, model, 4)
        since = s.since()
        assert since_core(since) == dict(ZERO, taken=1, rebuilds=1, merged_passes=1), since
        if which == "d":
            assert since["dropped"] >= 1 and X not in list(c.receiver_filter_table(A))
        else:
            assert since["seam_records"] >= 1


# ------------------------------------------------------------------------------------------------- 3. consecutive buffers, formats alternating
@lru_cache(maxsize=None)
def consecutive_case():
    """Receiver 0 has runs of consecutive buffers inside each pass and across the passes; passes alternate CS16 / CU8."""
    n_receivers = 3
    base = np.array([0, 0, 0, 1, 0, 0, 2, 2, 1, 0, 0, 0, 0, 1, 2, 0, 0, 1, 0, 0], dtype=np.uint32)
    maps = [base, base[::-1].copy(), base, base[::-1].copy()]
    raw, planted = SS.seam_passes(maps, seed=901, every=2)
    fmts = ["cs16", "cu8", "cs16", "cu8"]
    raw = [quantise(x) if f == "cu8" else x for x, f in zip(raw, fmts)]
    meant = [soapy_widen(x) if f == "cu8" else x for x, f in zip(raw, fmts)]
    calls = list(zip(meant, maps))
    wants, withouts, shareds, model = SS.expect(n_receivers, calls)
    # (a frame planted across a CS16 / CU8 seam has its halves quantised differently: what counts is that seams matter)
    found = [f for f in SS.seam_frames_of(planted) if S.found(sum(wants, []), f)]
    assert len(found) >= 8
    SS.assert_input_is_for_this(n_receivers, calls, wants, withouts, shareds, found)
    return n_receivers, maps, raw, fmts, wants, model


def test_consecutive_buffers_of_one_receiver_and_alternating_formats(hip_lib, oracle_mod):
    n_receivers, maps, raw, fmts, wants, model = consecutive_case()
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers) as s:
        c = s.c

        def submit(k):
            call = c.submit_iq_device_rx_u8 if fmts[k] == "cu8" else c.submit_iq_device_rx
            call(devs[k].data_ptr(), N * CHUNK, maps[k])

        assert run_pipeline(c, 4, submit) == wants
        S.tables_equal(c, model, n_receivers)
        all_taken(s, 4)


# ------------------------------------------------------------------------------------------------- 4. error correction
@lru_cache(maxsize=None)
def fix_case(mode):
    n_receivers = 3
    bits = (40,) if mode == 1 else (40, 77)
    score = 1200 if mode == 1 else 1100
    repaired = synth.df17_frame(X, 0x99AA5511223344)
    damaged = F.flip(repaired, *bits)
    iq = SS.dense(902).copy()
    m = map_ab(b3=A, b7=A, b9=B, b11=B, b13=A)
    m[m == 3] = 2
    a = quiet(iq, 3, 40000)
    synth.add_bursts(iq, [synth.Burst(5 * a + 1, 24000, 1, DF17_X)])          # A learns X in buffer 3
    SS.plant(iq, 3, iq, 7, -100, damaged, tick=2)                               # a damaged seam DF17 for A: repaired
    SS.plant(iq, 9, iq, 11, -100, damaged, tick=3)                              # ... and for B, who does not know X: not
    SS.plant(iq, 7, iq, 13, -1, damaged, tick=1)                                # ... and for A again at the very last sample
    calls = [(iq, m)]
    wants, withouts, shareds, model = SS.expect(n_receivers, calls, mode=mode)
    got = sorted({(k[0], k[1] < LEAD, k[3]) for k in wants[0] if k[4] == repaired})
    assert (7, True, score) in got and all(b != 11 for b, _, _ in got), got
    assert not [k for k in withouts[0] if k[4] == repaired and k[0] in (7, 11)]
    assert [k for k in shareds[0] if k[4] == repaired and k[0] == 11]          # one shared filter repairs B's too
    RS.assert_tells_apart(n_receivers, wants[0], shareds[0])
    assert len(wants[0]) >= 8 * N
    return n_receivers, iq, m, wants[0], model


@pytest.mark.parametrize("mode", [1, 3])
def test_error_correction_across_the_seam(hip_lib, oracle_mod, mode):
    """Seam DF17s with one (ADSB_FIX_1BIT) and two (ADSB_FIX_2BIT) flipped bits come back with corrected bytes at 1200 /
    1100 for the receiver that knows the aircraft alone, scored on the device."""
    n_receivers, iq, m, want, model = fix_case(mode)
    d = on_device(iq)
    with Combined(n_receivers, fix=mode) as s:
        c = s.c
        c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, m)
        assert collect_dense(c) == want
        S.tables_equal(c, model, n_receivers)
        all_taken(s, 1)


# ------------------------------------------------------------------------------------------------- 5. short last buffers
@lru_cache(maxsize=None)
def short_case(last_len):
    n_receivers = 3
    maps = random_maps(n_receivers, [N, N], 31)
    raw, planted = SS.seam_passes(maps, seed=903)
    cut = CHUNK - last_len
    raw[0] = raw[0][:N * CHUNK - cut]
    calls = list(zip(raw, maps))
    wants, withouts, shareds, model = SS.expect(n_receivers, calls)
    found = [f for f in SS.seam_frames_of(planted) if S.found(sum(wants, []), f)]
    assert len(found) >= len(SS.seam_frames_of(planted)) - 2
    SS.assert_input_is_for_this(n_receivers, calls, wants, withouts, shareds, found)
    return n_receivers, maps, raw, wants, model


@pytest.mark.parametrize("last_len", [100, 327])
def test_a_short_last_buffer(hip_lib, oracle_mod, last_len):
    """The first pass ends in a buffer of 100 / 327 samples; its receiver's next buffer, in the second pass, starts from
    the last 326 samples of (old carry ++ that buffer)."""
    n_receivers, maps, raw, wants, model = short_case(last_len)
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers) as s:
        c = s.c
        for d, x, m in zip(devs, raw, maps):
            c.submit_iq_device_rx(d.data_ptr(), len(x), m)
        got = [RS.keys(c.collect(cap=1 << 17)) for _ in maps]
        assert got == wants
        S.tables_equal(c, model, n_receivers)
        all_taken(s, 2)


# ------------------------------------------------------------------------------------------------- 6. flushes and resets in flight
@lru_cache(maxsize=None)
def flush_case(what):
    n_receivers = 4
    maps = random_maps(n_receivers, [N] * 4, 17)
    raw, planted = SS.seam_passes(maps, seed=900)
    # (the receiver to reset: one with a frame planted across the end of the second pass and the start of the third)
    across = [r for kind in ("straddle", "inside", "last") for k, b, r, _ in planted[kind] if k == 2 and b == list(maps[2]).index(r)]
    assert across
    before = {"flush_all": {2: [("flush", None)]}, "flush_one": {3: [("flush", 1)]},
              "reset_one": {2: [("reset", across[0])]}, "reset_all": {2: [("reset", None)]}}[what]
    calls = list(zip(raw, maps))
    wants, withouts, shareds, model = SS.expect(n_receivers, calls, before=before)
    plain = SS.expect(n_receivers, calls)[0]
    assert wants != plain      # the flush or reset shows
    found = [f for f in SS.seam_frames_of(planted) if S.found(sum(wants, []), f)]
    SS.assert_input_is_for_this(n_receivers, calls, wants, withouts, shareds, found)
    return n_receivers, maps, raw, before, wants, model


@pytest.mark.parametrize("what", ["flush_all", "flush_one", "reset_one", "reset_all"])
def test_flushes_and_resets_with_passes_in_flight(hip_lib, oracle_mod, what):
    """adsb_icao_flush switches to the empty keyed set (nothing drained); adsb_icao_flush_receiver drains and rebuilds;
    adsb_receiver_carry_reset of one receiver and of all is ordered between the passes around it."""
    n_receivers, maps, raw, before, wants, model = flush_case(what)
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers) as s:
        c = s.c

        def between(k):
            for kind, r in before.get(k, []):
                if kind == "flush":
                    c.icao_flush() if r is None else c.icao_flush_receiver(r)
                else:
                    c.receiver_carry_reset() if r is None else c.receiver_carry_reset(r)

        got = run_pipeline(c, 4, lambda k: c.submit_iq_device_rx(devs[k].data_ptr(), N * CHUNK, maps[k]), between=between)
        assert got == wants
        S.tables_equal(c, model, n_receivers)
        all_taken(s, 4, rebuilds=2 if what == "flush_one" else 1)


# ------------------------------------------------------------------------------------------------- 7. refusals
@lru_cache(maxsize=None)
def first_round_tables():
    """every receiver's table after the four passes of parity_case("cs16"), once each"""
    n_receivers, maps, raw = parity_case("cs16")[:3]
    model = S.expect_calls(n_receivers, list(zip(raw, maps)))[1]
    return [model.table(r) for r in range(n_receivers)]


def tables_after_first_round(c, n_receivers):
    for r, want in enumerate(first_round_tables()):
        assert list(c.receiver_filter_table(r)) == want, r


def test_a_seam_list_that_overflows_is_unscored_redone_and_replayed(hip_lib, oracle_mod):
    """adsb_selftest_rx_seam_tune(4): the second pass's seam records do not fit, the merge declares the pass unscored, the
    host refuses, redoes the seam step in pieces and replays; the pass behind it rebuilds the keyed set and is taken from
    the device again."""
    n_receivers, maps, raw, wants, again, model, planted = parity_case("cs16")
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers) as s:
        c = s.c
        steps = []
        for k in range(4):
            if k == 1:
                c.selftest_rx_seam_tune(4)
            if k == 2:
                c.selftest_rx_seam_tune(0)
            c.submit_iq_device_rx(devs[k].data_ptr(), N * CHUNK, maps[k])
            got = collect_dense(c)
            steps.append(s.since())
            print("pass", k, "messages", len(got), "of", len(wants[k]), steps[-1])
            assert got == wants[k], k
        tables_after_first_round(c, n_receivers)
        assert since_core(steps[0]) == dict(ZERO, taken=1, rebuilds=1, merged_passes=1), steps[0]
        assert since_core(steps[1]) == dict(ZERO, taken=1, refused=1, rebuilds=1, replays=1, merged_passes=2, unscored=1), steps[1]
        assert steps[1]["redone"] == 1 and steps[1]["host_seam_records"] > 0
        assert since_core(steps[2]) == dict(ZERO, taken=2, refused=1, rebuilds=2, replays=1, merged_passes=3, unscored=1), steps[2]
        assert since_core(steps[3]) == dict(ZERO, taken=3, refused=1, rebuilds=2, replays=1, merged_passes=4, unscored=1), steps[3]


def test_a_keyed_set_out_of_probes_is_replayed_with_its_seams(hip_lib, oracle_mod):
    n_receivers, maps, raw, wants, again, model, planted = parity_case("cs16")
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers) as s:
        c = s.c
        c.selftest_rx_score_tune(6, 4)    # 64 slots, 4 probes: the first pass's additions cannot all be placed
        c.submit_iq_device_rx(devs[0].data_ptr(), N * CHUNK, maps[0])
        assert collect_dense(c) == wants[0]
        since = s.since()
        assert since["no_room"] >= 1 and since["taken"] == 0 and since["refused"] == 1 and since["replays"] == 1, since
        assert since["merged_passes"] == 1 and since["unscored"] == 0 and since["host_seam_records"] > 0, since
        c.selftest_rx_score_tune(0, 0)
        for k in (1, 2, 3):
            c.submit_iq_device_rx(devs[k].data_ptr(), N * CHUNK, maps[k])
            assert collect_dense(c) == wants[k], k
        tables_after_first_round(c, n_receivers)
        since = s.since()
        assert since["taken"] == 3 and since["refused"] == 1 and since["replays"] == 1 and since["rebuilds"] == 1 + 1, since


@lru_cache(maxsize=None)
def near_full_case():
    n_receivers, n_passes = 2, 6
    m = np.array([0] * 18 + [1] * 2, dtype=np.uint32)
    base = SS.dense(903, n_passes * N, 80)
    raw = [base[k * N * CHUNK:(k + 1) * N * CHUNK].copy() for k in range(n_passes)]
    for k in range(n_passes):   # a straddling DF17 of a new aircraft across three of receiver 0's seams of every pass
        for n, (pb, b) in enumerate(((0, 1), (5, 6), (11, 12))):
            SS.plant(raw[k], pb, raw[k], b, -100, synth.df17_frame(0x490000 + 16 * k + n, 0x58B986D0B3BD25 + n), tick=n)
    own, without, shared = S.SeamModel(n_receivers), S.SeamModel(n_receivers, carry=False), SS.SharedFilterModel(n_receivers)
    held, wants, withouts, shareds = [], [], [], []
    for x in raw:
        held.append(sum(a != 0 for a in own.table(0)))
        wants.append(own.feed(x, m))
        withouts.append(without.feed(x, m))
        shareds.append(shared.feed(x, m))
    assert sum(wants, []) != sum(withouts, [])
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    assert all(len(w) >= 8 * N for w in wants)
    assert held[1] < 2500 and any(h + 64 >= 4096 for h in held) and sum(a != 0 for a in own.table(0)) == 4096
    full_tables = [own.table(r) for r in range(n_receivers)]
    # ... and behind an adsb_icao_flush the first pass once more: every receiver's stream goes on, the filters are empty
    own.flush()
    after_flush = own.feed(raw[0], m)
    assert len(after_flush) >= 8 * N and sum(a != 0 for a in own.table(0)) < 2500
    return n_receivers, m, raw, wants, held, full_tables, after_flush, own


def test_a_receiver_whose_table_comes_within_64_of_full_is_left_to_the_host(hip_lib, oracle_mod):
    """Receiver 0's table fills up pass by pass: while it is far from full the merged passes are taken from the device; once
    it is within 64 of its 4096 slots every pass is refused and replayed by the host, seams included.  Behind an
    adsb_icao_flush the next pass rebuilds the keyed set once and is taken from the device again."""
    n_receivers, m, raw, wants, held, full_tables, after_flush, model = near_full_case()
    with Combined(n_receivers) as s:
        c = s.c
        refused = 0
        for k, x in enumerate(raw):
            counters = s.since()
            d = on_device(x)
            c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, m)
            assert RS.keys(c.collect(cap=1 << 17)) == wants[k], k
            assert c.stats()["n_records"] >= 8 * N
            now = s.since()
            if k < 2:
                assert now["taken"] == counters["taken"] + 1 and now["merged_passes"] == counters["merged_passes"] + 1, (k, now)
            if held[k] + 64 >= 4096:
                assert now["refused"] == counters["refused"] + 1 and now["replays"] == counters["replays"] + 1, (k, now)
                refused += 1
        for r in range(n_receivers):
            assert list(c.receiver_filter_table(r)) == full_tables[r], r
        before = s.since()
        assert refused >= 1 and before["no_room"] == 0
        c.icao_flush()
        d = on_device(raw[0])
        c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, m)
        assert collect_dense(c) == after_flush
        S.tables_equal(c, model, n_receivers)
        now = s.since()
        moved = {k: now[k] - before[k] for k in ZERO}
        assert moved == dict(ZERO, taken=1, rebuilds=1, merged_passes=1), (before, now)


# ------------------------------------------------------------------------------------------------- 8. a blocking call cut into passes
@lru_cache(maxsize=None)
def blocking_case():
    n_receivers, n = 3, 45
    m1, m2 = random_maps(n_receivers, [n, n], 11)
    cuts = [(0, 20), (20, 40), (40, 45)]
    maps = [m1[a:z] for a, z in cuts] + [m2[a:z] for a, z in cuts]
    base = SS.dense(901, n)
    raw = []
    latest = {}
    pieces = [base[a * CHUNK:z * CHUNK].copy() for a, z in cuts] + [base[a * CHUNK:z * CHUNK].copy() for a, z in cuts]
    seams = 0
    planted = []
    for k, mp in enumerate(maps):
        for b, r in enumerate(int(x) for x in mp):
            if r in latest:
                if seams % 4 == 0:
                    pk, pb = latest[r]
                    f = synth.df17_frame(0x4A0000 + seams, 0x58B986D0B3BD25 + seams)
                    SS.plant(pieces[pk], pb, pieces[k], b, -100, f, tick=seams % 5)
                    planted.append(f)
                seams += 1
            latest[r] = (k, b)
    raw = [np.concatenate(pieces[:3]), np.concatenate(pieces[3:])]
    calls = [(raw[0], m1), (raw[1], m2)]
    wants, withouts, shareds, model = SS.expect(n_receivers, calls)
    SS.assert_input_is_for_this(n_receivers, calls, wants, withouts, shareds, planted)
    return n_receivers, n, raw, (m1, m2), wants, model


def test_blocking_call_cut_into_passes(hip_lib, oracle_mod):
    """adsb_demod_iq_device_rx over 45 buffers is cut into 20 + 20 + 5: two merged passes taken from the device and a small
    one the host scores, seams included; the next call rebuilds the keyed set."""
    n_receivers, n, raw, (m1, m2), wants, model = blocking_case()
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers) as s:
        c = s.c
        assert RS.keys(c.demod_iq_device_rx(devs[0].data_ptr(), n * CHUNK, m1, cap=1 << 18)) == wants[0]
        assert c.stats()["n_records"] >= 8 * n
        since = s.since()
        assert since_core(since) == dict(ZERO, taken=2, rebuilds=1, replays=1, merged_passes=2), since
        assert since["host_seam_records"] > 0        # the 5-buffer pass: merged and replayed by the host
        assert RS.keys(c.demod_iq_device_rx(devs[1].data_ptr(), n * CHUNK, m2, cap=1 << 18)) == wants[1]
        assert since_core(s.since()) == dict(ZERO, taken=4, rebuilds=2, replays=2, merged_passes=4), s.since()
        S.tables_equal(c, model, n_receivers)


# ------------------------------------------------------------------------------------------------- 9. the ring and the plain calls
def test_the_ring_and_the_plain_calls_as_receiver_0(hip_lib, oracle_mod):
    n_receivers, maps, raw, wants = parity_case("cs16")[:4]
    model = S.expect_calls(n_receivers, list(zip(raw, maps)))[1]   # (a model of this test's own: the plain call moves it on)
    with Combined(n_receivers) as s:
        c = s.c
        c.ring_create(N * CHUNK)

        def submit(k):
            buf = c.ring_acquire()
            buf[:N * CHUNK] = raw[k]
            c.ring_submit_rx(N * CHUNK, maps[k])

        assert run_pipeline(c, 4, submit, depth=3) == wants
        S.tables_equal(c, model, n_receivers)
        all_taken(s, 4)
        # the plain call: every buffer is receiver 0, a stream of 20 consecutive buffers with carry-over
        zeros = np.zeros(N, dtype=np.uint32)
        want_plain = model.feed(raw[0], zeros)
        d = on_device(raw[0])
        assert RS.keys(c.demod_iq_device(d.data_ptr(), N * CHUNK, cap=1 << 17)) == want_plain
        S.tables_equal(c, model, n_receivers)
        all_taken(s, 5)


# ------------------------------------------------------------------------------------------------- 10. the interface
def test_the_interface(hip_lib, oracle_mod):
    from dump1090_rs_amd import Context
    INVALID, BUSY, OK = -1, -7, 0
    d = on_device(SS.dense())
    zeros = np.zeros(N, dtype=np.uint32)
    with Context(0, N) as c:
        L, h = c._L, c._h
        assert L.adsb_set_receiver_carry_scoring(None, 1) == INVALID and L.adsb_get_receiver_carry_scoring(None) == INVALID
        assert L.adsb_set_receiver_carry_scoring(h, 1) == INVALID and L.adsb_set_receiver_carry_scoring(h, 0) == INVALID   # receivers off
        c.set_receivers(3)
        # the single modes still refuse each other, in both orders
        assert L.adsb_set_receiver_scoring(h, 1) == OK and L.adsb_set_receiver_carry(h, 1) == INVALID
        assert L.adsb_set_receiver_scoring(h, 0) == OK and L.adsb_set_receiver_carry(h, 1) == OK
        assert L.adsb_set_receiver_scoring(h, 1) == INVALID
        assert L.adsb_set_receiver_carry(h, 0) == OK
        held = c.selftest_reservations()      # (the keyed sets stay reserved once scoring has been on)
        # from any state of the single modes
        for first in (None, "carry", "scoring"):
            if first == "carry":
                c.set_receiver_carry(True)
            elif first == "scoring":
                c.set_receiver_scoring(True)
            assert L.adsb_set_receiver_carry_scoring(h, 1) == OK
            assert c.get_receiver_carry_scoring() and c.get_receiver_carry() and c.get_receiver_scoring()
            assert c.selftest_reservations() > held
            assert L.adsb_set_receiver_carry(h, 1) == OK and L.adsb_set_receiver_scoring(h, 1) == OK      # the value in effect
            assert L.adsb_set_receiver_carry(h, 0) == INVALID and L.adsb_set_receiver_scoring(h, 0) == INVALID   # a change
            assert c.get_receiver_carry() and c.get_receiver_scoring()
            assert L.adsb_set_receiver_carry_scoring(h, 1) == OK                                        # again: fine
            assert L.adsb_set_receiver_carry_scoring(h, 0) == OK
            assert not c.get_receiver_carry_scoring() and not c.get_receiver_carry() and not c.get_receiver_scoring()
            assert c.selftest_reservations() == held                                                  # the storage is back
        assert L.adsb_set_receiver_carry_scoring(h, 0) == OK   # off while off
        # BUSY while a pass is pending
        c.set_receiver_carry_scoring(True)
        c.submit_iq_device_rx(d.data_ptr(), N * CHUNK, zeros)
        assert L.adsb_set_receiver_carry_scoring(h, 0) == BUSY and L.adsb_set_receiver_carry_scoring(h, 1) == BUSY
        c.collect(cap=1 << 17)
        assert c.get_receiver_carry_scoring()
        # another number of receivers: still on, both footprints re-sized; none: off
        c.set_receivers(5)
        assert c.get_receiver_carry_scoring() and c.get_receiver_carry() and c.get_receiver_scoring()
        c.set_receivers(0)
        assert not c.get_receiver_carry_scoring() and not c.get_receiver_carry() and not c.get_receiver_scoring()
        assert c.selftest_reservations() == held
    # a context that never orders a pass on the device: ADSB_OK, and the host scores its seam passes
    with Context(0, 4) as c:
        c.set_receivers(2)
        c.set_receiver_carry_scoring(True)
        assert c.get_receiver_carry_scoring() and c.get_receiver_carry() and c.get_receiver_scoring()
        streams, planted = S.catalogue(2, 4)
        m = S.round_robin(2, 4)
        iq = S.interleave(streams, m)
        (want,), model = S.expect_calls(2, [(iq, m)])
        assert RS.keys(c.demod_iq_rx(iq, m, cap=1 << 17)) == want
        S.tables_equal(c, model, 2)
        assert c.selftest_rx_seam_score_counters() == {"merged_passes": 0, "seam_records": 0, "dropped": 0, "unscored": 0}
        assert c.selftest_rx_seam_counters()["records"] > 0


@pytest.mark.parametrize("mode", ["carry", "scoring", "neither"])
def test_with_the_mode_off_nothing_is_merged(hip_lib, oracle_mod, mode):
    """Each single mode and neither: no merge launch, the mode's counters stay where they were, and the lists are what
    that mode always returned."""
    n_receivers, maps, raw, wants, again, model, planted = parity_case("cs16")
    calls = list(zip(raw, maps))
    if mode == "carry":
        want = wants
    else:
        want = S.expect_calls(n_receivers, calls, carry=False)[0]
    devs = [on_device(x) for x in raw]
    with Combined(n_receivers, mode=mode) as s:
        c = s.c
        assert not c.get_receiver_carry_scoring()
        got = run_pipeline(c, 4, lambda k: c.submit_iq_device_rx(devs[k].data_ptr(), N * CHUNK, maps[k]))
        assert got == want
        since = s.since()
        assert since["merged_passes"] == 0 and since["seam_records"] == 0 and since["dropped"] == 0 and since["unscored"] == 0
        assert (since["taken"], since["replays"]) == ((4, 0) if mode == "scoring" else (0, 4)), since

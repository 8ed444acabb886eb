"""Device-side scoring where addresses collide in its first-adder table (ScoreDev::hash: k_records inserts through
score_hash_insert, k_score looks up through score_hash_first, k_emit empties the slot each adder remembered).  The
streams of tests/score_hash_support.py put 130 (or 600) different addresses on four (six) neighbouring home slots at the
END of the table, so that every insertion walks through a cluster, most of them across the wrap from the last slot to
slot 0, and looks up addresses nobody taught across that cluster.  Reference: the CPU oracle (the restatement of
single-bit repair for the fix test), tolerance 0; adsb_host_replays / adsb_host_sorts / retries (the adsb_multi counters)
say that the device ordered and scored the pass under test.  tests/test_score_hash_cpu.py holds the formulas the
construction rests on against the library's own."""
import pytest

from tests import fix_support as fs
from tests import formats_support as F
from tests import score_hash_support as H

pytestmark = pytest.mark.gpu
CHUNK = H.CHUNK
N = H.N_BUFFERS
_cache = {}


def lkeys(msgs):
    return [H.key(m) for m in msgs]


def want_of(orc, iq):
    return [H.okey(w) for w in orc.demod_iq(iq, cap=1 << 20)[0]]


def warm_up(n_buffers=N):
    if ("warm", n_buffers) not in _cache:
        _cache[("warm", n_buffers)] = F.fill_capture(0x5CA0, n_buffers)
    return _cache[("warm", n_buffers)]


def on_device(iq):
    import torch
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    return d


def host_counters(c):
    return int(c._L.adsb_host_replays(c._h)), int(c._L.adsb_host_sorts(c._h))


def open_dense(c):
    """one dense pass (the host's: it tells the context how dense the stream is) and an icao_flush; -> the counters that
    must not move from here on"""
    d = on_device(warm_up())
    c.demod_iq_device(d.data_ptr(), N * CHUNK, cap=1 << 20)
    c.icao_flush()
    return host_counters(c)


def scored_here(c, label):
    """the pass collected last was not redone buffer by buffer (no bucket of 1024 overflowed)"""
    st = c.stats()
    print(label, "n_records", st["n_records"], "per buffer", st["n_records"] / max(1, st["n_chunks"]))
    assert st["retries"] == 0 and st["n_chunks"] == N, (label, st)


def fresh_and_known(oracle_mod, s):
    """the oracle's lists of the stream on an empty filter and, without a flush, once more; its table after the first"""
    k = ("lists", s.max_chunks, s.form, len(s.iq))
    if k not in _cache:
        orc = oracle_mod.Oracle()
        fresh = want_of(orc, s.iq)
        table = list(orc.filter.a)
        _cache[k] = (fresh, want_of(orc, s.iq), table)
    return _cache[k]


@pytest.mark.parametrize("max_chunks, form", [(17, "small"), (29, "small"), (17, "large")])
def test_parity_across_the_cluster(hip_lib, oracle_mod, max_chunks, form):
    """The colliding stream through a context of 2^16 slots (17 buffers) and of 2^17 (29 buffers: other addresses make up
    the cluster there, so the mask is followed), blocking device-resident and submit / collect, each on an empty filter;
    then once more WITHOUT a flush, every taught address in the exact bitmap and inserted again -- the filter the device
    passes built answers like the oracle's for every taught address and every stranger (a plain context has no call
    that returns its table; test_refused_results_still_clean_up compares adsb_multi's slot for slot).
    n_records per buffer seen on the MI355X: 119.9 (17 buffers' context) and 120.0 (29) in the small form, 519.6 in the
    large one; every pass, with or without a flush in front."""
    from dump1090_rs_amd import Context
    s = H.colliding_stream(max_chunks, form)
    assert H.hash_size(max_chunks) == {17: 1 << 16, 29: 1 << 17}[max_chunks]
    if max_chunks == 29:
        other = H.colliding_stream(17, form)
        assert set(s.taught) != set(other.taught) and len({H.home(a, 29) for a in other.taught}) > 4
    fresh, known, table = fresh_and_known(oracle_mod, s)
    H.check_preconditions(fresh, s, table)
    assert sum(H.known_replies(known).get(a, 0) for a in s.taught) >= sum(H.known_replies(fresh).get(a, 0) for a in s.taught) + len(s.taught) // 2 - 5
    assert not any(a in H.known_replies(known) for a in s.strangers)
    d = on_device(s.iq)
    with Context(0, max_chunks) as c:
        before = open_dense(c)
        assert lkeys(c.demod_iq_device(d.data_ptr(), len(s.iq), cap=1 << 20)) == fresh, "blocking"
        scored_here(c, f"{max_chunks} {form} blocking")
        c.icao_flush()
        c.submit_iq_device(d.data_ptr(), len(s.iq))
        assert lkeys(c.collect(cap=1 << 20)) == fresh, "submit / collect"
        scored_here(c, f"{max_chunks} {form} pipelined")
        c.submit_iq_device(d.data_ptr(), len(s.iq))
        assert lkeys(c.collect(cap=1 << 20)) == known, "without a flush"
        scored_here(c, f"{max_chunks} {form} known")
        assert host_counters(c) == before


def test_nothing_is_left_behind_in_any_slots_table(hip_lib, oracle_mod):
    """Four colliding passes in flight, one per slot (each slot has a table of its own), an icao_flush before each; then,
    again flushed, four passes of ordinary dense fill whose last four buffers hold another small cluster at the same
    homes (its keys take the home slots, so a lookup of a taught address walks on into what was left behind them), a
    DF18 of every taught address and DF4, DF20 and all-call (DF11, IID != 0) replies to it
    (score_hash_support.replies_capture).  Nothing teaches these addresses: the oracle scores the DF18s 1400 and emits
    none of the replies.  An entry left in a slot's table carries a first index of a few hundred: the DF18 would score
    1800 (and add nothing), the replies 1000.
    n_records per buffer seen on the MI355X: 119.9 in the colliding passes, 301.0 in the fill passes."""
    from dump1090_rs_amd import Context
    s = H.colliding_stream(N, "small")
    rep = H.replies_capture([s.taught], avoid=s.strangers)
    fresh, _, table = fresh_and_known(oracle_mod, s)
    H.check_preconditions(fresh, s, table)
    orc = oracle_mod.Oracle()
    quiet = want_of(orc, rep)
    # the reference hears the DF18 of (nearly) every taught address at 1400 and answers none of the replies
    heard18 = {int.from_bytes(k[4][1:4], "big") for k in quiet if k[4][0] >> 3 == 18 and k[3] == 1400 and k[0] >= N - 4}
    assert len(heard18 & set(s.taught)) >= len(s.taught) - 2
    assert not H.replies_to(quiet, s.taught)
    assert sum(v != 0 for v in orc.filter.a) < 4096 - 64 - 600
    d, dr = on_device(s.iq), on_device(rep)
    with Context(0, N) as c:
        before = open_dense(c)
        depth = c.max_in_flight()
        assert depth == 4
        for stream, want, label in ((d, fresh, "colliding"), (dr, quiet, "replies")):
            for k in range(depth):
                c.icao_flush()
                c.submit_iq_device(stream.data_ptr(), N * CHUNK)
            assert c.pending() == depth
            for k in range(depth):
                got = lkeys(c.collect(cap=1 << 20))
                late = H.replies_to(got, s.taught) if label == "replies" else []
                assert not late, (k, late[:4])
                assert got == want, (label, k)
                scored_here(c, f"{label} {k}")
        assert host_counters(c) == before


def test_the_same_address_taught_twice_from_another_workgroup(hip_lib, oracle_mod):
    """Every taught address of the small form has a second teacher (a DF17 for half, a DF11 with IID 0 for the rest) in a
    later buffer than its first: the second insertion comes from another workgroup of k_records, finds the key in a slot
    some way down the walk and must leave the LOWER index there (atomicMin).  From the oracle's list alone: for at least
    100 taught addresses the first emission of a teacher is followed, in another buffer, by one at 1800 / 1600, and
    nothing answered for the address before that first teacher.  The first emission itself would be at 1400 / 750 only
    where a single trial phase of its position slices the frame clean; where a second one does too, the position emits
    that one, at 1800 / 1600 -- the first phase added the address (formats_support._expect).  At this stream's amplitudes
    every first teacher has two clean phases: the oracle emits all 130 at 1800 and none at 1400 / 750 (asserted below as
    what it is, so that a change of the stream shows).  That first 1800 rests on the same entry: the second phase's
    index is the first adder's + 1, and an entry holding any later index turns it into a 1400.
    n_records per buffer seen on the MI355X: 119.9."""
    from dump1090_rs_amd import Context
    s = H.colliding_stream(N, "small")
    fresh, _, table = fresh_and_known(oracle_mod, s)
    H.check_preconditions(fresh, s, table)
    twice, literal = H.taught_twice(fresh, s)
    print("taught twice across buffers:", len(twice), "first emission at 1400 / 750:", len(literal))
    assert len(twice) >= 100
    first_score = {}
    for k in fresh:
        a = int.from_bytes(k[4][1:4], "big")
        if k[4][0] >> 3 in (11, 17) and a in set(s.taught):
            first_score.setdefault(a, k[3])
    assert len(first_score) == 130 and set(first_score.values()) == {1800} and not literal
    d = on_device(s.iq)
    with Context(0, N) as c:
        before = open_dense(c)
        got = lkeys(c.demod_iq_device(d.data_ptr(), len(s.iq), cap=1 << 20))
        assert H.taught_twice(got, s) == (twice, literal)
        assert got == fresh
        scored_here(c, "taught twice")
        assert host_counters(c) == before


def test_with_an_earlier_passs_knowledge(hip_lib, oracle_mod):
    """The colliding pass without a flush behind a pass that taught the 60 addresses at home S-1 only: those are in the
    exact bitmap AND inserted again, their replies in front of the teachers now score 1000, their teachers 1800; the
    other 70 are taught by this pass as before.  One oracle stream over both passes.
    n_records per buffer seen on the MI355X: 81.7 in the teaching pass, 119.9 in the colliding pass."""
    from dump1090_rs_amd import Context
    s = H.colliding_stream(N, "small")
    early = s.at_home(-1)
    assert len(early) == 60
    pre = H.teaching_stream(early, N)
    orc = oracle_mod.Oracle()
    w0, w1 = want_of(orc, pre), want_of(orc, s.iq)
    H.check_preconditions(w1, s, list(orc.filter.a))
    taught_by_pre = {int.from_bytes(k[4][1:4], "big") for k in w0 if k[4][0] >> 3 == 17}
    assert set(early) <= taught_by_pre and not taught_by_pre & (set(s.taught) - set(early)) and not taught_by_pre & set(s.strangers)
    fresh, _, _ = fresh_and_known(oracle_mod, s)
    gained = sum(H.known_replies(w1).get(a, 0) for a in early) - sum(H.known_replies(fresh).get(a, 0) for a in early)
    assert gained >= 20, gained                                    # the replies "before", of those that have one
    assert not any(k[3] in (1400, 750) and int.from_bytes(k[4][1:4], "big") in set(early) for k in w1)
    assert w1 != fresh
    dp, d = on_device(pre), on_device(s.iq)
    with Context(0, N) as c:
        before = open_dense(c)
        c.submit_iq_device(dp.data_ptr(), N * CHUNK)
        c.submit_iq_device(d.data_ptr(), N * CHUNK)
        assert lkeys(c.collect(cap=1 << 20)) == w0
        scored_here(c, "teaching pass")
        assert lkeys(c.collect(cap=1 << 20)) == w1
        scored_here(c, "colliding pass behind it")
        assert host_counters(c) == before


@pytest.mark.parametrize("n_ctx", [2, 3])
def test_refused_results_still_clean_up(hip_lib, oracle_mod, n_ctx):
    """adsb_multi over n contexts of 17 buffers, a capture of 17 n: shard 0 is the small form; the later shards hold
    replies to everything the shards before them taught (ScoreDev::earlier) and a cluster of their own at the same
    homes.  With score_mode 0 the shards' device results are used, with 2 every one is refused and the host replays the
    records -- k_emit has emptied the tables all the same: behind a flush, a capture of ordinary fill whose shards end
    in DF18s of and replies to the addresses their device inserted the capture before emits none of those replies.  Each
    capture is sent once per capture in flight, so that every slot's table of every device has held the cluster.
    Messages and the filter table (slot for slot) equal the oracle's after both captures.
    n_records per buffer seen on the MI355X: 113.8 / 122.6 in the colliding captures of 2 / 3 shards, 301.4 / 301.7 in
    the fill captures."""
    from dump1090_rs_amd.multi import MultiContext
    cap = H.multi_capture(n_ctx)
    groups = [cap.taught] + cap.extra_taught
    everyone = [a for g in groups for a in g]
    assert len(groups) == n_ctx and len(cap.iq) == n_ctx * N * CHUNK and len(set(everyone)) == 130 * n_ctx
    rep = H.replies_capture(groups, avoid=cap.strangers)
    warm = warm_up(n_ctx * N)
    orc = oracle_mod.Oracle()
    w_cap = want_of(orc, cap.iq)
    t_cap = list(orc.filter.a)
    H.check_preconditions(w_cap, cap, t_cap, taught=everyone)
    # (found through `earlier`: the later shards' replies to shard 0's addresses)
    assert sum(1 for k in w_cap if k[0] >= N and k[3] == 1000 and H.ap_address(k[4]) in set(cap.taught)) >= 120 * (n_ctx - 1)
    orc.icao_flush()
    w_rep = want_of(orc, rep)
    t_rep = list(orc.filter.a)
    assert not H.replies_to(w_rep, everyone)
    heard18 = {int.from_bytes(k[4][1:4], "big") for k in w_rep if k[4][0] >> 3 == 18 and k[3] == 1400}
    assert len(heard18 & set(everyone)) >= 128 * n_ctx
    assert sum(v != 0 for v in t_rep) < 4096 - 64 - 600
    for score_mode in (0, 2):
        with MultiContext([0] * n_ctx, N) as m:
            m.selftest_tune(score_mode=score_mode)
            m.demod_iq(warm, cap=1 << 20)
            m.icao_flush()
            depth = m.max_in_flight()
            c0 = m.selftest_counters()
            for k in range(depth):                  # (once per slot of every device context: each slot has its own table)
                m.icao_flush()
                m.submit_iq(cap.iq)
            for k in range(depth):
                assert lkeys(m.collect(cap=1 << 20)) == w_cap, (n_ctx, score_mode, k)
                print("colliding capture", n_ctx, score_mode, k, "n_records per buffer", m.stats()["n_records"] / (n_ctx * N))
                assert m.stats()["retries"] == 0
            assert list(m.filter_table()) == t_cap
            c1 = m.selftest_counters()
            for k in range(depth):
                m.icao_flush()
                m.submit_iq(rep)
            for k in range(depth):
                got = lkeys(m.collect(cap=1 << 20))
                late = H.replies_to(got, everyone)
                assert not late, (score_mode, k, late[:4])
                assert got == w_rep, (n_ctx, score_mode, k)
                print("fill capture", n_ctx, score_mode, k, "n_records per buffer", m.stats()["n_records"] / (n_ctx * N))
                assert m.stats()["retries"] == 0
            assert list(m.filter_table()) == t_rep
            c2 = m.selftest_counters()
            print(n_ctx, score_mode, c0, c1, c2)
            for a, z in ((c0, c1), (c1, c2)):
                assert z["device_scored_shards"] - a["device_scored_shards"] >= depth * n_ctx, (a, z)
                if score_mode == 0:
                    assert z["scored_results_used"] - a["scored_results_used"] >= depth * n_ctx and z["scored_results_refused"] == 0, (a, z)
                else:
                    assert z["scored_results_used"] == 0 and z["scored_results_refused"] - a["scored_results_refused"] >= depth * n_ctx, (a, z)


def test_error_correction_on(hip_lib, oracle_mod):
    """The small form under ADSB_FIX_1BIT, with a DF17 whose message bit 40 is flipped (the address field intact) of ten
    taught addresses, behind their teachers, and of ten strangers: 1200 with the clean bytes for the former -- the
    repaired address is looked up through the cluster --, nothing for the latter.  Reference: tests/fix_restatement.c.
    n_records per buffer seen on the MI355X: 126.4."""
    from dump1090_rs_amd import Context
    s = H.colliding_stream(N, "small", fix=True)
    r = fs.Restated(1)
    want = [H.rkey(k) for k in r.demod_iq(s.iq)]
    H.check_preconditions(want, s, list(r.filter.a))
    assert sum(known for _, known in s.damaged.values()) == 10 and len(s.damaged) == 20
    for good, (a, known) in s.damaged.items():
        mine = [k for k in want if k[4] == good]
        if known:
            assert mine and all(k[3] == 1200 for k in mine), (hex(a), mine)
        else:
            assert not mine, (hex(a), mine)
    assert sum(k[3] == 1200 for k in want) >= 10
    d = on_device(s.iq)
    with Context(0, N) as c:
        c.set_error_correction(1)
        before = open_dense(c)
        assert lkeys(c.demod_iq_device(d.data_ptr(), len(s.iq), cap=1 << 20)) == want, "blocking"
        scored_here(c, "fix blocking")
        c.icao_flush()
        c.submit_iq_device(d.data_ptr(), len(s.iq))
        assert lkeys(c.collect(cap=1 << 20)) == want, "submit / collect"
        scored_here(c, "fix pipelined")
        assert host_counters(c) == before

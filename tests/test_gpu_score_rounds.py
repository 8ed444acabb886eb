"""Device-side ordering and scoring at the edges of its four fixed sizes (tests/score_rounds_support.py restates them,
tests/test_score_rounds_cpu.py holds the restatement against the sources):
  kHitCap = 32        hits a tile of the scan stages in LDS; the 33rd takes its place with an atomic of its own
  kTileBucket = 56    places in a tile's sub-bucket, shared by the scan's hits and the match's; the 57th redoes the pass
  kScoreBlocks = 256  blocks (of 256 threads) of k_score / k_emit: above 65536 hits a block runs more than one round
  ScoreDev::cap       hits a pass may have to be scored on the device; one more and the host replays it
Streams on an all-zero background with an EXACT number of hits (n_records is asserted in every leg), composed from patches
whose counts the device measured; every list against the CPU oracle at tolerance 0 -- (chunk, j, try_phase, score, msg,
signal_level bits), in order; adsb_host_sorts / adsb_host_replays / retries say which path the pass under test took.
Every leg: an ordinary dense pass first (the host's: it tells the context how dense the stream is), an icao_flush and the
pass under test, then ordinary passes, four in flight, until the slot of the pass under test has been used again."""
import ctypes as C
import time

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import score_rounds_support as S

pytestmark = pytest.mark.gpu
CHUNK = S.CHUNK
N17 = 17                      # the smallest three-launch pass
MIDDLE, LAST = (8, 8), (16, 16)   # (buffer, tile): a tile in the middle of a buffer; the last, ragged tile of the last buffer


# ------------------------------------------------------------------------------------ references
class OracleRef:
    def __init__(self, oracle_mod, host=lambda iq: iq):
        self.orc, self.host = oracle_mod.Oracle(), host

    def flush(self):
        self.orc.icao_flush()

    def run(self, iq):
        return S.oracle_list(self.orc, self.host(iq), threads=16)


class FixRef:
    """single-bit repair: the restatement of tests/fix_support.py (the oracle itself repairs nothing)"""

    def __init__(self):
        from tests import fix_support
        self.fs, self.r = fix_support, fix_support.Restated(1)

    def flush(self):
        self.r.icao_flush()

    def run(self, iq):
        a = np.ascontiguousarray(iq, dtype=np.int16)
        out = np.zeros(1 << 16, dtype=S.MSG)
        n = self.fs.restatement().fix_demod_iq(C.byref(self.r.filter), a.ctypes.data, a.shape[0], 1, None, out.ctypes.data, len(out))
        assert n <= len(out)
        return out[:n].copy()


class RxRef:
    """one oracle per receiver, one demod_iq per buffer (tests/receivers_support.py: Model.feed)"""

    def __init__(self, oracle_mod, receivers):
        self.orcs = [oracle_mod.Oracle() for _ in range(int(max(receivers)) + 1)]
        self.map = receivers

    def flush(self):
        for o in self.orcs:
            o.icao_flush()

    def run(self, iq):
        return S.oracle_list_rx(self.orcs, iq, self.map)


# ------------------------------------------------------------------------------------ one leg
class Leg:
    """The same passes through a context and through the reference, compared as they are collected."""

    def __init__(self, dev: S.Device, ref, streams: dict, n_samples: int):
        self.dev, self.ref, self.streams, self.n = dev, ref, streams, n_samples    # streams: kind -> (device tensor, host CS16)
        self.q = []

    def flush(self):
        self.dev.c.icao_flush()
        self.ref.flush()

    def _judge(self, kind, got, want):
        diff = S.first_difference(got, want)
        assert diff is None, (kind, diff)
        return self.dev.c.stats()

    def blocking(self, kind):
        want = self.ref.run(self.streams[kind][1])
        return self._judge(kind, self.dev.blocking(self.streams[kind][0].data_ptr(), self.n), want)

    def submit(self, kind):
        self.q.append((kind, self.ref.run(self.streams[kind][1])))
        self.dev.submit(self.streams[kind][0].data_ptr(), self.n)

    def collect(self):
        kind, want = self.q.pop(0)
        return self._judge(kind, self.dev.collect(), want)


def on_device_path(st, hits, dev, before, label):
    print(label, "n_records", st["n_records"], "retries", st["retries"], "counters", dev.counters(), "before", before)
    assert st["n_records"] == hits, (label, st)
    assert st["retries"] == 0, (label, st)
    assert dev.counters() == before, (label, "the host replayed or sorted the pass", dev.counters(), before)


def small_leg(dev, ref, streams, hits, overflows=False):
    """17 buffers.  W blocking (the host's); flush, T blocking; W, W blocking (dense again whatever T said about the
    stream); flush, T W W W in flight; T and one W collected, two more W submitted -- the first of them into T's slot --
    and everything collected.  Every list against the reference; T ordered and scored on the device with `hits` records,
    or (overflows) redone buffer by buffer with the pass behind it clean."""
    leg = Leg(dev, ref, streams, N17 * CHUNK)
    leg.flush()
    leg.blocking("W")
    before = dev.counters()
    leg.flush()
    st = leg.blocking("T")
    if overflows:
        print("blocking", st["n_records"], st["retries"])
        assert st["retries"] > 0, st
    else:
        on_device_path(st, hits, dev, before, "blocking")
    assert leg.blocking("W")["retries"] == 0
    assert leg.blocking("W")["retries"] == 0
    before = dev.counters()
    leg.flush()
    for kind in "TWWW":
        leg.submit(kind)
    assert dev.c.pending() == 4 == dev.c.max_in_flight()
    st = leg.collect()
    if overflows:
        assert st["retries"] > 0, st
    else:
        on_device_path(st, hits, dev, before, "in flight")
    assert leg.collect()["retries"] == 0
    leg.submit("W")        # T's slot
    leg.submit("W")
    while leg.q:
        assert leg.collect()["retries"] == 0
    if not overflows:
        assert dev.counters() == before     # every pass behind it was ordered and scored on the device too


# ------------------------------------------------------------------------------------ fixtures
_warm = {}


def warm_17(seed=0x5C0):
    if seed not in _warm:
        _warm[seed] = synth.make_iq(N17 * CHUNK, n_bursts=10 * N17, seed=seed, n_icao=9, df11_every=4)
    return _warm[seed]


class Bench17:
    """a meter, its pool and the context under test of one (format, error-correction mode)"""

    def __init__(self, fmt="cs16", fix=0):
        self.fmt, self.fix = fmt, fix
        self.meter = S.Meter(N17, fmt, fix)
        t0 = time.perf_counter()
        self.pool = S.Pool(self.meter)
        print(fmt, fix, "pool", self.pool.describe(), "seconds", round(time.perf_counter() - t0, 2))
        self.w = (self.meter.to_device(warm_17()), self.host(warm_17()))
        self.cache = {}

    def host(self, iq):
        """what the reference reads: the samples themselves, or what the CU8 bytes made of them mean"""
        return S.widen(S.quantise(iq)) if self.fmt == "cu8" else iq

    def ref(self, oracle_mod):
        return FixRef() if self.fix else OracleRef(oracle_mod)

    def streams(self, key, build):
        if key not in self.cache:
            patches = build()
            iq = S.paste(N17, patches)
            self.cache[key] = {"T": (self.meter.to_device(iq), self.host(iq)), "W": self.w}
        return self.cache[key]

    def scan_count(self, patches, place):
        """the hits the SCAN finds in the tile, from the oracle's trial records (not under repair: more trials are hits)"""
        return None if self.fix else S.scan_hits_in_tile(self.host(S.paste(N17, patches)), *place)

    def close(self):
        self.meter.close()


@pytest.fixture(scope="module")
def benches(hip_lib):
    made = {}

    def get(fmt="cs16", fix=0):
        if (fmt, fix) not in made:
            made[(fmt, fix)] = Bench17(fmt, fix)
        return made[(fmt, fix)]
    yield get
    for b in made.values():
        b.close()


def context_17(bench):
    from dump1090_rs_amd import Context
    c = Context(0, N17)
    if bench.fix:
        c.set_error_correction(bench.fix)
    return c


def scan_only_tile(bench, place, hits):
    """exactly `hits` records in the tile of `place`, every one a self-validating trial the scan finds"""
    pool = bench.pool

    def make(want, salt):
        ids = S.choose_slots(S.without_slot(pool.scan_options(), salt), lambda s, m: s == want)
        return None if ids is None else S.tile_patches(pool, *place, ids)

    def count(patches):
        return (bench.meter.count(patches), bench.scan_count(patches, place))
    made, got = S.settle(count, hits, make, accept=lambda got: got[0] == hits and got[1] in (None, hits))
    return made


# ------------------------------------------------------------------------------------ leg 1: one tile, scan hits only
@pytest.mark.parametrize("place", [MIDDLE, LAST], ids=["middle", "last"])
@pytest.mark.parametrize("hits", [31, 32, 33, 55, 56, 57])
def test_one_tiles_sub_bucket_scan_hits_only(hip_lib, oracle_mod, benches, place, hits):
    """31 and 32 hits are staged in LDS and leave in the epilogue's "alone" form; from 33 the extras leave stage_hit one by
    one and the epilogue takes hit_base from the same counter; 55 and 56 fill the sub-bucket; 57 overflows it."""
    bench = benches()
    streams = bench.streams(("scan", place, hits), lambda: scan_only_tile(bench, place, hits))
    with context_17(bench) as c:
        small_leg(S.Device(c), bench.ref(oracle_mod), streams, hits, overflows=hits > S.TILE_BUCKET)


@pytest.mark.parametrize("fmt, fix", [("cu8", 0), ("cs16", 1)], ids=["cu8", "fix1"])
@pytest.mark.parametrize("hits", [33, 56])
def test_one_tiles_sub_bucket_in_the_other_instantiations(hip_lib, oracle_mod, benches, fmt, fix, hits):
    """the same body as CU8 and under ADSB_FIX_1BIT (counts measured by a meter of the same kind)"""
    bench = benches(fmt, fix)
    streams = bench.streams(("scan", MIDDLE, hits), lambda: scan_only_tile(bench, MIDDLE, hits))
    with context_17(bench) as c:
        small_leg(S.Device(c, fmt), bench.ref(oracle_mod), streams, hits)


# ------------------------------------------------------------------------------------ leg 2: scan and match share a tile
SHARED = {"56 staged": (56, 16, 32), "56 extras": (56, 33, 48), "57": (57, 16, 48)}


@pytest.mark.parametrize("case", list(SHARED))
def test_scan_and_match_share_a_sub_bucket(hip_lib, oracle_mod, benches, case):
    """s self-validating hits and the DF4 / DF5 / DF20 / DF21 replies to an address a DF17 teaches in an earlier buffer of
    the pass, in one tile: 56 with s <= 32 (the scan's plain store of the count, then the match's atomics), 56 with
    s >= 33 (extras, the staged 32, then the match), and 57.  Slot 0 holds a reply to an address taught in a LATER buffer:
    a hit like the others, which the oracle scores -1 / -2."""
    total, s_lo, s_hi = SHARED[case]
    bench = benches()
    pool, place = bench.pool, MIDDLE
    teach = [(S.Pool.TEACH_AT[w], p) for w, p in enumerate(pool.teacher_p)]
    others = sum(pool.teacher)
    assert pool.reply[0] > 0 and pool.reply_alone[0] == 0

    def build():
        def make(want, salt):
            opts = S.without_slot([[o for o in opts if pool.reply_alone[q] == 0 or o[2][0] != "reply"]
                                   for q, opts in enumerate(pool.all_options())], salt)
            opts[0] = [(0, pool.reply[0], ("reply", 0))]
            ids = S.choose_slots(opts, lambda s, m: s + m == want and s_lo + 3 <= s <= s_hi - 3 and m >= 8 + pool.reply[0])
            return None if ids is None or ("reply", 0) not in ids else teach + S.tile_patches(pool, *place, ids)

        def count(patches):
            return (bench.meter.count(patches) - others, bench.scan_count(patches, place))
        made, got = S.settle(count, total, make, accept=lambda got: got[0] == total and s_lo <= got[1] <= s_hi)
        print(case, "records in the tile", got[0], "of them the scan's", got[1])
        return made
    streams = bench.streams(("shared", case), build)
    with context_17(bench) as c:
        small_leg(S.Device(c), bench.ref(oracle_mod), streams, total + others, overflows=total > S.TILE_BUCKET)


# ------------------------------------------------------------------------------------ leg 3: few hits on the score grid
@pytest.mark.parametrize("hits", [0, 1, S.SCORE_BLOCKS - 1, S.SCORE_BLOCKS, S.SCORE_BLOCKS + 1])
def test_few_hits_on_the_score_grid(hip_lib, oracle_mod, benches, hits):
    """0 hits (scored on the device all the same), 1 (255 blocks whose first >= n), and 255 / 256 / 257 (per = 1, 1, 2)."""
    bench = benches()
    pool = bench.pool
    streams = bench.streams(("few", hits), lambda: S.settle(bench.meter.count, hits, lambda want, salt: S.spread(pool, want, salt))[0])
    assert S.per_block(hits) == {0: 0, 1: 1, 255: 1, 256: 1, 257: 2}[hits]
    with context_17(bench) as c:
        small_leg(S.Device(c), bench.ref(oracle_mod), streams, hits)


# ------------------------------------------------------------------------------------ legs 4 to 6: many hits
class Large:
    """The templates (once per module) and, per context size, a meter, an ordinary dense pass and the composed streams."""

    def __init__(self, bench17):
        self.pool = bench17.pool
        t0 = time.perf_counter()
        self.templates = S.Templates(bench17.meter)
        print("templates: frames", self.templates.frames, "hits", self.templates.counts, "hits per frame",
              round(self.templates.hits_per_frame(), 3), "seconds", round(time.perf_counter() - t0, 2))
        self.meters, self.warm, self.made = {}, {}, {}

    def meter(self, n_buf):
        if n_buf not in self.meters:
            self.meters[n_buf] = S.Meter(n_buf)
        return self.meters[n_buf]

    def warm_up(self, n_buf):
        if n_buf not in self.warm:
            d = synth.make_iq_torch(n_buf * CHUNK, n_bursts=10 * n_buf, seed=0x5C1 + n_buf, n_icao=60, df11_every=4, device="cuda")
            self.warm[n_buf] = (d, d.cpu().numpy())
        return self.warm[n_buf]

    def stream(self, n_buf, lo, hi):
        """a stream of n_buf buffers whose pass has lo <= n_records <= hi: (device tensor, host samples, n_records, the
        groups of trials that straddle a block or round boundary of the score grid)"""
        if (n_buf, lo, hi) not in self.made:
            m = self.meter(n_buf)
            t0 = time.perf_counter()
            iq, n = S.settle(lambda iq: m.count_device(m.to_device(iq), n_buf * CHUNK), (lo + hi + 1) // 2,
                             lambda want, salt: S.compose(self.pool, self.templates, n_buf, want, salt),
                             accept=lambda got: lo <= got <= hi, tries=10)
            d = m.to_device(iq)
            rec = S.device_records(m.ctx, d.data_ptr(), n_buf * CHUNK)
            assert len(rec) == n, (len(rec), n)
            groups = S.straddling_groups(S.positions(rec))
            print(n_buf, "buffers:", n, "records, per", S.per_block(n), "rounds", S.rounds(n), "straddling groups", len(groups),
                  groups[:3], "seconds", round(time.perf_counter() - t0, 2))
            self.made[(n_buf, lo, hi)] = (d, iq, n, groups)
        return self.made[(n_buf, lo, hi)]

    def close(self):
        for m in self.meters.values():
            m.close()


@pytest.fixture(scope="module")
def large(benches):
    lg = Large(benches())
    yield lg
    lg.close()


def large_leg(dev, ref, t, w, n_buf, hits, flushes=False):
    """W blocking (the host's); flush, T W W W in flight; T collected: ordered and scored on the device, `hits` records;
    one more W into T's slot, everything collected, nothing replayed or sorted by the host.  flushes: an icao_flush in
    front of every pass (k_emit clears the retired exact bitmap beside its rounds)."""
    leg = Leg(dev, ref, {"T": t, "W": w}, n_buf * CHUNK)
    leg.flush()
    leg.blocking("W")
    before = dev.counters()
    for kind in "TWWW":
        if flushes or kind == "T":
            leg.flush()
        leg.submit(kind)
    on_device_path(leg.collect(), hits, dev, before, f"{n_buf} buffers in flight")
    if flushes:
        leg.flush()
    leg.submit("W")
    while leg.q:
        assert leg.collect()["retries"] == 0
    assert dev.counters() == before


ROUNDS = {"two rounds": (128, 65537, 65792, 2), "one full round": (128, 65536, 65536, 1), "three rounds": (256, 131073, 131328, 3)}


@pytest.mark.parametrize("case", list(ROUNDS))
def test_more_than_one_round(hip_lib, oracle_mod, large, case):
    """(a) 128 buffers, n in (65536, 65792]: per = 257, every full block's second round holds one hit.  (b) the same
    templates and pool trimmed to exactly 65536: one full round.  (c) 256 buffers, n in (131072, 131328]: three rounds."""
    from dump1090_rs_amd import Context
    n_buf, lo, hi, want_rounds = ROUNDS[case]
    d, iq, n, groups = large.stream(n_buf, lo, hi)
    assert lo <= n <= hi and S.rounds(n) == want_rounds and n <= S.score_cap(n_buf)
    assert any(g1 > g0 and g0 < m <= g1 for m, g0, g1 in groups), "no group of trials straddles a block or round boundary"
    with Context(0, n_buf) as c:
        large_leg(S.Device(c), OracleRef(oracle_mod), (d, iq), large.warm_up(n_buf), n_buf, n)


def test_two_rounds_with_a_flush_before_every_pass(hip_lib, oracle_mod, large):
    from dump1090_rs_amd import Context
    n_buf, lo, hi, _ = ROUNDS["two rounds"]
    d, iq, n, groups = large.stream(n_buf, lo, hi)
    assert groups and S.rounds(n) == 2
    with Context(0, n_buf) as c:
        large_leg(S.Device(c), OracleRef(oracle_mod), (d, iq), large.warm_up(n_buf), n_buf, n, flushes=True)


def test_two_rounds_with_a_filter_per_receiver(hip_lib, oracle_mod, large):
    """(a) with four receivers dealt over the buffers and device-side scoring of receivers passes on: k_rx_adders,
    k_score_rx and k_emit_rx share the bodies.  Against one oracle per receiver."""
    from dump1090_rs_amd import Context
    n_buf, lo, hi, _ = ROUNDS["two rounds"]
    d, iq, n, groups = large.stream(n_buf, lo, hi)
    assert groups and S.rounds(n) == 2
    receivers = np.arange(n_buf, dtype=np.uint32) % 4
    with Context(0, n_buf) as c:
        c.set_receivers(4)
        c.set_receiver_scoring(True)
        large_leg(S.Device(c, receivers=receivers), RxRef(oracle_mod, receivers), (d, iq), large.warm_up(n_buf), n_buf, n)
        counters = c.selftest_rx_score_counters()
        print(counters)
        assert counters["no_room"] == 0 and counters["refused"] == 0 and counters["taken"] >= 5


def test_the_cap(hip_lib, oracle_mod, large):
    """512 buffers: exactly 262144 hits are scored on the device; 262145 are replayed by the host -- and so is the pass that
    was in flight behind them (planned against a filter the replay has since changed: its epoch is over); the first pass
    submitted after that collect finds the exact bitmap invalid, rebuilds it and is scored on the device again
    (adsb_pass.cpp: plan_pass; adsb_collect.cpp: finish_pass)."""
    from dump1090_rs_amd import Context
    n_buf = 512
    cap = S.score_cap(n_buf)
    assert cap == S.SCORE_CAP_MAX
    at_cap, over = large.stream(n_buf, cap, cap), large.stream(n_buf, cap + 1, cap + 1)
    assert at_cap[2] == cap and over[2] == cap + 1 and at_cap[3] and S.rounds(cap) == 4
    w = large.warm_up(n_buf)
    with Context(0, n_buf) as c:
        dev = S.Device(c)
        leg = Leg(dev, OracleRef(oracle_mod), {"T": at_cap[:2], "U": over[:2], "W": w}, n_buf * CHUNK)
        leg.flush()
        leg.blocking("W")
        before = dev.counters()
        leg.flush()
        leg.submit("T")
        leg.submit("W")
        on_device_path(leg.collect(), cap, dev, before, "at the cap")
        on_device_path(leg.collect(), c.stats()["n_records"], dev, before, "behind it")
        leg.flush()
        leg.submit("U")
        leg.submit("W")
        st = leg.collect()
        assert st["n_records"] == cap + 1 and st["retries"] == 0, st
        assert dev.counters()[0] == before[0] + 1, (dev.counters(), before)
        leg.collect()                                    # (in flight while the host replayed: replayed too)
        assert dev.counters()[0] == before[0] + 2, (dev.counters(), before)
        after = dev.counters()
        leg.submit("W")
        on_device_path(leg.collect(), c.stats()["n_records"], dev, after, "after the rebuild")

"""What tests/test_gpu_profiling_levels.py shares: the probes that prove which profiling level a pass ran at, and the
streams of its scenarios with their expectations from the CPU oracle alone.  Every builder asserts that its scenario is
not vacuous (enough frames per pass, the planted frames where they belong, the score classes present), so the same
conditions can be checked without a GPU:  python -c "from tests import profiling_support as P; P.check_all()"

Nothing here compares the library with itself: a want is the oracle's (or, under error correction, signal statistics
and receivers, the restatement the neighbouring tests use)."""
import math
from functools import lru_cache

import numpy as np

from dump1090_rs_amd import synth
from tests.test_gpu_small_pass import ap_frame, want_key

CHUNK = 131072
TIMING = ("ms_scan", "ms_scan_exclusive", "ms_match", "ms_records", "ms_total_device")
LEVEL_CYCLE = (1, 2, 0, 2, 1, 0)


# ------------------------------------------------------------------------------------------------------ probes
def assert_level(c, level, what=""):
    """The timing fields of the call (or collect) that returned last say which level its passes ran at."""
    st = c.stats()
    t = {k: float(st[k]) for k in TIMING}
    assert all(math.isfinite(v) for v in t.values()), (what, t)
    if level == 0:
        assert all(v == 0.0 for v in t.values()), (what, t)
    elif level == 1:
        assert t["ms_scan"] > 0 and t["ms_match"] == 0.0 and t["ms_records"] == 0.0 and t["ms_total_device"] == 0.0, (what, t)
    else:
        assert t["ms_scan"] > 0 and t["ms_total_device"] > 0 and t["ms_match"] >= 0 and t["ms_records"] >= 0, (what, t)


def rematches(c) -> int:
    return int(c._L.adsb_host_rematches(c._h))


def replays(c) -> int:
    return int(c._L.adsb_host_replays(c._h))


class Probed:
    """A context as test_gpu_small_pass.ring_stream drives it, with the level's probe behind every collect (and, for a CU8
    ring, ring_acquire handing out that ring's buffer)."""

    def __init__(self, c, level, u8=False):
        self._c, self._level, self._u8 = c, level, u8

    def __getattr__(self, name):
        return getattr(self._c, name)

    def ring_acquire(self):
        return self._c.ring_acquire_u8() if self._u8 else self._c.ring_acquire()

    def collect(self, *a, **kw):
        out = self._c.collect(*a, **kw)
        assert_level(self._c, self._level, "collect")
        return out


def run_pipeline(c, n_passes, submit, depth, level, flush_before=(), keys=None):
    """submit(k) for k < n_passes with `depth` passes in flight, icao_flush in front of the passes named; the key lists
    of the passes in order.  The level's probe follows every collect."""
    from tests.test_gpu_small_pass import key
    keys = keys or (lambda msgs: [key(m) for m in msgs])
    got = []

    def collect():
        got.append(keys(c.collect(cap=1 << 17)))
        assert_level(c, level, ("pass", len(got) - 1))

    for k in range(n_passes):
        if c.pending() == depth:
            collect()
        if k in flush_before:
            c.icao_flush()
        submit(k)
    while c.pending():
        collect()
    assert len(got) == n_passes
    return got


# ------------------------------------------------------------------------------------------------------ pieces
def df4(icao, k=0):
    return ap_frame(bytes([0x20, 0x00, 0x05, 0x30 + k]), icao)


def df20(icao, k=0):
    return ap_frame(bytes([0xA0, 0x00, 0x05, 0x30, 1, 2, 3, 4, 5, 6, 7 + k]), icao)


def at(buf, j, phase=0):
    return 5 * (buf * CHUNK + j) + phase


def pool(k):
    """the address synth.plan_bursts gives aircraft k of its pool"""
    return 0xA00000 + k * 0x101


class Stream:
    """synth.make_iq at `per_buffer` bursts a buffer, and (replies) two address/parity replies per buffer for aircraft
    of its pool, so that a stream holds every score class: 750 / 1600 (DF11), 1400 / 1800 (DF17), 1000 (the replies).
    plant() adds a frame where no other burst is: a planted frame's fate is then the filter's alone."""
    SPAN = 300   # samples a burst covers, rounded up

    def __init__(self, n_samples, seed, per_buffer=30, n_icao=30, df11_every=4, replies=True):
        n_buf = -(-n_samples // CHUNK)
        plan = synth.plan_bursts(n_samples, per_buffer * n_buf, seed, n_icao, df11_every)
        self.iq = synth.noise_numpy(n_samples, seed)
        synth.add_bursts(self.iq, plan)
        self.taken = sorted(b.tick // 5 for b in plan)
        self.n_icao = n_icao
        if replies:
            for b in range(n_buf):
                self.plant(b, 11000 + 37 * b, df4(pool(b % n_icao), b % 8), b % 5, 21000)
                if b * CHUNK + 80000 + 91 * b < n_samples:   # (a ragged last buffer may end before it)
                    self.plant(b, 77000 + 91 * b, df20(pool((b + 7) % n_icao), b % 8), (b + 2) % 5, 19000)

    def window(self, a, z):
        """samples a .. z as a stream of its own (a copy: what is planted there stays there)"""
        w = object.__new__(Stream)
        w.iq, w.n_icao = np.array(self.iq[a:z]), self.n_icao
        w.taken = [t - a for t in self.taken if a - self.SPAN <= t < z]
        return w

    def free(self, s):
        import bisect
        k = bisect.bisect_left(self.taken, s - self.SPAN - 20)
        return k == len(self.taken) or self.taken[k] > s + self.SPAN + 20

    def plant(self, buf, j, frame, phase=0, amplitude=22000, step=40, reach=2400):
        """`frame` at the first free sample at or behind (step < 0: in front of) sample j of buffer `buf`, within
        `reach` samples; the sample (within the buffer) it went to."""
        import bisect
        for d in range(0, reach, abs(step)):
            s = buf * CHUNK + j + (d if step > 0 else -d)
            if 0 <= s and s + self.SPAN < len(self.iq) and self.free(s):
                synth.add_bursts(self.iq, [synth.Burst(5 * s + phase, amplitude, (buf + j) % 16, frame)])
                bisect.insort(self.taken, s)
                return s - buf * CHUNK
        raise AssertionError(("no room for a frame", buf, j))


def base_stream(n_samples, seed, **kw):
    return Stream(n_samples, seed, **kw).iq


def oracle_passes(oracle_mod, pieces, flush_before=(), orc=None):
    """One oracle stream over `pieces` (arrays), flushed in front of the pieces named: a list of want_key lists."""
    orc = orc or oracle_mod.Oracle()
    out = []
    for k, part in enumerate(pieces):
        if k in flush_before:
            orc.icao_flush()
        out.append([want_key(w) for w in orc.demod_iq(part, cap=1 << 17)[0]])
    return out


def scores(wants):
    return {w[3] for ws in wants for w in ws}


def assert_classes(wants, what=""):
    s = scores(wants)
    assert 1000 in s and 1400 in s and (1600 in s or 1800 in s), (what, sorted(s))


def passes_with(wants, frame, score=None):
    """the passes whose list holds `frame` (7 or 14 bytes), at `score` if given"""
    n = len(frame)
    return sorted({k for k, ws in enumerate(wants) for w in ws if bytes(w[4][:n]) == frame and (n == 14 or w[4][0] >> 7 == 0)
                   and (score is None or w[3] == score)})


def cut(iq, per):
    return [iq[a:a + per] for a in range(0, len(iq), per)]


def quantise(iq):
    from tests.test_gpu_u8 import quantise as q
    return q(iq)


def widen(raw):
    from tests.test_gpu_u8 import widen as w
    return w(raw)


# ------------------------------------------------------------------------------------------------------ 1. blocking
@lru_cache(maxsize=None)
def blocking(max_chunks):
    """(cs16, its want as one call, cu8, its want): max_chunks buffers and a ragged one of 70001 samples -- a blocking call
    a context of max_chunks cuts into two passes."""
    from oracle import binding
    n = max_chunks * CHUNK + 70001
    iq = base_stream(n, seed=7100 + max_chunks)
    raw = quantise(iq)
    want = [want_key(w) for w in binding.Oracle().demod_iq(iq, cap=1 << 17)[0]]
    want8 = [want_key(w) for w in binding.Oracle().demod_iq(widen(raw), cap=1 << 17)[0]]
    for w in (want, want8):
        assert len(w) > 20 * (max_chunks + 1), len(w)
        assert w[-1][0] == max_chunks                       # frames in the ragged buffer, i.e. in the second pass
        assert_classes([w], ("blocking", max_chunks))
    for a in (iq, raw):
        a.setflags(write=False)
    return iq, want, raw, want8


# ------------------------------------------------------------------------------------------------------ 2. pipeline full
A, B = 0x4B1A2C, 0x3C6589
N_PIPE = 24
PLANTED = {"early_a": 3, "teach_a": 5, "df4_a": 6, "df20_a": 7, "early_b": 10, "teach_b": 12, "df4_b": 13, "df20_b": 14}


@lru_cache(maxsize=None)
def planted(per_pass):
    """(iq, wants per pass): 24 passes of per_pass buffers (the last ragged) that keep teaching the filter; a DF4 for A
    before A is known, the DF17 that teaches A in pass 5, a DF4 / DF20 for A in passes 6 / 7; the same for B with the DF17
    in the last tile of pass 12's last buffer and the DF4 in the first tile of pass 13's first."""
    from oracle import binding
    n = N_PIPE * per_pass * CHUNK - 30001
    st = Stream(n, seed=7200 + per_pass)
    iq = st.iq
    first = lambda p: p * per_pass                 # noqa: E731
    last = lambda p: p * per_pass + per_pass - 1   # noqa: E731
    P = PLANTED
    st.plant(first(P["early_a"]), 50000, df4(A))
    st.plant(last(P["teach_a"]), 100000, synth.df17_frame(A, 7), 2)
    assert st.plant(first(P["df4_a"]), 300, df4(A), 1) < 7000
    st.plant(first(P["df20_a"]), 60000, df20(A), 3)
    st.plant(first(P["early_b"]), 40000, df4(B, 1), 4)
    assert st.plant(last(P["teach_b"]), 126000, synth.df17_frame(B, 9), 2, step=-40) > CHUNK - 7712     # the last tile
    assert st.plant(first(P["df4_b"]), 300, df4(B, 1), 1) < 7000                                         # the first tile
    st.plant(first(P["df20_b"]), 64000, df20(B, 1), 3)
    wants = oracle_passes(binding, cut(iq, per_pass * CHUNK))
    check_planted(wants)
    assert all(len(w) > 20 * per_pass for w in wants), [len(w) for w in wants]
    assert_classes(wants, ("planted", per_pass))
    iq.setflags(write=False)
    return iq, wants


def check_planted(lists):
    """the planted frames decode in exactly their passes, at score 1000 (`lists`: want_key / key tuples per pass)"""
    P = PLANTED
    assert passes_with(lists, df4(A)) == passes_with(lists, df4(A), 1000) == [P["df4_a"]]
    assert passes_with(lists, df20(A)) == passes_with(lists, df20(A), 1000) == [P["df20_a"]]
    assert passes_with(lists, df4(B, 1)) == passes_with(lists, df4(B, 1), 1000) == [P["df4_b"]]
    assert passes_with(lists, df20(B, 1)) == passes_with(lists, df20(B, 1), 1000) == [P["df20_b"]]
    assert passes_with(lists, synth.df17_frame(A, 7)) == [P["teach_a"]] and passes_with(lists, synth.df17_frame(B, 9)) == [P["teach_b"]]


# ------------------------------------------------------------------------------------------------------ 3. flushes
N_FLUSH = 20
FLUSH_SOME = (0, 5, 6, 13)
FLUSH_EVERY = tuple(range(N_FLUSH))


def taught(p):
    return 0x480000 + 0x1111 * (p % N_FLUSH)


@lru_cache(maxsize=None)
def flushed(per_pass, flush_before):
    """(iq, wants[rep][pass]) -- 20 passes, run twice over on one stream: pass p teaches taught(p) late in its last
    buffer, pass p + 1 holds a DF4 for it in its first tile and pass p + 2 one in the middle (wrapping into the next
    repetition), so every pass behind a flush needs what the flushed pass taught while that one is still in flight, and
    every flushed pass holds replies for addresses known only before the flush."""
    from oracle import binding
    n = N_FLUSH * per_pass * CHUNK - 4001
    st = Stream(n, seed=7300 + per_pass)
    iq = st.iq
    for p in range(N_FLUSH):
        st.plant(p * per_pass + per_pass - 1, 122000 - (4100 if p == N_FLUSH - 1 else 0), synth.df17_frame(taught(p), 100 + p), p % 5, step=-40)
        assert st.plant(p * per_pass, 2500, df4(taught(p - 1), 1), (p + 1) % 5) < 7000
        st.plant(p * per_pass, 64000, df4(taught(p - 2), 2), (p + 2) % 5)
    orc = binding.Oracle()
    pieces = cut(iq, per_pass * CHUNK)
    wants = [oracle_passes(binding, pieces, flush_before, orc) for rep in range(2)]
    for rep in range(2):
        ws = wants[rep]
        assert all(len(w) > 20 * per_pass for w in ws)
        for p in range(N_FLUSH):
            assert p in passes_with(ws, synth.df17_frame(taught(p), 100 + p)), p
            known1 = p not in flush_before and (p > 0 or rep > 0)
            known2 = known1 and p - 1 not in flush_before and (p > 1 or rep > 0)
            # ("known only before the flush": a flushed pass decodes neither reply; behind it the first one comes back)
            assert (p in passes_with(ws, df4(taught(p - 1), 1), 1000)) == known1, (rep, p)
            assert (p in passes_with(ws, df4(taught(p - 2), 2), 1000)) == known2, (rep, p)
    if flush_before == FLUSH_SOME:   # behind each flush the next pass needs the flushed pass's address (6 is flushed itself)
        assert all(f + 1 in passes_with(wants[0], df4(taught(f), 1), 1000) for f in (0, 6, 13))
        assert 6 not in passes_with(wants[0], df4(taught(5), 1))
        assert_classes(wants[0], "flushed")
    iq.setflags(write=False)
    return iq, wants


# ------------------------------------------------------------------------------------------------------ 4. the ring
N_RING = 13
RING_FLUSH = (0, 7)


@lru_cache(maxsize=None)
def ring(per_slot, u8=False):
    """(the stream as the slots take it, (slot,) + want_key per message): 13 slots of per_slot buffers, the last one
    ragged, flushes before slots 0 and 7 -- the shape of test_ring_slots_copied_in_front_of_their_pass.  Slots of 16 and
    20 buffers are windows of a 40-buffer stream (a buffer heard again scores differently: its aircraft are known)."""
    from oracle import binding
    if per_slot <= 3:
        stream = base_stream(N_RING * per_slot * CHUNK, seed=7400 + per_slot)
    else:
        base = base_stream(40 * CHUNK, seed=7400 + per_slot)
        stream = np.concatenate([base[s * CHUNK:(s + per_slot) * CHUNK] for s in ((7 * b) % (41 - per_slot) for b in range(N_RING))])
    stream = np.ascontiguousarray(stream[:(N_RING - 1) * per_slot * CHUNK + 31007])
    raw = quantise(stream) if u8 else stream
    meant = widen(raw) if u8 else stream
    wants = oracle_passes(binding, cut(meant, per_slot * CHUNK), RING_FLUSH)
    assert len(wants) == N_RING and sum(len(w) for w in wants) > 20 * N_RING * per_slot and all(len(w) > 3 for w in wants)
    assert_classes(wants, ("ring", per_slot, u8))
    raw.setflags(write=False)
    return raw, [(b,) + w for b, ws in enumerate(wants) for w in ws]


# ------------------------------------------------------------------------------------------------------ 5. magnitudes, carry-over
@lru_cache(maxsize=None)
def magnitudes():
    """[(data, length, want)] for adsb_demodulate2400 at lengths 131072 and 34915, a lead-in that is not zero, one oracle
    stream over both (the second buffer's replies need the first one's aircraft)."""
    from oracle import binding
    orc = binding.Oracle()
    out = []
    for length, seed in ((CHUNK, 7501), (34915, 7502)):
        iq = base_stream(length, seed=seed, per_buffer=40 if length == CHUNK else 10)
        data, n = orc.to_mag(iq)
        assert n == length
        data[3:40] = np.arange(37, dtype=np.uint16) * 911
        data[300:326] = 40000
        want = [want_key(w) for w in orc.demodulate2400(data, n)[0]]
        assert len(want) > (20 if length == CHUNK else 4)
        out.append((data, n, want))
    assert_classes([w for _, _, w in out], "magnitudes")
    return out


CARRY_N = 893685
CARRY_CUTS = {1: [131072, 200, 128072, 131072, 70000, 131072, 52, 131072, 131072, 40001],
              16: [262644, 200, 261072, 131072, 52, 70000, 100000, 40000, 20000, 8645]}
CARRY_ICAO = 0xABCDEF


def carry_bounds(max_chunks):
    b = np.cumsum([0] + CARRY_CUTS[max_chunks]).tolist()
    assert b[-1] == CARRY_N and all(x % 4 == 0 for x in b[:-1])
    return b


@lru_cache(maxsize=None)
def carry(max_chunks):
    """(iq, [want per call]) in carry-over mode: one stream cut into ten calls at awkward places (two of them shorter than
    the 326-sample lead-in), a DF17 across every call's end and across the buffer ends inside the calls."""
    from oracle import binding
    st = Stream(CARRY_N, seed=7551)
    iq = st.iq
    ends = sorted(set(carry_bounds(1)[1:-1] + carry_bounds(16)[1:-1] + [131072 + 262644]))
    placed = 0
    for e in ends:   # (a frame starts 30 .. 250 samples in front of the end it lies across, where there is room)
        try:
            st.plant(0, e - 30, synth.df17_frame(CARRY_ICAO, 500 + placed), placed % 5, 20000, step=-20, reach=230)
            placed += 1
        except AssertionError:
            pass
    assert placed >= 10, placed
    b = carry_bounds(max_chunks)
    orc, state = binding.Oracle(), np.zeros((326, 2), np.int16)
    wants = [[want_key(w) for w in binding.demod_iq_carry(orc, iq[a:z], state, cap=1 << 17)[0]] for a, z in zip(b[:-1], b[1:])]
    plain = oracle_passes(binding, [iq[a:z] for a, z in zip(b[:-1], b[1:])])
    ours = lambda lists: sum(1 for ws in lists for w in ws if w[4][1:4] == CARRY_ICAO.to_bytes(3, "big"))   # noqa: E731
    assert ours(wants) >= ours(plain) + 4, (ours(wants), ours(plain))     # frames only the carried lead-in recovers
    assert sum(len(w) for w in wants) > 20 * (CARRY_N // CHUNK)
    assert_classes(wants, "carry")
    iq.setflags(write=False)
    return iq, wants


# ------------------------------------------------------------------------------------------------------ 6. dense, device-scored
DENSE_N = 17
DENSE_ORDER = (0, 1, 2, 2, 0, 1)     # six passes over three captures; icao_flush before the first and the fourth


@lru_cache(maxsize=None)
def dense():
    """(captures, want of the priming call, wants of the six passes): 17-buffer captures of 40 bursts a buffer, replies in
    captures 1 and 2 for an aircraft only capture 0 teaches."""
    from oracle import binding
    caps = []
    for k in range(3):
        st = Stream(DENSE_N * CHUNK, seed=7600 + k, per_buffer=40, df11_every=3, replies=False)
        iq = st.iq
        if k == 0:
            st.plant(3, 5000, synth.df17_frame(A, 7), 2, 21000)
        else:
            for q in range(1, 6):
                st.plant(2 + q, 900 * q + 333, df4(A), q % 5, 21000)
        iq.setflags(write=False)
        caps.append(iq)
    orc = binding.Oracle()
    prime = [want_key(w) for w in orc.demod_iq(caps[2], cap=1 << 17)[0]]
    wants = oracle_passes(binding, [caps[k] for k in DENSE_ORDER], (0, 3), orc)
    assert all(len(w) >= 8 * DENSE_N for w in wants) and len(prime) >= 8 * DENSE_N
    assert passes_with(wants, df4(A), 1000) == [1, 2, 5] and not passes_with([prime], df4(A))   # (pass 3 comes behind the flush, in front of the DF17)
    assert {1000, 1400, 1600, 1800} <= scores(wants)
    return caps, prime, wants


@lru_cache(maxsize=None)
def dense_fix(mode):
    """(iq, wants of: the priming call, then four passes with a flush before the first and the third) -- the first 17
    buffers of fix_scored_support.order_stream under error-correction `mode`, from that module's restatement."""
    from tests import fix2_support as f2
    from tests import fix_scored_support as S
    iq = np.ascontiguousarray(S.order_stream()[0][:DENSE_N * CHUNK])
    r = f2.Restated(mode)
    wants = [r.demod_iq(iq)]
    for k in range(4):
        if k in (0, 2):
            r.icao_flush()
        wants.append(r.demod_iq(iq))
    assert all(len(w) >= 8 * DENSE_N for w in wants)
    assert sum(k[1] == 1200 for k in wants[1]) >= 20 and (mode != 3 or sum(k[1] == 1100 for k in wants[1]) >= 20)
    assert wants[1] != wants[2] and wants[1] == wants[3]           # the early copies come back once their aircraft is known
    iq.setflags(write=False)
    return iq, wants


# ------------------------------------------------------------------------------------------------------ 7. overflow
OVERFLOW_PERIOD = 1


@lru_cache(maxsize=None)
def overflowing(n_buf, u8=False, period=OVERFLOW_PERIOD):
    """(raw input, want): n_buf buffers of ordinary traffic in their first 40000 samples and one of test_gpu_parity's
    ADVERSARIAL_PERIODS from there to the end: several address/parity trials per position, many times what a pass's
    lists hold.  CU8: the bytes whose widened values are nearest."""
    from oracle import binding
    from tests.test_gpu_parity import ADVERSARIAL_PERIODS
    st = Stream(n_buf * CHUNK, seed=7700 + n_buf)
    iq = st.iq
    for b in range(n_buf):   # replies in the clean part for what the buffer before taught: the fallback must keep them
        st.plant(b, 30000, synth.df17_frame(taught(b), b), b % 5)
        st.plant(b, 35000, df20(taught(b), 6), (b + 1) % 5)
        for q in range(8):   # (weak first frames of new aircraft: where one trial phase alone slices them clean they score 1400)
            st.plant(b, 14000 + 1500 * q, synth.df17_frame(0x500000 + 0x333 * (8 * b + q), q), q % 5, 5200 + 600 * q)
        if b:
            st.plant(b, 3000, df4(taught(b - 1), 5), b % 5)
    amps = np.array(ADVERSARIAL_PERIODS[period], dtype=np.int16)
    for b in range(n_buf):
        a, z = b * CHUNK + 40000, (b + 1) * CHUNK
        iq[a:z, 0] = np.tile(amps, (z - a) // len(amps) + 1)[: z - a]
        iq[a:z, 1] = 0
    raw = quantise(iq) if u8 else iq
    meant = widen(raw) if u8 else iq
    want, stats = binding.Oracle().demod_iq(meant, cap=1 << 20)
    assert stats.quiet_pass > 10000 * n_buf, stats.quiet_pass        # (noise: ~1300 a buffer)
    want = [want_key(w) for w in want]
    assert len(want) > 8 * n_buf
    assert n_buf == 1 or passes_with([want], df4(taught(0), 5), 1000) == [0]
    assert_classes([want], "overflowing")
    raw.setflags(write=False)
    return raw, want


@lru_cache(maxsize=None)
def overflowing_magnitudes():
    """(data, length, want) of overflowing(1) as a caller's MagnitudeBuffer with a lead-in that is not zero"""
    from oracle import binding
    orc = binding.Oracle()
    data, n = orc.to_mag(overflowing(1)[0])
    data[3:40] = np.arange(37, dtype=np.uint16) * 911
    want = [want_key(w) for w in orc.demodulate2400(data, n, cap=1 << 18)[0]]
    assert len(want) > 2
    return data, n, want


@lru_cache(maxsize=None)
def aftermath(per_pass):
    """(iq, wants per pass): ten ordinary passes for the context an overflow fallback has been through"""
    from oracle import binding
    iq = base_stream(10 * per_pass * CHUNK, seed=7750 + per_pass)
    wants = oracle_passes(binding, cut(iq, per_pass * CHUNK), (0,))
    assert all(len(w) > 20 * per_pass for w in wants)
    assert_classes(wants, "aftermath")
    iq.setflags(write=False)
    return iq, wants


# ------------------------------------------------------------------------------------------------------ 8. receivers
RX_PASSES, RX_FLUSH_AT = 14, 7


@lru_cache(maxsize=None)
def receivers_pipeline(n):
    """(iq, passes, the receiver flushed in front of pass 7, wants, the model after the last pass): five receivers, 14
    passes of n buffers over windows of receivers_support.batch(3, 8), a map of its own per pass, the last pass ragged."""
    from tests import receivers_support as RS
    from tests.test_gpu_receivers import PER, expect_passes, random_maps
    n_receivers = 5
    iq, _ = RS.batch(3, PER[3])
    total = len(iq) // CHUNK
    maps = random_maps(n_receivers, [n] * RX_PASSES, 60 + n)
    passes = [((3 * k) % (total - n + 1), (3 * k) % (total - n + 1) + n, mp, 30001 if k == RX_PASSES - 1 else 0) for k, mp in enumerate(maps)]
    unflushed, _, _ = expect_passes(n_receivers, iq, passes)
    for flushed_rx in range(n_receivers):   # (the first receiver whose flush there changes what comes back)
        wants, shareds, model = expect_passes(n_receivers, iq, passes, before={RX_FLUSH_AT: [flushed_rx]})
        if wants != unflushed:
            break
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    assert wants != unflushed and wants[:RX_FLUSH_AT] == unflushed[:RX_FLUSH_AT]      # the flush shows in the results
    assert all(len(w) > 20 * n for w in wants)
    return iq, passes, flushed_rx, wants, model


@lru_cache(maxsize=None)
def receivers_dense():
    """(iq, maps, want of the priming call -- every buffer receiver 0 --, wants of four passes behind a flush, the model):
    three receivers over a dense 17-buffer capture."""
    from tests import receivers_support as RS
    from tests.test_gpu_receivers import expect_passes, random_maps
    from tests.test_gpu_receivers_scored import dense as dense_capture
    n_receivers, n = 3, DENSE_N
    iq = dense_capture(900, n, 60)
    maps = random_maps(n_receivers, [n] * 4, 19)
    wants, shareds, model = expect_passes(n_receivers, iq, [(0, n, mp, 0) for mp in maps])
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    prime = RS.Model(n_receivers).feed(iq, np.zeros(n, dtype=np.uint32))
    assert len(prime) >= 8 * n and all(len(w) >= 8 * n for w in wants)
    return iq, maps, prime, wants, model


# ------------------------------------------------------------------------------------------------------ 9. signal statistics
@lru_cache(maxsize=None)
def stats_stream():
    """18 buffers, the last one of 70001 samples: (iq, want of it as one blocking call)"""
    from oracle import binding
    iq = base_stream(17 * CHUNK + 70001, seed=7900)
    want = [want_key(w) for w in binding.Oracle().demod_iq(iq, cap=1 << 17)[0]]
    assert len(want) > 20 * 18
    assert_classes([want], "stats_stream")
    iq.setflags(write=False)
    return iq, want


def stats_windows(max_chunks):
    """(first buffer, buffers) of the passes submitted with the pipeline full: more passes than fit in flight, the sizes
    mixed; a context of 17 takes passes of 17 buffers among them"""
    sizes = {1: [1] * 10, 16: [1, 2, 3, 1, 16, 2, 1, 3, 2, 1], 17: [17, 1, 2, 17, 3, 1]}[max_chunks]
    return [((3 * k) % (18 - n), n) for k, n in enumerate(sizes)]


@lru_cache(maxsize=None)
def stats_expect(max_chunks):
    """{"call": records of the whole stream as one call, "submit": (pieces, wants, records per pass), "ring": the same for
    ten one-buffer slots, the last one ragged} -- the records from signal_support's restatement over the oracle's
    magnitudes, the frames from one oracle stream flushed in front of the first pass."""
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE as dt
    from oracle import binding
    from tests import signal_support as ss
    iq, _ = stats_stream()
    orc = binding.Oracle()
    out = {"call": ss.restated(orc, iq, iq, dt)}
    pieces = [iq[a * CHUNK:(a + n) * CHUNK - (1000 * k if n > 1 else 0)] for k, (a, n) in enumerate(stats_windows(max_chunks))]
    slots = cut(iq[:9 * CHUNK + 31007], CHUNK)
    for name, parts in (("submit", pieces), ("ring", slots)):
        wants = oracle_passes(binding, parts, (0,))
        assert all(len(w) > 20 * (len(part) // CHUNK) and len(w) > 3 for w, part in zip(wants, parts))
        out[name] = (parts, wants, [ss.restated(orc, part, part, dt) for part in parts])
    assert len({len(part) for part in pieces}) > 1 or max_chunks == 1
    return out


# ------------------------------------------------------------------------------------------------------ 10. shards
SHARD_ICAO = 0x4840D6


@lru_cache(maxsize=None)
def sharded():
    """(iq of 34 buffers, want as one stream, the DF4 that depends on the other shard): a DF17 in buffer 3 teaches an
    address that replies in buffers 1 (too early), 10, 20 and 30 need -- the last two in the second shard."""
    from oracle import binding
    st = Stream(34 * CHUNK, seed=8000, per_buffer=20)
    iq = st.iq
    reply = df4(SHARD_ICAO, 3)
    st.plant(1, 20000, reply)
    st.plant(3, 60000, synth.df17_frame(SHARD_ICAO, 77), 2)
    for b, j, ph in ((10, 90000, 1), (20, 5000, 3), (30, 70000, 4)):
        st.plant(b, j, reply, ph)
    want = [want_key(w) for w in binding.Oracle().demod_iq(iq, cap=1 << 17)[0]]
    assert sorted({w[0] for w in want if bytes(w[4][:7]) == reply}) == sorted({w[0] for w in want if bytes(w[4][:7]) == reply and w[3] == 1000}) == [10, 20, 30]
    assert len(want) > 10 * 34
    assert_classes([want], "sharded")
    iq.setflags(write=False)
    return iq, want, reply


# ------------------------------------------------------------------------------------------------------ 11. levels changing
N_CHANGE = 24
CHANGE_FLUSH = (0, 3, 8, 11, 12, 20)    # 3, 11: the last pass under a level; 8, 12, 20: the first under the next


def change_sizes(max_chunks):
    """buffers per pass: passes of 17 buffers under every level in the context that can take them"""
    if max_chunks == 17:
        return [17 if p % 4 == 1 else 1 + p % 2 for p in range(N_CHANGE)]
    return [1 if max_chunks == 1 else 1 + p % 3 for p in range(N_CHANGE)]


def change_address(g):
    return 0x3C0000 + 0x2222 * g


@lru_cache(maxsize=None)
def changing(max_chunks):
    """(pass inputs, wants): one stream of 24 passes, the level changing every four (LEVEL_CYCLE).  The last pass under a
    level teaches change_address(group) late; the first pass under the next level needs it in its first tile.  Flushes
    right before a change (in front of the teaching pass: the reply still decodes) and right after one (in front of the
    pass that needs it: it must not)."""
    from oracle import binding
    sizes = change_sizes(max_chunks)
    base = Stream(40 * CHUNK, seed=8100 + max_chunks)
    pieces = []
    for p, n in enumerate(sizes):
        s = (5 * p) % (41 - n)
        st = base.window(s * CHUNK, (s + n) * CHUNK - (1001 if p % 5 == 4 else 0))
        g = p // 4
        if p % 4 == 3:
            st.plant(n - 1, 120000, synth.df17_frame(change_address(g), 300 + g), p % 5, step=-40)
        if p % 4 == 0 and p:
            assert st.plant(0, 400, df4(change_address(g - 1), 4), p % 5) < 7000
        st.iq.setflags(write=False)
        pieces.append(st.iq)
    wants = oracle_passes(binding, pieces, CHANGE_FLUSH)
    assert all(len(w) > 20 * n for w, n in zip(wants, sizes))
    needs = {p: p in passes_with(wants, df4(change_address(p // 4 - 1), 4), 1000) for p in range(4, N_CHANGE, 4)}
    assert needs == {4: True, 8: False, 12: False, 16: True, 20: False}, needs
    assert_classes(wants, ("changing", max_chunks))
    return pieces, wants


def check_all():
    """Every stream above and its conditions, from the oracle alone (no GPU)."""
    import time
    todo = [(blocking, (m,)) for m in (1, 16, 17)] + [(planted, (n,)) for n in (1, 3)]
    todo += [(flushed, (n, f)) for n in (1, 2) for f in (FLUSH_SOME, FLUSH_EVERY)]
    todo += [(ring, (n, u8)) for n in (1, 2, 3, 16, 20) for u8 in (False, True)]
    todo += [(magnitudes, ()), (carry, (1,)), (carry, (16,)), (dense, ()), (dense_fix, (1,)), (dense_fix, (3,))]
    todo += [(overflowing, (n, u8)) for n in (1, 4) for u8 in (False, True)] + [(overflowing_magnitudes, ()), (aftermath, (1,)), (aftermath, (2,))]
    todo += [(receivers_pipeline, (1,)), (receivers_pipeline, (5,)), (receivers_dense, ())]
    todo += [(stats_stream, ()), (sharded, ())] + [(stats_expect, (m,)) for m in (1, 16, 17)] + [(changing, (m,)) for m in (1, 16, 17)]
    for f, args in todo:
        t0 = time.time()
        f(*args)
        print(f"{f.__name__}{args}: ok, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    check_all()

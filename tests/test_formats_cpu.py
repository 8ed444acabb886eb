"""Every Mode S downlink format and score class without a GPU (tests/formats_support.py): the frame builders, the
Python model of score_modes_message against the oracle's, the formats stream through the oracle, and the host replay
(adsb_replay_records, its single-bit repair form and the parallel replay) over the oracle's trials of that stream --
DF18 tags, residual 0 and repaired DF18s in the host code."""
import ctypes as C

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import fix_support as fs
from tests import formats_support as F

N_BUFFERS = 4


def oracle_checksum(O, frame: bytes) -> int:
    return int(O.orc_modes_checksum(frame, 8 * len(frame)))


def test_every_builder_leaves_the_residual_it_was_built_for(oracle_mod):
    O = oracle_mod.lib()
    r = np.random.default_rng(5)
    for _ in range(40):
        a = int(r.integers(0, 1 << 24))
        p = int(r.integers(0, 1 << 62))
        cases = [(F.ap_frame(df, a, p), a) for df in F.AP_SHORT + F.AP_LONG + F.COMM_D]
        cases += [(F.undefined_frame(df, a, p), a) for df in F.UNDEFINED]
        iid = int(r.integers(0, 128))
        bad = 0x80 << int(r.integers(0, 17))
        cases += [(F.df11_frame(a, iid, ca=int(r.integers(0, 8))), iid), (F.df11_frame(a, iid, bad_pi=bad), iid | bad)]
        for df in (17, 18):
            ca = int(r.integers(0, 8))
            f = F.es_frame(df, a, p, ca=ca)
            assert f[0] == (df << 3) | ca and int.from_bytes(f[1:4], "big") == a
            cases.append((f, 0))
        for f, want in cases:
            df = f[0] >> 3
            assert len(f) == (14 if df >= 16 else 7), f.hex()
            got = synth.crc24(f[:-3]) ^ int.from_bytes(f[-3:], "big")
            assert got == want == oracle_checksum(O, f) == F.crc_residual(f, 8 * len(f)), (f.hex(), want)
    assert oracle_checksum(O, F.ZERO14) == 0 and oracle_checksum(O, F.ZERO7_TAIL[:7]) == 0
    assert F.ZERO7_TAIL[0] >> 3 == 0 and all(F.ZERO7_TAIL[7:])
    # a value that folds onto a known address under a ^ (a >> 19) is another value
    for d in range(1, 32):
        v = F.folds_onto(0x4840D6, d)
        assert v != 0x4840D6 and F.fold(v) == F.fold(0x4840D6) and v < 1 << 24


def test_the_python_model_scores_like_the_oracle(oracle_mod):
    """The model (written from mod.rs / icao_filter.rs) and the oracle's orc_score_modes_message on one sequence of
    frames of every DF, each with a filter of its own: the same score every time and the same table slot for slot,
    through a full table (where address 0 still tests true: table B, icao_filter.rs:84-94)."""
    O = oracle_mod.lib()
    r = np.random.default_rng(11)
    pool = [int(x) for x in r.integers(1, 1 << 24, size=24)]
    orc, mine = oracle_mod.OrcFilter(), F.PyFilter()
    seen = {}

    def one(msg14):
        ln, sc = C.c_int(), C.c_int32()
        some = O.orc_score_modes_message(C.byref(orc), msg14, 14, C.byref(ln), C.byref(sc))
        got = F.score_modes_message(mine, msg14)
        assert (got is None) == (not some), msg14.hex()
        if got is not None:
            assert got == (ln.value, sc.value), (msg14.hex(), got, sc.value)
            seen[(msg14[0] >> 3, got[1])] = seen.get((msg14[0] >> 3, got[1]), 0) + 1

    def frames(a):
        p = int(r.integers(0, 1 << 62))
        out = [F.ap_frame(int(r.choice(F.AP_SHORT + F.AP_LONG + F.COMM_D)), a, p),
               F.ap_frame(int(r.choice(F.AP_SHORT + F.AP_LONG + F.COMM_D)), 0, p),
               F.undefined_frame(int(r.choice(F.UNDEFINED)), a, p), F.df11_frame(a, int(r.integers(0, 2)) * int(r.integers(0, 128))),
               F.df11_frame(a, 3, bad_pi=0x100), F.es_frame(int(r.choice([17, 18])), a, p), F.ZERO14, F.ZERO7_TAIL]
        return [f + bytes(r.integers(0, 256, 14 - len(f)).tolist()) if len(f) < 14 else f for f in out]

    for _ in range(1500):
        for f in frames(pool[int(r.integers(0, len(pool)))]):
            one(f)
    assert list(orc.a) == mine.a
    # fill the table with thousands of fresh addresses (DF17 and DF18 alike), on past full
    for k in range(5000):
        a = int(r.integers(1, 1 << 24))
        for f in frames(a)[:6]:
            one(f)
    assert list(orc.a) == mine.a and 0 not in mine.a
    one(F.ap_frame(0, 0, 77) + bytes(7))
    assert mine.test(0)
    for c in [(18, 1400), (18, 1800), (17, 1400), (17, 1800), (11, 750), (11, 1600), (11, 1000), (0, 1000)]:
        assert seen.get(c, 0) >= 20, (c, seen)
    assert sum(v for (df, s), v in seen.items() if df >= 24 and s == 1000) >= 20


def expected_classes(events, keys):
    """Check the first emission of every planned burst against the plan's model; (DF, score) counts of the bursts."""
    fe = F.first_emissions(events, keys)
    counts = {}
    for i, e in enumerate(events):
        if not e.whole or e.cls == "zero14":
            continue
        m = fe[i]
        if e.expect == ():
            assert m is None, (e.cls, e.sample, e.frame.hex(), m)
            continue
        assert m is not None and m[1] in e.expect, (e.cls, e.expect, e.sample, e.frame.hex(), m)
        key = (e.emits[0] >> 3, m[1]) if not e.cls.startswith("residual0") else ("residual0", e.emits[0] >> 3, m[1])
        counts[key] = counts.get(key, 0) + 1
    return counts


@pytest.mark.parametrize("seed", [1, 2])
def test_the_formats_stream_through_the_oracle(seed, oracle_mod):
    iq, events = F.formats_capture(seed, N_BUFFERS)
    F.assert_classes(events, N_BUFFERS)
    want, _ = oracle_mod.Oracle().demod_iq(iq)
    keys = [(w["buffer"], w["score"], w["j"], w["try_phase"], w["chunk"]) for w in want]
    # the model, fed the oracle's trials, emits what the oracle emits
    trials = np.concatenate([oracle_mod.all_trials(np.ascontiguousarray(iq[o:o + F.CHUNK]), c)[1]
                             for c, o in enumerate(range(0, len(iq), F.CHUNK))])
    assert F.model_demod(trials) == [(w["chunk"], w["j"], w["try_phase"], w["score"], w["buffer"]) for w in want]
    counts = expected_classes(events, keys)
    # nothing that was not sent
    sent = {e.emits for e in events}
    assert [k for k in keys if k[0] not in sent] == []
    # no undefined DF, no unknown DF11 IID, no AP reply of a DF18-only aircraft
    assert not any(k[0][0] >> 3 in F.UNDEFINED for k in keys)
    never = {e.emits for e in events if e.whole and e.expect == () and e.cls != "zero14"}
    assert not any(k[0] in never for k in keys)
    # the 14 zero bytes are sliced as such (the reference's None), and scored nowhere where they are
    zero = [e for e in events if e.cls == "zero14"]
    for e in zero:
        near = trials[(trials["chunk"].astype(np.int64) * F.CHUNK + (trials["j_tp"] & 0xFFFFFF) - F.LEAD >= e.sample - 2)
                      & (trials["chunk"].astype(np.int64) * F.CHUNK + (trials["j_tp"] & 0xFFFFFF) - F.LEAD <= e.sample + 2)]
        blank = {(int(t["chunk"]), int(t["j_tp"]) & 0xFFFFFF) for t in near if not bytes(t["msg"]).strip(b"\0")}
        assert blank, e.sample
        for pos in blank:
            at = [t for t in near if (int(t["chunk"]), int(t["j_tp"]) & 0xFFFFFF) == pos]
            if all(not any(bytes(t["msg"])[7:]) for t in at):   # every phase there is all zero: nothing to emit
                assert not any((k[4], k[2]) == pos for k in keys), pos
    # "7 zero bytes + tail": DF0, residual 0, 1000
    z7 = [m for i, m in F.first_emissions(events, keys).items() if events[i].cls == "zero7_tail"]
    assert len(z7) == N_BUFFERS and all(m is not None and m[0] == bytes(7) and m[1] == 1000 for m in z7)
    n = N_BUFFERS
    assert counts.get((18, 1400), 0) >= 8 * n and counts.get((18, 1800), 0) >= 8 * n
    assert counts.get((11, 1000), 0) >= 6 * n and counts.get((11, 1600), 0) >= 3 * n
    assert sum(v for k, v in counts.items() if len(k) == 2 and k[0] >= 24 and k[1] == 1000) >= 6 * n
    assert counts.get(("residual0", 0, 1000), 0) >= n
    assert sum(v for k, v in counts.items() if len(k) == 3 and k[2] == 1000) >= 6 * n
    assert sum(v for k, v in counts.items() if len(k) == 2 and k[0] in F.AP_LONG and k[1] == 1000) >= 6 * n


def oracle_records(iq, oracle_mod) -> np.ndarray:
    return np.concatenate([oracle_mod.all_trials(np.ascontiguousarray(iq[o:o + F.CHUNK]), c)[1]
                           for c, o in enumerate(range(0, len(iq), F.CHUNK))])


def parallel_replay(L, rec, mode, runs, parts, threads):
    from dump1090_rs_amd import _lib
    table = np.zeros(4096, dtype=np.uint32)
    cap = len(rec) + 8
    out, n, par = (_lib.AdsbMsg * cap)(), C.c_size_t(), C.c_int(-1)
    assert L.adsb_selftest_parallel_replay_fix(table.ctypes.data, np.ascontiguousarray(rec).ctypes.data, len(rec), runs,
                                               parts, threads, mode, out, cap, C.byref(n), C.byref(par)) == 0
    got = [(bytes(m.msg[: m.len]), int(m.score), int(m.j), int(m.try_phase), int(m.chunk), float(m.signal_level))
           for m in out[: n.value]]
    return got, table.tolist(), par.value


@pytest.mark.parametrize("fix", [False, True])
def test_the_host_replay_of_the_oracles_records(fix, oracle_mod):
    """The oracle's trials of the formats stream as adsb_trial records: adsb_replay_records (or its repair form) and the
    parallel replay at the parts and threads of test_host_sanitizers.py give the oracle's messages and the oracle's
    final filter table, DF18-tagged entries and their probe order included."""
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd.context import replay_records
    iq, events = F.formats_capture(3, N_BUFFERS, fix=fix)
    F.assert_classes(events, N_BUFFERS, fix=fix)
    rec = oracle_records(iq, oracle_mod)
    mode = 1 if fix else 0
    ref = fs.Restated(mode)
    want = ref.demod_iq(iq)
    want_table = list(ref.filter.a)
    if not fix:
        orc = oracle_mod.Oracle()
        assert want == [fs.okey(m) for m in [_as_msg(w) for w in orc.demod_iq(iq)[0]]]
        assert want_table == list(orc.filter.a)
    assert sum(v >> 25 == 1 for v in want_table) >= 7 * N_BUFFERS       # DF18-tagged entries: DF18-only, DF18 first
    if fix:
        fixed = [k for k in want if k[1] == 1200]
        assert sum(k[0][0] >> 3 == 18 for k in fixed) >= 6 * N_BUFFERS and sum(k[0][0] >> 3 == 17 for k in fixed) >= 3 * N_BUFFERS
        fe = F.first_emissions(events, want)
        for i, e in enumerate(events):
            if e.whole and e.cls.startswith("damaged"):
                m = fe[i] if e.expect else next((k for k in want if k[1] == 1200 and k[0] == e.emits and
                                                 abs(k[4] * F.CHUNK + k[2] - F.LEAD - e.sample) <= 2), None)
                assert (m is not None and m[1] == 1200) if e.expect else m is None, (e.cls, e.sample, m)
    table = np.zeros(4096, dtype=np.uint32)
    assert [fs.key(m) for m in replay_records(rec, table, mode=mode)] == want
    assert table.tolist() == want_table
    L = _lib.lib()
    went = set()
    for runs, parts, threads in ((1, 2, 2), (3, 7, 3), (8, 8, 4), (2, 33, 5)):
        got, t, par = parallel_replay(L, rec, mode, runs, parts, threads)
        assert got == want and t == want_table, (runs, parts, threads, par)
        went.add(par)
    assert 1 in went                         # (the parallel plan was taken, not refused)


def _as_msg(w):
    class M:
        pass
    m = M()
    m.msg, m.len, m.score, m.j, m.try_phase, m.chunk, m.signal_level = (
        w["msg"], w["len"], w["score"], w["j"], w["try_phase"], w["chunk"], w["signal_level"])
    return m

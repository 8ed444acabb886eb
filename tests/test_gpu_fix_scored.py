"""Device-side scoring and emission of repaired DF17/18 trials (k_score / k_emit under ADSB_FIX_1BIT / ADSB_FIX_2BIT):
a dense pass in a fix mode is scored where a mode-0 pass is.  Every result is compared with the CPU restatement
(tests/fix_restatement.c, tests/fix2_restatement.c) with tolerance 0, and adsb_host_replays / the adsb_multi counters
say who scored."""
import ctypes as C

import numpy as np
import pytest

from tests import fix2_support as f2
from tests import fix_scored_support as S
from tests import fix_support as fs
from tests import formats_support as F
from tests.test_gpu_fix import damaged_stream, quantise, widen

pytestmark = pytest.mark.gpu
CHUNK = fs.CHUNK
_cache = {}


def keys(msgs):
    return [fs.key(m) for m in msgs]


def host_replays(c):
    return int(c._L.adsb_host_replays(c._h))


def pairs():
    if "pairs" not in _cache:
        _cache["pairs"] = f2.pair_stream()
    return _cache["pairs"]


def ordered():
    if "order" not in _cache:
        _cache["order"] = S.order_stream()
    return _cache["order"]


def six_calls(c, d, iq, restated):
    """three blocking device-resident calls with an icao_flush before each, then three without: every one the
    restatement's; the host scored the first only"""
    got = []
    for call in range(6):
        if call < 3:
            c.icao_flush()
            restated.icao_flush()
        got.append(keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)))
        assert got[-1] == restated.demod_iq(iq), call
    assert host_replays(c) == 1, host_replays(c)      # the first call only (it told the context how dense the stream is)
    return got


def test_dense_pair_stream_is_repaired_and_scored_on_the_device(hip_lib):
    """All 5671 two-bit copies of a known DF17 and the one-bit, unknown-address and DF-bit extras, ~32 buffers through a
    context of 64: mode 3 repairs them on the device (adsb_host_replays stays at 1 over six calls -- it was 6 while a
    fix pass was the host's); mode 1 on the same stream must not bring a single two-bit copy back."""
    import torch
    from dump1090_rs_amd import Context
    iq, want = pairs()
    assert len(iq) > 16 * CHUNK
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, 64) as c:
        c.set_error_correction(f2.FIX2)
        got = six_calls(c, d, iq, f2.Restated(f2.FIX2))
        for g in got:
            f2.check_pair_stream(g, want)
    with Context(0, 64) as c:
        c.set_error_correction(1)
        got = six_calls(c, d, iq, f2.Restated(1))
        one = {s: g for s, (kind, g) in want.items() if kind == "1bit"}
        for g in got:
            assert not any(k[1] == 1100 for k in g)
            r1 = f2.repaired(g, 1200)
            # (a two-bit copy comes back only where another trial phase slices one of its two bits right)
            assert {s: b for s, b in r1.items() if want[s][0] == "1bit"} == one
            assert sum(want[s][0] == "2bit" for s in r1) <= 0.01 * len(f2.PAIRS)


def test_dense_single_bit_stream_is_scored_on_the_device(hip_lib):
    """40 buffers of fix_support.damaged_capture in mode 1: the restatement's list, nothing at 1100, one host replay."""
    import torch
    from dump1090_rs_amd import Context
    iq = damaged_stream(40, seed=9300)
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, 64) as c:
        c.set_error_correction(1)
        got = six_calls(c, d, iq, f2.Restated(1))
    for g in got:
        assert not any(k[1] == 1100 for k in g)
        assert sum(k[1] == 1200 for k in g) >= 100 * 40


def test_order_inside_a_pass(hip_lib):
    """Damaged copies BEFORE their aircraft's first clean frame of the pass are not repaired, those after it are; DF18,
    flips inside the address field and at bit 111, positions whose trial phases compete (tests/test_fix_scored_cpu.py
    checks from the restatement alone that the stream holds at least 20 of each)."""
    import torch
    from dump1090_rs_amd import Context
    iq, want = ordered()
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    for mode in (f2.FIX2, 1):
        r = f2.Restated(mode)
        with Context(0, 32) as c:
            c.set_error_correction(mode)
            c.icao_flush()
            assert keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)) == r.demod_iq(iq)   # (the host's: density unknown)
            for call in range(2):
                c.icao_flush()
                r.icao_flush()
                first = keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20))
                assert first == r.demod_iq(iq), (mode, call)
                second = keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20))
                assert second == r.demod_iq(iq), (mode, call)
                if mode == f2.FIX2:
                    S.check_first_call(first, want)
                    S.check_second_call(second, want)
            assert host_replays(c) == 1


@pytest.mark.parametrize("u8", [False, True])
def test_pipelined_passes_switching_modes(hip_lib, u8):
    """submit / collect, four dense passes of 20 buffers in flight, the mode changed 0 -> 1 -> 3 -> 0 between drained
    groups, one flush in the middle: each pass the restatement of its mode on one continuous filter, and after the pass
    that tells the context the stream is dense the host scores nothing."""
    import torch
    from dump1090_rs_amd import Context
    srcs = [ordered()[0], damaged_stream(20, seed=9400), pairs()[0][: 20 * CHUNK], damaged_stream(20, seed=9500)]
    if u8:
        raw = [quantise(s) for s in srcs]
        srcs = [widen(b) for b in raw]
    else:
        raw = srcs
    dev = [torch.from_numpy(b).cuda() for b in raw]
    torch.cuda.synchronize()
    r = f2.Restated(0)
    with Context(0, 32) as c:
        submit = c.submit_iq_device_u8 if u8 else c.submit_iq_device
        depth = c.max_in_flight()
        assert depth == 4
        c.icao_flush()
        submit(dev[0].data_ptr(), 20 * CHUNK)
        assert keys(c.collect(cap=1 << 20)) == r.demod_iq(srcs[0])
        assert host_replays(c) == 1
        for group, mode in enumerate((0, 1, f2.FIX2, 0)):
            c.set_error_correction(mode)
            r.mode = mode
            wants = []
            for k in range(depth):
                if group == 2 and k == 2:
                    c.icao_flush()
                    r.icao_flush()
                submit(dev[(group + k) % 4].data_ptr(), 20 * CHUNK)
                wants.append(r.demod_iq(srcs[(group + k) % 4]))
            for k in range(depth):
                assert keys(c.collect(cap=1 << 20)) == wants[k], (group, mode, k)
            assert c.pending() == 0
            if mode:
                assert sum(m[1] == 1200 for w in wants for m in w) >= 400
                assert (sum(m[1] == 1100 for w in wants for m in w) >= 400) == (mode == f2.FIX2)
        assert host_replays(c) == 1, host_replays(c)


def test_a_filter_about_to_fill_up_goes_back_to_the_host_in_fix_mode(hip_lib):
    """Thousands of distinct aircraft, no flush, until the 4096-slot table is within 64 of full and on past it, each pass
    with a buffer of damaged copies behind it, in mode 3: the device's result is dropped there, the host fetches the
    records (damaged bytes + residual, as k_emit left them) and repairs them itself."""
    import torch
    from dump1090_rs_amd import Context
    n_pass = 7
    host = [np.concatenate([F.fill_capture(500 + k, 20, per_buffer=60), fs.damaged_capture(9600 + k)[0]]) for k in range(n_pass)]
    r = f2.Restated(f2.FIX2)
    want = [r.demod_iq(h) for h in host]
    assert all(r.filter.a), "the table fills up"
    assert all(sum(m[1] == 1200 for m in w) >= 100 for w in want)
    bufs = [torch.from_numpy(h).cuda() for h in host]
    torch.cuda.synchronize()
    with Context(0, 32) as c:
        c.set_error_correction(f2.FIX2)
        c.icao_flush()
        got = [keys(c.demod_iq_device(bufs[0].data_ptr(), 21 * CHUNK, cap=1 << 20))]
        assert host_replays(c) == 1
        for k in range(1, n_pass):
            c.submit_iq_device(bufs[k].data_ptr(), 21 * CHUNK)
            if k >= 2:
                got.append(keys(c.collect(cap=1 << 20)))
        got.append(keys(c.collect(cap=1 << 20)))
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, k
        assert 2 <= host_replays(c) < n_pass, host_replays(c)     # some device-scored, the full table the host's


def test_a_small_pass_between_dense_ones_in_fix_mode(hip_lib):
    """A pass of three buffers is the host's (adsb_host_replays + 1): the device result of what is in flight is disowned,
    the exact bitmap rebuilt from the host's table, and the dense passes behind it are scored on the device again."""
    import torch
    from dump1090_rs_amd import Context
    iq, _ = ordered()
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    r = f2.Restated(f2.FIX2)
    with Context(0, 32) as c:
        c.set_error_correction(f2.FIX2)
        c.icao_flush()
        for _ in range(3):
            assert keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)) == r.demod_iq(iq)
        assert host_replays(c) == 1
        small = iq[5 * CHUNK: 8 * CHUNK]
        assert keys(c.demod_iq(small, cap=1 << 20)) == r.demod_iq(small)
        assert host_replays(c) == 2
        c.icao_flush()
        r.icao_flush()
        for _ in range(2):
            c.submit_iq_device(d.data_ptr(), len(iq))
        for _ in range(2):
            assert keys(c.collect(cap=1 << 20)) == r.demod_iq(iq)
        assert host_replays(c) == 2, host_replays(c)


@pytest.mark.parametrize("n_ctx", [1, 3])
def test_adsb_multi_scores_repairing_shards_on_their_devices(hip_lib, n_ctx):
    """Dense captures of 60 buffers over n contexts in modes 1 and 3: the shards are scored on their devices
    (device_scored_shards / scored_results_used rise; they stayed 0 while a fix shard was the host's), and with every
    scored result refused (score_mode 2) the records are fetched and host-repaired: the same list, the single stream's."""
    from dump1090_rs_amd.multi import MultiContext
    iq = np.concatenate([ordered()[0], damaged_stream(20, seed=9700), pairs()[0][: 20 * CHUNK]])
    for mode in (1, f2.FIX2):
        if ("multi", mode) not in _cache:
            r = f2.Restated(mode)
            _cache[("multi", mode)] = (r.demod_iq(iq), r.demod_iq(iq))
        fresh, known = _cache[("multi", mode)]
        assert sum(m[1] == 1200 for m in fresh) >= 2000 and (sum(m[1] == 1100 for m in fresh) >= 2000) == (mode == f2.FIX2)
        assert fresh != known
        for score_mode in (0, 2):
            with MultiContext([0] * n_ctx, 64 if n_ctx == 1 else 20) as m:
                m.set_error_correction(mode)
                m.selftest_tune(score_mode=score_mode)
                for want, flush in ((fresh, True), (known, False), (known, False), (fresh, True), (known, False)):
                    if flush:
                        m.icao_flush()
                    assert keys(m.demod_iq(iq, cap=1 << 20)) == want, (n_ctx, mode, score_mode)
                ctr = m.selftest_counters()
                assert ctr["device_scored_shards"] >= 2 * n_ctx, ctr
                if score_mode == 0:
                    assert ctr["scored_results_used"] >= 2 * n_ctx and ctr["scored_results_refused"] == 0, ctr
                else:
                    assert ctr["scored_results_used"] == 0 and ctr["scored_results_refused"] >= 2 * n_ctx, ctr


@pytest.mark.parametrize("mode", [1, f2.FIX2])
def test_adsb_multi_reading_learned_addresses_out_of_records_in_fix_mode(hip_lib, mode):
    """A fresh list cut to two addresses: every shard reads the addresses it can add out of its records, where a repairable
    DF17 is a record too.  Shard 0 (the ordered stream) holds damaged copies whose sliced address is a one-bit neighbour of
    LATE or EARLY; shards 1 and 2 hold, for each of those neighbours, damaged copies, then its first clean frame, then
    more copies.  Device-scored shards take the exchanged lists for "in the filter", so a damaged address among them
    would repair the copies in front of the clean frame: the restatement's list says they are not."""
    from dump1090_rs_amd.multi import MultiContext
    victims = S.damaged_addresses()
    parts = [ordered(), S.victim_stream(9900, victims[:24]), S.victim_stream(9950, victims[24:])]
    iq = np.concatenate([p[0] for p in parts])
    r = f2.Restated(mode)
    fresh, known = r.demod_iq(iq), r.demod_iq(iq)
    S.check_victims(fresh, parts[1][1], S.N_BUFFERS, mode)
    S.check_victims(fresh, parts[2][1], 2 * S.N_BUFFERS, mode)
    with MultiContext([0] * 3, 20) as m:
        m.set_error_correction(mode)
        m.selftest_tune(fresh_cap=2)
        for call, (want, flush) in enumerate(((fresh, True), (fresh, True), (known, False), (fresh, True), (known, False))):
            if flush:
                m.icao_flush()
            assert keys(m.demod_iq(iq, cap=1 << 20)) == want, (mode, call)
        ctr = m.selftest_counters()
        assert ctr["fresh_list_fallbacks"] >= 3 and ctr["device_scored_shards"] >= 3 and ctr["scored_results_used"] >= 3, ctr
        assert ctr["scored_results_refused"] == 0, ctr


def test_the_lookup_exhaustively(hip_lib, oracle_mod):
    """adsb_selftest_fix_lookup -- the device function k_score and k_emit repair with -- over all 107 single syndromes,
    all 5671 pair syndromes, zero and 4096 seeded non-syndromes, in modes 0, 1 and 3.  Expected values from the
    restatement's pair list and adsb_selftest_fix_table, both cross-checked against the oracle's CRC here."""
    from dump1090_rs_amd import Context
    O = oracle_mod.lib()
    syn = []
    for b in range(112):
        e = bytearray(14)
        e[b >> 3] = 0x80 >> (b & 7)
        syn.append(int(O.orc_modes_checksum(bytes(e), 112)))
    table = (C.c_uint32 * 112)()
    assert hip_lib.adsb_selftest_fix_table(table) == 0 and list(table) == syn
    pair_syn = (C.c_uint32 * 5671)()
    assert f2.restatement().fix2_pair_syndromes(pair_syn) == 5671
    assert list(pair_syn) == [syn[a] ^ syn[b] for a, b in f2.PAIRS]
    singles, doubles = set(syn[5:]), set(pair_syn)
    assert len(singles) == 107 and len(doubles) == 5671 and not singles & doubles and 0 not in singles | doubles
    rng = np.random.default_rng(9800)
    others = [int(v) for v in rng.integers(1, 1 << 24, size=8192) if int(v) not in singles and int(v) not in doubles][:4096]
    assert len(others) == 4096
    # (the syndromes of the DF bits 0..4 and of pairs that touch them are no repair either)
    df_bits = [syn[b] for b in range(5)] + [syn[a] ^ syn[b] for a in range(5) for b in range(a + 1, 112)]
    df_bits = [v for v in df_bits if v not in singles and v not in doubles]
    residuals = np.array(syn[5:] + list(pair_syn) + [0] + others + df_bits, dtype=np.uint32)
    none = 0xFFFF
    want1 = [0xFF | b << 8 for b in range(5, 112)]
    want2 = [a | b << 8 for a, b in f2.PAIRS]
    rest = [none] * (1 + len(others) + len(df_bits))
    with Context(0, 32) as c:
        assert list(c.selftest_fix_lookup(residuals, 3)) == want1 + want2 + rest
        assert list(c.selftest_fix_lookup(residuals, 1)) == want1 + [none] * 5671 + rest
        assert list(c.selftest_fix_lookup(residuals, 0)) == [none] * len(residuals)
        assert list(c.selftest_fix_lookup(residuals[:0], 3)) == []
        out = (C.c_uint32 * 4)()
        assert hip_lib.adsb_selftest_fix_lookup(c._h, residuals.ctypes.data, 4, 2, out) == -1      # ADSB_ERR_INVALID
        assert hip_lib.adsb_selftest_fix_lookup(c._h, None, 4, 3, out) == -1
    with Context(0, 1) as c:    # (a context for passes of a few buffers carries the same tables)
        assert list(c.selftest_fix_lookup(residuals, 3)) == want1 + want2 + rest

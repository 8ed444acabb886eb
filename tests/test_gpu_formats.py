"""Every Mode S downlink format and score class through the device (tests/formats_support.py): DF18 with and without
its plain address known, DF11 with IID != 0 and a bad PI, Comm-D, address/parity replies known, unknown, of DF18-only
aircraft and folding onto known addresses, undefined DFs, residual 0 and the all-zero edges -- in every buffer, over
tile seams and buffer edges, through every path the library has, against the oracle (or the restatement of
single-bit repair, tests/fix_restatement.c) with tolerance 0."""
import subprocess
import sys

import numpy as np
import pytest

from tests import fix_support as fs
from tests import formats_support as F
from tests.test_gpu_fix import quantise, widen

pytestmark = pytest.mark.gpu
CHUNK = F.CHUNK


def keys(msgs):
    return [fs.key(m) for m in msgs]


def okeys(ws):
    return [(w["buffer"], w["score"], w["j"], w["try_phase"], w["chunk"], w["signal_level"]) for w in ws]


def host_replays(c):
    return int(c._L.adsb_host_replays(c._h))


@pytest.mark.parametrize("max_chunks, n_buffers", [(1, 3), (16, 16), (64, 40), (512, 40)])
def test_blocking_host_and_device_resident(hip_lib, oracle_mod, max_chunks, n_buffers):
    """One-launch passes with folded supersets (1, 16 buffers) and three-launch passes with full bitmaps (64, 512);
    each twice, so that the dense stream's second passes are ordered and scored on the device (k_score / k_emit)."""
    import torch
    from dump1090_rs_amd import Context
    iq, events = F.formats_capture(100 + max_chunks, n_buffers)
    F.assert_classes(events, n_buffers)
    want = okeys(oracle_mod.Oracle().demod_iq(iq, cap=1 << 20)[0])
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, max_chunks) as c:
        calls = 0
        for run in range(2):
            c.icao_flush()
            assert keys(c.demod_iq(iq, cap=1 << 20)) == want, ("host", run)
            c.icao_flush()
            assert keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)) == want, ("device", run)
            calls += 2
        if max_chunks > 16:
            assert host_replays(c) < calls, host_replays(c)      # at least one pass was scored on the device


@pytest.mark.parametrize("max_chunks, per_pass", [(1, 1), (2, 2), (17, 17)])
def test_both_orders_across_pipelined_passes_and_the_ring(hip_lib, oracle_mod, max_chunks, per_pass):
    """Aircraft heard by DF18 in one pass and by DF17 in the next, and the other way round, through submit / collect
    at depth 1, 4 and 8 and through the ring, with an icao_flush between two passes."""
    import torch
    from dump1090_rs_amd import Context
    n_pass = 9
    iq, events = F.formats_capture(200 + per_pass, n_pass * per_pass, extra=F.cross_pass(n_pass, per_pass))
    F.assert_classes(events, n_pass * per_pass)
    assert sum(e.cls == "x_df18" for e in events) >= 4 * n_pass and sum(e.cls == "y_df17" for e in events) >= 4 * (n_pass // 2)
    cuts = [k * per_pass * CHUNK for k in range(n_pass + 1)]
    flush_before = {5}
    orc = oracle_mod.Oracle()
    wants = []
    for k, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
        if k in flush_before:
            orc.icao_flush()
        wants.append(okeys(orc.demod_iq(iq[a:z], cap=1 << 20)[0]))
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, max_chunks) as c:
        for depth in sorted({1, min(4, c.max_in_flight()), min(8, c.max_in_flight())}):
            c.icao_flush()
            got = []
            for k, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
                if c.pending() == depth:
                    got.append(keys(c.collect(cap=1 << 20)))
                if k in flush_before:
                    c.icao_flush()
                c.submit_iq_device(d.data_ptr() + 4 * a, z - a)
            while c.pending():
                got.append(keys(c.collect(cap=1 << 20)))
            assert got == wants, depth
        c.icao_flush()
        c.ring_create(per_pass * CHUNK)
        got = []
        for k, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
            if c.pending() == min(4, c.max_in_flight()):
                got.append(keys(c.collect(cap=1 << 20)))
            if k in flush_before:
                c.icao_flush()
            buf = c.ring_acquire()
            buf[: z - a] = iq[a:z]
            c.ring_submit(z - a)
        while c.pending():
            got.append(keys(c.collect(cap=1 << 20)))
        assert got == wants


def test_cu8_and_carry_over(hip_lib, oracle_mod):
    import torch
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    iq, events = F.formats_capture(300, 8)
    F.assert_classes(events, 8)
    b = quantise(iq)
    want8 = okeys(oracle_mod.Oracle().demod_iq(widen(b), cap=1 << 20)[0])
    d8 = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    with Context(0, 16) as c:
        c.icao_flush()
        assert keys(c.demod_iq_u8(b, cap=1 << 20)) == want8
        c.icao_flush()
        assert keys(c.demod_iq_device_u8(d8.data_ptr(), len(b), cap=1 << 20)) == want8
    # carry-over, buffer by buffer: the frames across every buffer end are found in the next one
    orc = oracle_mod.Oracle()
    carry = np.zeros((326, 2), np.int16)
    with Context(0, 1) as c:
        c.set_carry_over(True)
        c.icao_flush()
        edge = {e.frame for e in events if e.cls == "edge" and not e.whole}
        found = set()
        for a in range(0, len(iq), CHUNK):
            want = okeys(demod_iq_carry(orc, iq[a:a + CHUNK], carry, cap=1 << 20)[0])
            got = keys(c.demod_iq(iq[a:a + CHUNK], cap=1 << 20))
            assert got == want, a // CHUNK
            found |= {k[0] for k in got} & edge
        assert len(found) >= 5


def test_an_overfull_buffer_of_every_format_falls_back_and_stays_exact(hip_lib, oracle_mod):
    """One buffer of back-to-back frames of every class inside a dense stream: its bucket overflows, the pass is redone
    buffer by buffer (k_scan_simple classifies the trials), identical to the oracle, the passes around it unaffected."""
    import torch
    from dump1090_rs_amd import Context
    host = [F.formats_capture(400 + k, 20)[0] for k in range(3)]
    host[1][5 * CHUNK:6 * CHUNK] = F.packed_buffer(401)
    orc = oracle_mod.Oracle()
    want = [okeys(orc.demod_iq(h, cap=1 << 20)[0]) for h in host]
    assert sum(w[4] == 5 for w in want[1]) >= 250
    assert {w[0][0] >> 3 for w in want[1] if w[4] == 5} >= {0, 4, 5, 11, 16, 17, 18, 20, 21} | {24, 25, 26, 27}
    bufs = [torch.from_numpy(h).cuda() for h in host]
    torch.cuda.synchronize()
    with Context(0, 32) as c:
        c.icao_flush()
        got = [keys(c.demod_iq_device(bufs[0].data_ptr(), 20 * CHUNK, cap=1 << 20))]
        c.submit_iq_device(bufs[1].data_ptr(), 20 * CHUNK)
        c.submit_iq_device(bufs[2].data_ptr(), 20 * CHUNK)
        got.append(keys(c.collect(cap=1 << 20)))
        assert c.stats()["retries"] >= 1
        got.append(keys(c.collect(cap=1 << 20)))
        assert got == want


def test_filling_the_table_with_df18_and_df17_aircraft(hip_lib, oracle_mod):
    """Thousands of distinct DF17 and DF18-only aircraft, no flush, until the 4096-slot table is full and on past it:
    identical to the oracle through the device -> host hand-over and after.  Residual-0 replies keep scoring 1000
    with the table full: icao_filter_test(0) finds the empty slot of table B (src/icao_filter.rs:84-94)."""
    import torch
    from dump1090_rs_amd import Context
    n_pass = 7
    host = [F.fill_capture(500 + k, 20, per_buffer=60) for k in range(n_pass)]
    orc = oracle_mod.Oracle()
    want = []
    full_at = None
    for k, h in enumerate(host):
        want.append(okeys(orc.demod_iq(h, cap=1 << 20)[0]))
        if full_at is None and all(orc.filter.a):
            full_at = k
    assert full_at is not None and full_at < n_pass - 1, full_at
    assert sum(v >> 25 == 1 for v in orc.filter.a) > 1000                         # DF18-tagged entries
    after = [w for ws in want[full_at + 1:] for w in ws]
    assert sum(w[0] == bytes(7) or (w[1] == 1000 and F.crc_residual(w[0], 8 * len(w[0])) == 0) for w in after) >= 50
    assert sum(w[0][0] >> 3 == 18 and w[1] == 1400 for w in after) > 200
    bufs = [torch.from_numpy(h).cuda() for h in host]
    torch.cuda.synchronize()
    with Context(0, 32) as c:
        c.icao_flush()
        got = [keys(c.demod_iq_device(bufs[0].data_ptr(), 20 * CHUNK, cap=1 << 20))]
        assert host_replays(c) == 1
        for k in range(1, n_pass):
            c.submit_iq_device(bufs[k].data_ptr(), 20 * CHUNK)
            if k >= 2:
                got.append(keys(c.collect(cap=1 << 20)))
        got.append(keys(c.collect(cap=1 << 20)))
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, k
        assert 2 <= host_replays(c) < n_pass, host_replays(c)     # some device-scored, the full table the host's


@pytest.mark.parametrize("n_ctx, per, score_mode", [(2, 17, 0), (2, 17, 1), (4, 4, 0), (4, 4, 1)])
def test_adsb_multi_parallel_replay_and_filter_table(hip_lib, oracle_mod, n_ctx, per, score_mode):
    """adsb_multi over [0] * n: captures scored by several host threads (ParallelReplay, parallel_min 1), shards scored
    on their devices or not; the filter table equals the oracle's slot for slot, DF18-tagged entries included."""
    from dump1090_rs_amd.multi import MultiContext
    caps = [F.formats_capture(600 + k, n_ctx * per, extra=F.cross_pass(1, n_ctx * per, first_pass=k))[0] for k in range(3)]
    orc = oracle_mod.Oracle()
    wants = [okeys(orc.demod_iq(iq, cap=1 << 20)[0]) for iq in caps]
    want_table = list(orc.filter.a)
    assert sum(v >> 25 == 1 for v in want_table) >= 7 * n_ctx * per
    with MultiContext([0] * n_ctx, per) as m:
        m.selftest_tune(parallel_min=1, score_mode=score_mode)
        m.icao_flush()
        assert keys(m.demod_iq(caps[0], cap=1 << 20)) == wants[0]
        m.submit_iq(caps[1])
        m.submit_iq(caps[2])
        assert keys(m.collect(cap=1 << 20)) == wants[1]
        assert keys(m.collect(cap=1 << 20)) == wants[2]
        assert list(m.filter_table()) == want_table
        assert m.selftest_counters()["parallel_scored_captures"] > 0


@pytest.mark.parametrize("max_chunks, n_buffers", [(1, 2), (16, 6), (64, 20)])
def test_single_bit_repair_of_df18(hip_lib, max_chunks, n_buffers):
    """ADSB_FIX_1BIT: damaged DF18s (bits 5..111) of aircraft known by DF17 / DF11 come back at 1200 with the corrected
    bytes, those of DF18-only aircraft do not (the plain address is tested), copies in front of the aircraft's first
    clean frame (same buffer, tile, pass) and two-bit copies never; blocking, pipelined and one-launch passes."""
    import torch
    from dump1090_rs_amd import Context
    iq, events = F.formats_capture(700 + max_chunks, n_buffers, fix=True)
    F.assert_classes(events, n_buffers, fix=True)
    want = fs.Restated(1).demod_iq(iq)
    fe = F.first_emissions(events, want)
    repaired = 0
    for i, e in enumerate(events):
        if e.whole and e.cls.startswith("damaged"):
            near = [k for k in want if k[1] == 1200 and k[0] == e.emits and abs(k[4] * CHUNK + k[2] - F.LEAD - e.sample) <= 2]
            if e.expect:   # (a copy the noise damages once more is not repairable: nearly all are)
                repaired += fe[i] is not None and fe[i][1] == 1200
            else:
                assert not near, (e.cls, e.sample)
    assert repaired >= 0.9 * sum(e.whole and e.cls.startswith("damaged") and e.expect != () for e in events)
    assert sum(k[1] == 1200 and k[0][0] >> 3 == 18 for k in want) >= 6 * n_buffers
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, max_chunks) as c:
        c.set_error_correction(1)
        c.icao_flush()
        assert keys(c.demod_iq(iq, cap=1 << 20)) == want
        c.icao_flush()
        assert keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)) == want
        # pipelined, a pass per buffer (or per max_chunks buffers), the filter carried along
        step = max_chunks * CHUNK
        r = fs.Restated(1)
        wants = [r.demod_iq(iq[a:a + step]) for a in range(0, len(iq), step)]
        c.icao_flush()
        got = []
        for a in range(0, len(iq), step):
            if c.pending() == min(4, c.max_in_flight()):
                got.append(keys(c.collect(cap=1 << 20)))
            c.submit_iq_device(d.data_ptr() + 4 * a, min(step, len(iq) - a))
        while c.pending():
            got.append(keys(c.collect(cap=1 << 20)))
        assert got == wants


def test_randomised_soak_of_formats_and_repair(hip_lib, oracle_mod):
    """tests/fuzz_gpu.py --formats --fix: every frame kind in the random captures of every entry point, and a third of
    the single-context cases under ADSB_FIX_1BIT against the restatement."""
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "fuzz_gpu.py"), "--cases", "150", "--seed", "31", "--dense", "10",
                        "--mixed", "20", "--multi", "15", "--formats", "--fix", "0.3"],
                       capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "150 cases identical" in r.stdout and "dense_pipeline=10" in r.stdout and "mixed_pipeline=20" in r.stdout
    assert "multi=15" in r.stdout and "formats=on" in r.stdout
    fixed = int(r.stdout.split("fix_cases=")[1].split(",")[0].split()[0])
    assert fixed >= 25, r.stdout[-500:]

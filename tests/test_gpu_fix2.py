"""Two-bit repair of DF17/18 (ADSB_FIX_2BIT) on the device: every path the mode reaches, each compared with the CPU
restatement (tests/fix2_restatement.c) with tolerance 0; every two-bit copy of a known DF17 comes back."""
import subprocess

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import fix2_support as f2
from tests import fix_support as fs
from tests.test_gpu_fix import damaged_stream, quantise, widen
from tests.test_gpu_parity import ADVERSARIAL_PERIODS

pytestmark = pytest.mark.gpu
CHUNK = f2.CHUNK
FIX2 = f2.FIX2
_cache = {}


def keys(msgs):
    return [fs.key(m) for m in msgs]


def stream():
    """(iq, want, restated mode-3 keys) of the full pair stream, built once"""
    if "pairs" not in _cache:
        iq, want = f2.pair_stream()
        _cache["pairs"] = (iq, want, f2.Restated(FIX2).demod_iq(iq))
    return _cache["pairs"]


def mixed(n_buffers, seed):
    """damaged_capture buffers (one-bit copies, unknown aircraft) followed by the first buffers of the pair stream"""
    return np.concatenate([damaged_stream(n_buffers, seed), stream()[0][: n_buffers * CHUNK]])


@pytest.mark.parametrize("max_chunks", [1, 32])
def test_every_two_bit_copy_of_a_known_aircraft_comes_back(hip_lib, max_chunks):
    import torch
    from dump1090_rs_amd import Context
    iq, want, restated = stream()
    f2.check_pair_stream(restated, want)
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, max_chunks) as c:
        c.set_error_correction(FIX2)
        assert c.error_correction == FIX2
        c.icao_flush()
        got = keys(c.demod_iq(iq, cap=1 << 20))
        assert got == restated
        c.icao_flush()
        assert keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)) == restated
    f2.check_pair_stream(got, want)


@pytest.mark.parametrize("max_chunks, n_buffers", [(1, 2), (16, 6)])
def test_blocking_host_and_device_cs16_and_cu8(hip_lib, max_chunks, n_buffers):
    import torch
    from dump1090_rs_amd import Context
    iq = mixed(n_buffers, 8200)
    b = quantise(iq)
    wide = widen(b)
    d = torch.from_numpy(iq).cuda()
    d8 = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    want, want8 = f2.Restated(FIX2).demod_iq(iq), f2.Restated(FIX2).demod_iq(wide)
    assert sum(k[1] == 1100 for k in want) >= 100 * n_buffers
    with Context(0, max_chunks) as c:
        c.set_error_correction(FIX2)
        for run in range(2):
            c.icao_flush()
            assert keys(c.demod_iq(iq, cap=1 << 20)) == want, run
            c.icao_flush()
            assert keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)) == want, run
            c.icao_flush()
            assert keys(c.demod_iq_u8(b, cap=1 << 20)) == want8, run
            c.icao_flush()
            assert keys(c.demod_iq_device_u8(d8.data_ptr(), len(b), cap=1 << 20)) == want8, run


def test_modes_switch_between_passes(hip_lib):
    from dump1090_rs_amd import Context
    iq = mixed(3, 8300)
    with Context(0, 8) as c:
        for mode in (0, FIX2, 1, 0):
            c.set_error_correction(mode)
            c.icao_flush()
            assert keys(c.demod_iq(iq, cap=1 << 20)) == f2.Restated(mode).demod_iq(iq), mode
        assert c._L.adsb_set_error_correction(c._h, 2) == -1   # ADSB_ERR_INVALID
        assert c.error_correction == 0


@pytest.mark.parametrize("max_chunks, per_pass, u8", [(1, 1, False), (16, 4, False), (16, 4, True)])
def test_submit_collect_and_ring(hip_lib, max_chunks, per_pass, u8):
    import torch
    from dump1090_rs_amd import Context
    with Context(0, max_chunks) as c:
        c.set_error_correction(FIX2)
        depth = c.max_in_flight()
        n_pass = depth + 2
        iq = mixed((n_pass * per_pass + 1) // 2, 8400)[: n_pass * per_pass * CHUNK]
        b = quantise(iq)
        src = widen(b) if u8 else iq
        cuts = [k * per_pass * CHUNK for k in range(n_pass + 1)]
        if not u8:
            d = torch.from_numpy(iq).cuda()
            torch.cuda.synchronize()
            r = f2.Restated(FIX2)
            wants = [r.demod_iq(iq[a:z]) for a, z in zip(cuts[:-1], cuts[1:])]
            c.icao_flush()
            got = []
            for a, z in zip(cuts[:-1], cuts[1:]):
                if c.pending() == depth:
                    got.append(keys(c.collect()))
                c.submit_iq_device(d.data_ptr() + 4 * a, z - a)
                if c.pending() == 1:
                    assert c._L.adsb_set_error_correction(c._h, 0) == -7   # ADSB_ERR_BUSY while passes are pending
            while c.pending():
                got.append(keys(c.collect()))
            assert got == wants
            assert c.error_correction == FIX2
        # the ring
        c.icao_flush()
        (c.ring_create_u8 if u8 else c.ring_create)(per_pass * CHUNK)
        r = f2.Restated(FIX2)
        got, wants = [], []
        for a, z in zip(cuts[:-1], cuts[1:]):
            if c.pending() == depth:
                got.append(keys(c.collect()))
            buf = c.ring_acquire_u8() if u8 else c.ring_acquire()
            buf[: z - a] = b[a:z] if u8 else iq[a:z]
            c.ring_submit(z - a)
            wants.append(r.demod_iq(src[a:z]))
        while c.pending():
            got.append(keys(c.collect()))
        assert got == wants


def test_carry_over_and_caller_magnitudes(hip_lib):
    from dump1090_rs_amd import Context
    iq = mixed(2, 8500)
    good = synth.df17_frame(fs.KNOWN[1], 0x58C382D690C8AC + 0x1000)
    for k in (1, 2, 3):   # a two-bit copy across every buffer edge
        synth.add_bursts(iq, [synth.Burst(5 * (k * CHUNK - 60) + 2, 20000, 3, f2.flip2(good, 20 + k, 70 + k))])
    with Context(0, 16) as c:
        c.set_error_correction(FIX2)
        for step in (CHUNK, 2 * CHUNK):
            c.set_carry_over(True)
            r = f2.Restated(FIX2, carry=True)
            c.icao_flush()
            for a in range(0, len(iq), step):
                assert keys(c.demod_iq(iq[a:a + step], cap=1 << 20)) == r.demod_iq(iq[a:a + step])
            c.set_carry_over(False)
        r = f2.Restated(FIX2)
        c.icao_flush()
        n_fixed = 0
        for a in range(0, len(iq), CHUNK):
            mag = c.to_mag(iq[a:a + CHUNK])
            want = r.demodulate2400(mag.data, mag.length)
            assert keys(c.demodulate2400(mag, cap=1 << 16)) == want
            n_fixed += sum(k[1] == 1100 for k in want)
        assert n_fixed >= 100


def test_the_list_overflow_fallback(hip_lib):
    from dump1090_rs_amd import Context
    # a periodic stretch overflows a one-buffer context's lists: that buffer goes through k_scan_simple_fix2
    iq = mixed(1, 8600)
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 10000, CHUNK + 95000   # (the second buffer's two-bit copies start at 99300)
    iq[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    iq[a:z, 1] = 0
    with Context(0, 1) as c:
        c.set_error_correction(FIX2)
        c.icao_flush()
        got = keys(c.demod_iq(iq, cap=1 << 20))
        assert c.stats()["retries"] > 0
    want = f2.Restated(FIX2).demod_iq(iq)
    assert got == want
    assert sum(k[1] == 1100 and k[4] == 1 for k in want) >= 40


def test_shards_and_adsb_multi(hip_lib):
    import torch
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import replay_records
    from dump1090_rs_amd.multi import MultiContext
    iq = mixed(3, 8700)
    want = f2.Restated(FIX2).demod_iq(iq)
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, 8) as c:
        c.set_error_correction(FIX2)
        c.icao_flush()
        learned = c.shard_scan(d.data_ptr(), len(iq))
        rec = c.shard_finish(learned)
    assert keys(replay_records(rec, mode=FIX2)) == want
    for n_ctx, parallel_min in ((2, 0), (3, 1)):
        with MultiContext([0] * n_ctx, 4) as m:
            m.set_error_correction(FIX2)
            if parallel_min:
                m.selftest_tune(parallel_min=parallel_min)
            for _ in range(2):
                m.icao_flush()
                assert keys(m.demod_iq(iq, cap=1 << 20)) == want, n_ctx
            m.set_error_correction(0)
            m.icao_flush()
            assert keys(m.demod_iq(iq, cap=1 << 20)) == f2.Restated(0).demod_iq(iq)


def test_feed_tool_fix_2bit(hip_lib, tmp_path):
    from tests.conftest import ROOT
    iq = mixed(2, 8800)
    want = f2.Restated(FIX2).demod_iq(iq)
    path = tmp_path / "cap.iq"
    path.write_bytes(np.ascontiguousarray(iq[:, ::-1]).tobytes())     # the capture format: im first
    r = subprocess.run([str(ROOT / "dump1090_rs_amd" / "adsb_feed"), "--fix", "2bit", "--buffers", "2", str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [f"*{k[0].hex()};" for k in want]
    assert sum(k[1] == 1100 for k in want) >= 100

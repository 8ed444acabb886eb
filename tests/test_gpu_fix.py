"""Single-bit repair of DF17/18 (ADSB_FIX_1BIT) on the device: every path the mode reaches, each compared with the CPU
restatement (tests/fix_restatement.c); mode 0 with the reference's result."""
import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import fix_support as fs
from tests.test_gpu_parity import ADVERSARIAL_PERIODS
from tests.test_u8_cpu import t_soapy_numpy

pytestmark = pytest.mark.gpu
CHUNK = fs.CHUNK
FIX = 1


def quantise(iq):
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def widen(b):
    return np.ascontiguousarray(t_soapy_numpy()[b.reshape(-1, 2)])


def keys(msgs):
    return [fs.key(m) for m in msgs]


def damaged_stream(n_buffers, seed=7100):
    """n_buffers of damaged_capture, each with its own noise (the aircraft are the same ones throughout)."""
    return np.concatenate([fs.damaged_capture(seed + k)[0] for k in range(n_buffers)])


def test_every_single_bit_copy_of_a_known_aircraft_comes_back(hip_lib):
    from dump1090_rs_amd import Context
    iq, clean, repairable = fs.damaged_capture()
    want0, want1 = fs.Restated(0).demod_iq(iq), fs.Restated(FIX).demod_iq(iq)
    with Context(0, 1) as c:
        assert c.error_correction == 0
        c.icao_flush()
        got0 = keys(c.demod_iq(iq))
        c.set_error_correction(FIX)
        assert c.error_correction == FIX
        c.icao_flush()
        got1 = keys(c.demod_iq(iq))
    assert got0 == want0 and all(k[1] != 1200 for k in got0)
    assert got1 == want1
    assert fs.repaired_by_slot([k for k in got1 if k[1] == 1200], got0) == {4 + b: f for b, f in repairable.items()}


@pytest.mark.parametrize("max_chunks, n_buffers", [(1, 1), (16, 5), (16, 16), (64, 40)])
def test_blocking_host_and_device_cs16_and_cu8(hip_lib, max_chunks, n_buffers):
    import torch
    from dump1090_rs_amd import Context
    iq = damaged_stream(n_buffers)
    b = quantise(iq)
    wide = widen(b)
    d = torch.from_numpy(iq).cuda()
    d8 = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    want = fs.Restated(FIX).demod_iq(iq)
    want8 = fs.Restated(FIX).demod_iq(wide)
    assert sum(k[1] == 1200 for k in want) >= 100 * n_buffers
    with Context(0, max_chunks) as c:
        c.set_error_correction(FIX)
        for run in range(2):   # (the second time round a dense stream is ordered on the device)
            c.icao_flush()
            assert keys(c.demod_iq(iq, cap=1 << 20)) == want, run
            c.icao_flush()
            assert keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)) == want, run
            c.icao_flush()
            assert keys(c.demod_iq_u8(b, cap=1 << 20)) == want8, run
            c.icao_flush()
            assert keys(c.demod_iq_device_u8(d8.data_ptr(), len(b), cap=1 << 20)) == want8, run
        c.set_error_correction(0)
        c.icao_flush()
        assert keys(c.demod_iq(iq, cap=1 << 20)) == fs.Restated(0).demod_iq(iq)


@pytest.mark.parametrize("max_chunks, per_pass", [(1, 1), (16, 16), (64, 64)])
def test_submit_collect_and_ring(hip_lib, max_chunks, per_pass):
    import torch
    from dump1090_rs_amd import Context
    with Context(0, max_chunks) as c:
        c.set_error_correction(FIX)
        depth = c.max_in_flight()
        n_pass = depth + 2
        iq = damaged_stream(n_pass * per_pass, seed=7300)
        d = torch.from_numpy(iq).cuda()
        torch.cuda.synchronize()
        cuts = [k * per_pass * CHUNK for k in range(n_pass + 1)]
        r = fs.Restated(FIX)
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
        assert c.error_correction == FIX
        # the ring
        c.icao_flush()
        c.ring_create(per_pass * CHUNK)
        r = fs.Restated(FIX)
        got, wants = [], []
        for a, z in zip(cuts[:-1], cuts[1:]):
            if c.pending() == depth:
                got.append(keys(c.collect()))
            buf = c.ring_acquire()
            buf[: z - a] = iq[a:z]
            c.ring_submit(z - a)
            wants.append(r.demod_iq(iq[a:z]))
        while c.pending():
            got.append(keys(c.collect()))
        assert got == wants


@pytest.mark.parametrize("max_chunks", [1, 16])
def test_carry_over_and_caller_magnitudes(hip_lib, max_chunks):
    from dump1090_rs_amd import Context
    iq = damaged_stream(3, seed=7500)
    # a frame across every buffer edge
    for k in (1, 2):
        synth.add_bursts(iq, [synth.Burst(5 * (k * CHUNK - 60) + 2, 20000, 3, fs.flip(synth.df17_frame(fs.KNOWN[1], 0x58C382D690C8AC + 0x1000), 70))])
    with Context(0, max_chunks) as c:
        c.set_error_correction(FIX)
        c.set_carry_over(True)
        r = fs.Restated(FIX, carry=True)
        c.icao_flush()
        for a in range(0, len(iq), CHUNK if max_chunks == 1 else 2 * CHUNK):
            part = iq[a:a + (CHUNK if max_chunks == 1 else 2 * CHUNK)]
            assert keys(c.demod_iq(part, cap=1 << 20)) == r.demod_iq(part)
        c.set_carry_over(False)
        # adsb_demodulate2400 on the caller's magnitudes, the filter carried along
        r = fs.Restated(FIX)
        c.icao_flush()
        for a in range(0, len(iq), CHUNK):
            mag = c.to_mag(iq[a:a + CHUNK])
            assert keys(c.demodulate2400(mag, cap=1 << 16)) == r.demodulate2400(mag.data, mag.length)


def test_dense_stream_and_the_list_overflow_fallback(hip_lib):
    from dump1090_rs_amd import Context
    # busy sky: 40 buffers of ~130 frames each, scored on the host under the fix (mode 0: on the device)
    iq = damaged_stream(40, seed=7700)
    with Context(0, 64) as c:
        for mode in (0, FIX, 0):
            c.set_error_correction(mode)
            for _ in range(2):
                c.icao_flush()
                assert keys(c.demod_iq(iq, cap=1 << 20)) == fs.Restated(mode).demod_iq(iq), mode
    # a periodic stretch with 3.4 address/parity trials per position overflows a one-buffer context's lists: that
    # buffer (the clean frames and ~50 damaged copies in front of the stretch) goes through the fallback kernel
    iq = damaged_stream(2, seed=7800)
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 40000, CHUNK + 125000
    iq[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    iq[a:z, 1] = 0
    with Context(0, 1) as c:
        c.set_error_correction(FIX)
        c.icao_flush()
        got = keys(c.demod_iq(iq, cap=1 << 20))
        assert c.stats()["retries"] > 0
    want = fs.Restated(FIX).demod_iq(iq)
    assert got == want
    assert sum(k[1] == 1200 and k[4] == 1 for k in want) >= 40


def test_shards_and_adsb_multi(hip_lib):
    import torch
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import replay_records
    from dump1090_rs_amd.multi import MultiContext
    iq = damaged_stream(6, seed=7900)
    want = fs.Restated(FIX).demod_iq(iq)
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, 8) as c:
        c.set_error_correction(FIX)
        c.icao_flush()
        learned = c.shard_scan(d.data_ptr(), len(iq))
        rec = c.shard_finish(learned)
    assert keys(replay_records(rec, mode=FIX)) == want
    assert keys(replay_records(rec)) == fs.Restated(0).demod_iq(iq)
    for n_ctx, parallel_min in ((2, 0), (3, 1), (4, 0)):
        with MultiContext([0] * n_ctx, 4) as m:
            m.set_error_correction(FIX)
            if parallel_min:
                m.selftest_tune(parallel_min=parallel_min)
            for _ in range(2):
                m.icao_flush()
                assert keys(m.demod_iq(iq, cap=1 << 20)) == want, n_ctx
            m.set_error_correction(0)
            m.icao_flush()
            assert keys(m.demod_iq(iq, cap=1 << 20)) == fs.Restated(0).demod_iq(iq)


def test_reference_captures(hip_lib, fixture_iq):
    from dump1090_rs_amd import Context
    with Context(0, 1) as c:
        for name, iq in sorted(fixture_iq.items()):
            c.set_error_correction(0)
            c.icao_flush()
            got0 = keys(c.demod_iq(iq))
            c.set_error_correction(FIX)
            c.icao_flush()
            got1 = keys(c.demod_iq(iq))
            assert set(got0) <= set(got1)
            assert got0 == fs.Restated(0).demod_iq(iq) and got1 == fs.Restated(FIX).demod_iq(iq), name

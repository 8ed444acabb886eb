"""CU8 (8-bit RTL-SDR IQ, include/adsb_hip.h "8-bit IQ") on the device.  The contract: a CU8 call on bytes b returns
what its CS16 twin returns on widen(b) = T[b], bit for bit -- so every test widens in numpy and compares with the CPU
oracle (which takes CS16) on exactly those samples, or with the CS16 entry point itself."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from dump1090_rs_amd import synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
CHUNK = 131072


def t_soapy() -> np.ndarray:
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


T = t_soapy()


def widen(b: np.ndarray, table: np.ndarray = T) -> np.ndarray:
    """CU8 (N, 2) uint8 -> the CS16 (N, 2) int16 it means."""
    return np.ascontiguousarray(table[b.reshape(-1, 2)])


def narrow_exact(iq: np.ndarray) -> np.ndarray:
    """CS16 whose every value is an entry of T_soapy (the reference's captures) -> its bytes."""
    lut = np.full(65536, -1, dtype=np.int32)
    lut[T.astype(np.int64) + 32768] = np.arange(256)
    b = lut[iq.astype(np.int64) + 32768]
    assert (b >= 0).all()
    return np.ascontiguousarray(b.astype(np.uint8))


def quantise(iq: np.ndarray) -> np.ndarray:
    """Any CS16 stream -> CU8 bytes near it (the synthetic streams)."""
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msglen, m.msg.hex(), m.signal_level)


def assert_same(msgs, want):
    got = [key(m) for m in msgs]
    exp = [(w["chunk"], w["j"], w["try_phase"], w["score"], w["len"], w["msg"].hex(), w["signal_level"]) for w in want]
    assert got == exp


def golden_u8(fixture_iq, golden):
    return [(fx, narrow_exact(fixture_iq[fx["file"]])) for fx in golden["fixtures"]]


# ----------------------------------------------------------------------------------------------- golden
def test_golden_captures_as_cu8_give_the_reference_frames(hip_lib, golden, fixture_iq):
    from dump1090_rs_amd import Context
    with Context(0, 1) as c:
        for fx, b in golden_u8(fixture_iq, golden):
            assert np.array_equal(widen(b), fixture_iq[fx["file"]])
            c.icao_flush()
            got = c.demod_iq_u8(b)
            assert [m.buffer().hex() for m in got] == fx["frames"]
            assert [m.j for m in got] == fx["j"] and [m.try_phase for m in got] == fx["try_phase"]
            c.icao_flush()
            want = c.demod_iq(fixture_iq[fx["file"]])
            assert [key(m) for m in got] == [key(m) for m in want]
            # and the same from device memory, and as the reference's two calls
            import torch
            d = torch.from_numpy(b).cuda()
            torch.cuda.synchronize()
            c.icao_flush()
            assert [key(m) for m in c.demod_iq_device_u8(d.data_ptr(), len(b))] == [key(m) for m in want]
            mag = c.to_mag_u8(b)
            assert np.array_equal(mag.data, c.to_mag(fixture_iq[fx["file"]]).data) and mag.length == len(b)


# ----------------------------------------------------------------------------------------------- to_mag
def test_to_mag_u8_every_byte_pair_and_the_edges(hip_lib, oracle_mod):
    from dump1090_rs_amd import Context
    orc = oracle_mod.Oracle()
    pairs = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.uint8)
    rng = np.random.default_rng(11)
    cases = [pairs] + [rng.integers(0, 256, size=(n, 2), dtype=np.uint8) for n in (0, 1, 3, 131071, 131072)]
    with Context(0, 1) as c:
        for b in cases:
            got = c.to_mag_u8(b)
            data, n = orc.to_mag(widen(b))
            assert got.length == n == len(b)
            assert np.array_equal(got.data, data)
            assert not got.data[:326].any() and not got.data[326 + len(b):].any()   # T[0] != 0: zero by position
        # the lead-in of a buffer of bytes 0 is still zero, its samples are not
        zeros = np.zeros((1000, 2), np.uint8)
        m = c.to_mag_u8(zeros)
        assert not m.data[:326].any() and m.data[326:1326].all() and not m.data[1326:].any()


# ----------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("n_chunks, ragged, n_bursts", [(1, 0, 40), (2, 777, 80), (16, 5, 600), (64, 131071, 2000)])
def test_cu8_streams_host_and_device(hip_lib, oracle_mod, n_chunks, ragged, n_bursts):
    import torch
    from dump1090_rs_amd import Context
    n = n_chunks * CHUNK - ragged
    b = quantise(synth.make_iq(n, n_bursts=n_bursts, seed=300 + n_chunks, n_icao=20, df11_every=3))
    want, _ = oracle_mod.Oracle().demod_iq(widen(b), cap=1 << 20)
    assert len(want) > 0
    d = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    for max_chunks in sorted({min(n_chunks, 16), n_chunks}):
        with Context(0, max_chunks) as c:
            c.icao_flush()
            assert_same(c.demod_iq_u8(b, cap=1 << 20), want)
            c.icao_flush()
            assert_same(c.demod_iq_device_u8(d.data_ptr(), n, cap=1 << 20), want)


@pytest.mark.parametrize("n_bursts", [64, 5000])
def test_cu8_512_buffers_device_resident_and_device_scored(hip_lib, oracle_mod, n_bursts):
    import torch
    from dump1090_rs_amd import Context
    n = 512 * CHUNK
    b = quantise(synth.make_iq_torch(n, n_bursts=n_bursts, device="cuda").cpu().numpy())
    want, st = oracle_mod.Oracle().demod_iq(widen(b), cap=1 << 20)
    d = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    with Context(0, 512) as c:
        c.icao_flush()
        c.demod_iq_device_u8(d.data_ptr(), n, cap=1 << 20)   # (tells the context how dense this stream is)
        c.icao_flush()
        got = c.demod_iq_device_u8(d.data_ptr(), n, cap=1 << 20)
        s = c.stats()
        host_sorts, host_replays = c._L.adsb_host_sorts(c._h), c._L.adsb_host_replays(c._h)
    assert_same(got, want)
    assert s["n_candidates"] == st.quiet_pass and s["retries"] == 0
    if n_bursts >= 5000:
        assert (host_sorts, host_replays) == (1, 1)   # the second pass ordered and scored on the device
    else:
        assert (host_sorts, host_replays) == (2, 2)


@pytest.mark.parametrize("max_chunks, per_pass", [(1, 1), (16, 16), (64, 64)])
def test_cu8_pipelined_submit_collect_at_full_depth(hip_lib, oracle_mod, max_chunks, per_pass):
    import torch
    from dump1090_rs_amd import Context
    with Context(0, max_chunks) as c:
        depth = c.max_in_flight()
        n_pass = depth + 3
        n = n_pass * per_pass * CHUNK - 999
        b = quantise(synth.make_iq(n, n_bursts=30 * n_pass * per_pass, seed=77 + max_chunks, n_icao=15, df11_every=4))
        orc = oracle_mod.Oracle()
        d = torch.from_numpy(b).cuda()
        torch.cuda.synchronize()
        cuts = [min(k * per_pass * CHUNK, n) for k in range(n_pass + 1)]
        wants = [orc.demod_iq(widen(b[a:z]), cap=1 << 20)[0] for a, z in zip(cuts[:-1], cuts[1:])]
        c.icao_flush()
        got = []
        for a, z in zip(cuts[:-1], cuts[1:]):
            if c.pending() == depth:
                got.append(c.collect())
            c.submit_iq_device_u8(d.data_ptr() + 2 * a, z - a)
        while c.pending():
            got.append(c.collect())
        assert len(got) == n_pass
        for g, w in zip(got, wants):
            assert_same(g, w)


def test_list_overflow_fallback_widens_cu8(hip_lib, oracle_mod):
    """Input far denser than a one-buffer context's lists: the buffer-by-buffer fallback (the reference-shaped
    kernel, CS16 only) takes CU8 through a widened staging buffer -- in reference and carry-over semantics."""
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    n = 8 * CHUNK - 4321
    b = quantise(synth.make_iq(n, n_bursts=300, n_icao=3, seed=99))
    want, _ = oracle_mod.Oracle().demod_iq(widen(b), cap=1 << 20)
    carry = np.zeros((326, 2), np.int16)
    want_c, _ = demod_iq_carry(oracle_mod.Oracle(), widen(b), carry, cap=1 << 20)
    with Context(0, 1) as c:
        c.icao_flush()
        assert_same(c.demod_iq_u8(b, cap=1 << 20), want)
        c.set_carry_over(True)
        c.icao_flush()
        assert_same(c.demod_iq_u8(b, cap=1 << 20), want_c)


# ----------------------------------------------------------------------------------------------- tables
def test_custom_table_and_a_change_between_calls(hip_lib, oracle_mod):
    from dump1090_rs_amd import Context
    rng = np.random.default_rng(5)
    custom = rng.integers(-32768, 32768, size=256).astype(np.int16)
    custom[[0, 1, 255]] = [0, -32768, 32767]
    n = 3 * CHUNK + 1234
    iq = synth.make_iq(n, n_bursts=200, seed=21, n_icao=10)
    b = quantise(iq)
    # a table that makes a real signal of the same bytes: the identity ramp scaled, then T_soapy's mirror image
    ramp = ((np.arange(256) - 128) * 256).astype(np.int16)
    with Context(0, 4) as c:
        assert np.array_equal(c.u8_table(), T)
        orc = oracle_mod.Oracle()
        for table in (custom, ramp, None, -T):
            c.set_u8_table(table)
            tab = T if table is None else table
            assert np.array_equal(c.u8_table(), tab)
            want, _ = orc.demod_iq(widen(b, tab), cap=1 << 20)
            assert_same(c.demod_iq_u8(b, cap=1 << 20), want)      # the filter carries over from call to call
            data, _ = orc.to_mag(widen(b[:CHUNK], tab))
            assert np.array_equal(c.to_mag_u8(b[:CHUNK]).data, data)
        assert len(want) > 0
        with pytest.raises(ValueError):
            c.set_u8_table(np.zeros(255, np.int16))


# ----------------------------------------------------------------------------------------------- carry-over
def test_carry_over_alternating_cu8_and_cs16_is_one_stream(hip_lib, oracle_mod):
    import torch
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    n = 6 * CHUNK + 999
    b = quantise(synth.make_iq(n, n_bursts=120, seed=42, n_icao=8, df11_every=3))
    fr = synth.df17_frame(0xABCDEF, 4242)
    # calls cut at awkward places (16-byte aligned as CU8 device input), one of them shorter than the carry
    cuts = [0, CHUNK - 104, 2 * CHUNK + 304, 3 * CHUNK + 56, 3 * CHUNK + 256, 5 * CHUNK + 7000, n]
    # a frame straddling four of the cuts: only carry-over finds those, and only if the carry holds the widened samples
    burst = synth.make_iq(3000, n_bursts=0, seed=1)
    synth.add_bursts(burst, [synth.Burst(5 * 1000, 20000, 3, fr)])
    seg = quantise(burst[900:1400])                    # the frame starts 100 samples in
    for cut in (cuts[1], cuts[2], cuts[3], cuts[5]):
        b[cut - 250: cut + 250] = seg
    cs16 = widen(b)
    w = cs16
    orc, carry = oracle_mod.Oracle(), np.zeros((326, 2), np.int16)
    wants = [demod_iq_carry(orc, w[a:z], carry, cap=1 << 20)[0] for a, z in zip(cuts[:-1], cuts[1:])]
    assert sum(x["buffer"] == fr for ws in wants for x in ws) >= 3
    with Context(0, 8) as c:
        c.set_carry_over(True)
        c.icao_flush()
        for k, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
            got = c.demod_iq_u8(b[a:z], cap=1 << 20) if k % 2 == 0 else c.demod_iq(cs16[a:z], cap=1 << 20)
            assert_same(got, wants[k])
        # pipelined, device resident, the formats alternating
        db, dw = torch.from_numpy(b).cuda(), torch.from_numpy(cs16).cuda()
        torch.cuda.synchronize()
        c.set_carry_over(True)
        c.icao_flush()
        got = []
        for k, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
            if c.pending() == c.max_in_flight():
                got.append(c.collect(cap=1 << 20))
            if k % 2:
                c.submit_iq_device_u8(db.data_ptr() + 2 * a, z - a)
            else:
                c.submit_iq_device(dw.data_ptr() + 4 * a, z - a)
        while c.pending():
            got.append(c.collect(cap=1 << 20))
        for g, wnt in zip(got, wants):
            assert_same(g, wnt)


# ----------------------------------------------------------------------------------------------- ring
@pytest.mark.parametrize("per_slot_chunks, max_chunks", [(1, 16), (2, 16), (16, 16), (64, 64)])
def test_cu8_ring_is_one_stream(hip_lib, oracle_mod, per_slot_chunks, max_chunks):
    from dump1090_rs_amd import Context
    per_slot = per_slot_chunks * CHUNK
    n_slots = 3 if per_slot_chunks == 64 else 11
    n = n_slots * per_slot - 1111
    b = quantise(synth.make_iq(n, n_bursts=20 * n_slots * per_slot_chunks, seed=9 + per_slot_chunks, n_icao=12, df11_every=3))
    orc = oracle_mod.Oracle()
    wants = [orc.demod_iq(widen(b[k * per_slot:(k + 1) * per_slot]), cap=1 << 20)[0] for k in range(n_slots)]
    with Context(0, max_chunks) as c:
        c.ring_create_u8(per_slot)
        with pytest.raises(Exception):
            c.ring_acquire()                                    # a CU8 ring hands out no CS16 slot
        for depth in sorted({4, c.max_in_flight()}):
            c.icao_flush()
            got = []
            for k in range(n_slots):
                if c.pending() == depth:
                    got.append(c.collect(cap=1 << 20))
                part = b[k * per_slot:(k + 1) * per_slot]
                buf = c.ring_acquire_u8()
                assert buf.shape == (per_slot, 2) and buf.dtype == np.uint8
                buf[: len(part)] = part
                c.ring_submit(len(part))
            while c.pending():
                got.append(c.collect(cap=1 << 20))
            assert len(got) == n_slots
            for g, w in zip(got, wants):
                assert_same(g, w)


# ----------------------------------------------------------------------------------------------- tool
def test_adsb_feed_format_cu8_prints_the_cs16_lines(hip_lib, golden, fixture_iq, tmp_path):
    feed = ROOT / "dump1090_rs_amd" / "adsb_feed"
    fx = golden["fixtures"][1]
    raw = tmp_path / "capture.cu8"
    narrow_exact(fixture_iq[fx["file"]]).tofile(raw)     # rtl_sdr's order: I, Q
    cs16 = subprocess.run([str(feed), "--buffers", "2", str(GOLDEN / fx["file"])], capture_output=True, text=True, timeout=120)
    cu8 = subprocess.run([str(feed), "--buffers", "2", "--format", "cu8", str(raw)], capture_output=True, text=True, timeout=120)
    assert cs16.returncode == 0 and cu8.returncode == 0, cs16.stderr + cu8.stderr
    assert cs16.stdout == cu8.stdout
    assert cs16.stdout.splitlines() == ["*" + f + ";" for f in fx["frames"]]
    # ... and from a pipe
    with open(raw, "rb") as f:
        piped = subprocess.run([str(feed), "--buffers", "2", "--format", "cu8", "-"], stdin=f, capture_output=True,
                               text=True, timeout=120)
    assert piped.returncode == 0 and piped.stdout == cs16.stdout


# ----------------------------------------------------------------------------------------------- errors
def test_cu8_argument_errors(hip_lib):
    import torch
    from dump1090_rs_amd import Context, _lib
    from dump1090_rs_amd._lib import AdsbError
    d = torch.zeros(4 * CHUNK, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with Context(0, 1) as c:
        with pytest.raises(AdsbError) as e:
            c.demod_iq_device_u8(d.data_ptr() + 2, 1000)
        assert e.value.status == _lib.ADSB_ERR_INVALID
        with pytest.raises(AdsbError) as e:
            c.submit_iq_device_u8(d.data_ptr() + 8, 1000)
        assert e.value.status == _lib.ADSB_ERR_INVALID
        with pytest.raises(IndexError):
            c.to_mag_u8(np.zeros((CHUNK + 1, 2), np.uint8))
        c.submit_iq_device_u8(d.data_ptr(), 1000)
        with pytest.raises(AdsbError) as e:
            c.set_u8_table(None)
        assert e.value.status == _lib.ADSB_ERR_BUSY
        c.collect()
        c.set_u8_table(None)
    with Context(0, 1) as c:
        c.ring_create(CHUNK)
        with pytest.raises(AdsbError) as e:
            c.ring_acquire_u8()
        assert e.value.status == _lib.ADSB_ERR_INVALID
        assert c.ring_acquire().shape == (CHUNK, 2)

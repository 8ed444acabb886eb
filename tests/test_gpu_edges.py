"""The preamble gates and the bit slicer at exact ties and thresholds on the device (tests/edges_support.py), with
tolerance 0 against the oracle: stage lists of the comparison-pattern and small-alphabet streams, and the edge-frame
catalogue through every path that evaluates the gates -- one- and three-launch passes, caller magnitudes, CU8,
carry-over, the list-overflow fallback (k_scan_simple) and the repair modes (k_scan_fix / k_scan_fix2)."""
import numpy as np
import pytest

from tests import edges_support as E
from tests import fix2_support as f2s
from tests import fix_support as fs
from tests.test_edges_cpu import cu8_stream, cu8_table
from tests.test_gpu_parity import ADVERSARIAL_PERIODS

pytestmark = pytest.mark.gpu
CHUNK = E.CHUNK
STAGE_STREAMS = ["debruijn", "low", "wide", "odd", "full", "planted"]


def keys(msgs):
    return [fs.key(m) for m in msgs]


def okeys(ws):
    return [(w["buffer"], w["score"], w["j"], w["try_phase"], w["chunk"], w["signal_level"]) for w in ws]


def frame_stream(n_buffers: int) -> np.ndarray:
    """The planted catalogue, then the small-alphabet streams, repeated to n_buffers."""
    one = np.concatenate([E.iq_stream(n) for n in ("planted", "low", "wide", "odd", "full")])
    reps = n_buffers // (len(one) // CHUNK) + 1
    return np.ascontiguousarray(np.concatenate([one] * reps)[: n_buffers * CHUNK])


@pytest.mark.parametrize("name", STAGE_STREAMS)
def test_stage_lists_equal_the_oracle(hip_lib, oracle_mod, name):
    """Preamble, 3.5 dB, candidate and address/parity lists of every IQ-domain stream: the fast scan's "<=" pattern
    stage, gate_eval's rebuilt sums and its tie fallback, position for position."""
    import torch
    from dump1090_rs_amd import Context
    iq = E.iq_stream(name)
    sl = oracle_mod.stage_lists(iq)
    d = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
    torch.cuda.synchronize()
    with Context(0, 16) as c:
        pre, snr = c.selftest_gate_stages(d.data_ptr(), len(iq))
        cand, ap = c.selftest_stage_lists(d.data_ptr(), len(iq))
    assert pre.tolist() == sl["preamble"]
    assert snr.tolist() == sl["snr"]
    assert cand.tolist() == sl["cand"]
    assert ap.tolist() == sl["ap"]
    assert len(sl["preamble"]) > 500


@pytest.mark.parametrize("max_chunks, n_buffers", [(16, 9), (64, 20)])
def test_frames_one_and_three_launch_passes(hip_lib, oracle_mod, max_chunks, n_buffers):
    import torch
    from dump1090_rs_amd import Context
    iq = frame_stream(n_buffers)
    want, st = oracle_mod.Oracle().demod_iq(iq, cap=1 << 20)
    want = okeys(want)
    assert st.quiet_pass > 3000 and len(want) >= 80
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    with Context(0, max_chunks) as c:
        for run in range(2):   # (the second time round a dense stream is ordered on the device)
            c.icao_flush()
            got = keys(c.demod_iq(iq, cap=1 << 20))
            s = c.stats()
            assert s["retries"] == 0 and got == want, ("host", run)   # the fast scan decided, not the fallback
            assert s["n_candidates"] == st.quiet_pass, (run, s["n_candidates"], st.quiet_pass)
            c.icao_flush()
            got = keys(c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20))
            assert c.stats()["retries"] == 0 and got == want, ("device", run)


def test_caller_magnitudes_with_a_lead_in(hip_lib, oracle_mod):
    """demodulate2400 on magnitudes no IQ pair reaches (1, 5, 65534 on the axis, 65535), a non-zero lead-in, and the
    catalogue handed over as magnitudes."""
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import MagnitudeBuffer
    cases = [(E.alphabet_stream("caller", 1, 5), E.alphabet_stream("caller", 1, 15)[:E.LEAD]),
             (E.alphabet_stream("caller_full", 1, 6), E.alphabet_stream("caller_full", 1, 16)[:E.LEAD]),
             (E.catalogue_mags(E.catalogue(), CHUNK)[0], None)]
    with Context(0, 1) as c:
        for k, (mags, lead) in enumerate(cases):
            data = E.data_of(mags, lead)
            want, st = oracle_mod.Oracle().demodulate2400(data, CHUNK)
            assert st.quiet_pass > 100, k
            c.icao_flush()
            got = keys(c.demodulate2400(MagnitudeBuffer(data=data, length=CHUNK), cap=1 << 16))
            s = c.stats()
            assert s["retries"] == 0 and got == okeys(want), k
            assert s["n_candidates"] == st.quiet_pass, k


def test_cu8_with_a_custom_table(hip_lib, oracle_mod):
    import torch
    from dump1090_rs_amd import Context
    t = cu8_table()
    b = cu8_stream(3, seed=11)
    want, st = oracle_mod.Oracle().demod_iq(np.ascontiguousarray(t[b]), cap=1 << 20)
    assert st.quiet_pass > 1000
    d8 = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    with Context(0, 16) as c:
        c.set_u8_table(t)
        assert np.array_equal(c.u8_table(), t)
        c.icao_flush()
        got = keys(c.demod_iq_u8(b, cap=1 << 20))
        assert c.stats()["retries"] == 0 and got == okeys(want)
        assert c.stats()["n_candidates"] == st.quiet_pass
        c.icao_flush()
        assert keys(c.demod_iq_device_u8(d8.data_ptr(), len(b), cap=1 << 20)) == okeys(want)


def test_carry_over_with_edges_across_buffer_ends(hip_lib, oracle_mod):
    """At every buffer end a catalogue slot whose p0..p18 straddle it (p0 1..18 samples before the end), and half the
    catalogue inside every buffer, buffer by buffer with carry-over."""
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    cases = E.catalogue()
    offsets = (1, 4, 7, 10, 13, 16, 18)
    n_buf = len(offsets) + 1
    inner, _ = E.catalogue_mags(cases, CHUNK)
    mags = np.zeros(n_buf * CHUNK, dtype=np.int64)
    for k in range(n_buf):
        mags[k * CHUNK:k * CHUNK + CHUNK // 2] = inner[:CHUNK // 2]
    straddle = [c for c in cases if c.passes][:: 11][:len(offsets)]
    for k, (c, off) in enumerate(zip(straddle, offsets)):
        s = (k + 1) * CHUNK - off - c.j0
        mags[s:s + E.SPACING] = c.mags
    iq = E.to_iq(mags)
    orc = oracle_mod.Oracle()
    carry = np.zeros((326, 2), np.int16)
    edge = 0
    with Context(0, 1) as c:
        c.set_carry_over(True)
        c.icao_flush()
        for a in range(0, len(iq), CHUNK):
            want, st = demod_iq_carry(orc, iq[a:a + CHUNK], carry, cap=1 << 20)
            got = keys(c.demod_iq(iq[a:a + CHUNK], cap=1 << 20))
            assert c.stats()["retries"] == 0 and got == okeys(want), a // CHUNK
            assert c.stats()["n_candidates"] == st.quiet_pass, a // CHUNK
            edge += sum(E.LEAD - 18 <= w["j"] < E.LEAD for w in want)
    assert edge >= len(offsets) - 1


def test_the_overflow_fallback_decides_the_edges_alike(hip_lib, oracle_mod):
    """The planted catalogue in a buffer that also carries a periodic stretch dense enough to overflow a one-buffer
    context's lists: that buffer goes through k_scan_simple (preamble_gates, slice_message)."""
    from dump1090_rs_amd import Context
    cat = E.iq_stream("planted")
    iq = np.concatenate([cat, cat])
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 66000, CHUNK + 131000
    iq[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    iq[a:z, 1] = 0
    want, _ = oracle_mod.Oracle().demod_iq(iq, cap=1 << 20)
    with Context(0, 1) as c:
        c.icao_flush()
        got = keys(c.demod_iq(iq, cap=1 << 20))
        assert c.stats()["retries"] > 0
    assert got == okeys(want)
    assert sum(w["chunk"] == 1 and w["j"] < 66000 for w in want) >= 40     # the catalogue's frames in that buffer


@pytest.mark.parametrize("mode", [1, 3])
def test_repair_modes_at_the_edges(hip_lib, mode):
    """ADSB_FIX_1BIT / ADSB_FIX_2BIT against the restatements: clean copies come first, so the aircraft is known and
    the slicer cases whose D == 0 bit broke the frame come back repaired."""
    from dump1090_rs_amd import Context
    R = fs.Restated if mode == 1 else f2s.Restated
    iq = np.concatenate([E.iq_stream("planted"), E.iq_stream("low")])
    want = R(mode).demod_iq(iq)
    assert sum(k[1] in (1200, 1100) for k in want) >= 5
    with Context(0, 16) as c:
        c.set_error_correction(mode)
        c.icao_flush()
        got = keys(c.demod_iq(iq, cap=1 << 20))
        assert c.stats()["retries"] == 0
    assert got == want

"""Signal statistics on the device (include/adsb_hip.h, "Signal statistics"): with the mode on every pass delivers one
integer record per 131072-sample buffer, and every field equals the plain restatement -- numpy over the ORACLE's
to_mag magnitudes, and over the raw input for the rails (tests/signal_support.py).  Tolerance 0.  With the mode off
nothing changes: the same adsb_msg fields, no record, no k_signal_stats launch."""
import subprocess

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import signal_support as ss
from tests.conftest import ROOT
from tests.test_gpu_parity import ADVERSARIAL_PERIODS
from tests.test_gpu_u8 import narrow_exact, quantise, widen

pytestmark = pytest.mark.gpu

CHUNK = ss.CHUNK
GOLDEN = ROOT / "tests" / "golden"


def dtype():
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
    return SIGNAL_STATS_DTYPE


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msglen, m.msg, m.signal_level)


def launches(c) -> int:
    return int(c._L.adsb_selftest_signal_launches(c._h))


def assert_records(got, want, what=""):
    assert got.dtype == dtype() and got.dtype.itemsize == 272
    assert len(got) == len(want), what
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), (what, name, got[name], want[name])


def cs16_of(raw):
    return widen(raw) if raw.dtype == np.uint8 else raw


def boundary_buffer(orc) -> np.ndarray:
    """One sample of every bin boundary: for every bin's smallest magnitude e, a sample of magnitude e and one of e - 1,
    plus the two sides of the -3 dBFS line and full scale; found by asking the oracle what candidates near
    |iq| = m / 2 give."""
    targets = sorted({ss.bin_edge(b) for b in range(60)} | {ss.bin_edge(b) - 1 for b in range(1, 60)} | {46340, 46341, 65535})
    cand = []
    for t in targets:
        r = t * 32768.0 / 65535.0
        for re in range(max(int(r) - 6, 0), min(int(r) + 2, 32768)):
            im0 = int(round(max(r * r - re * re, 0.0) ** 0.5))
            cand += [(re, im) for im in range(max(im0 - 3, 0), min(im0 + 4, 32768))]
    cand = np.array(sorted(set(cand)), dtype=np.int16)
    assert len(cand) <= CHUNK
    data, n = orc.to_mag(cand)
    mags = data[326:326 + n]
    picked, missing = [], []
    for t in targets:
        at = np.flatnonzero(mags == t)
        if len(at):
            picked.append(cand[at[0]])
        else:
            missing.append(t)
    assert missing == [1, 5]  # (no integer sample has these magnitudes: 1 + 0j already has 2, and 2 + 1j has 4, 2 + 2j has 6)
    iq = np.array(picked, dtype=np.int16)
    got, _ = orc.to_mag(iq)
    assert sorted(got[326:326 + len(iq)].tolist()) == [t for t in targets if t not in (1, 5)]
    return iq


@pytest.fixture(scope="module")
def inputs(fixture_iq, golden, oracle_mod):
    """{name: the raw samples of one call, (N, 2) int16 or uint8}."""
    orc = oracle_mod.Oracle()
    out = {}
    for fx in golden["fixtures"]:
        out["golden " + fx["file"]] = fixture_iq[fx["file"]]
        out["golden cu8 " + fx["file"]] = narrow_exact(fixture_iq[fx["file"]])
    out["sparse 64"] = synth.make_iq(64 * CHUNK, n_bursts=64, seed=801, n_icao=30, df11_every=4)
    out["busy 64"] = synth.make_iq(64 * CHUNK, n_bursts=64 * 60, seed=802, n_icao=200, df11_every=3)
    out["ragged"] = synth.make_iq(2 * CHUNK + 70001, n_bursts=90, seed=803, n_icao=10)          # 70001 = 4 * 17500 + 1
    out["ragged cu8"] = quantise(synth.make_iq(3 * CHUNK + 4099, n_bursts=120, seed=804, n_icao=10))   # ... + 3
    rails = np.empty((CHUNK, 2), np.int16)
    rails[:, 0] = np.where(np.arange(CHUNK) % 3 == 0, -32768, 32767)
    rails[:, 1] = np.where(np.arange(CHUNK) % 5 == 0, 32767, -32768)
    out["all rails"] = rails
    out["all rails cu8"] = np.where(np.arange(2 * CHUNK).reshape(-1, 2) % 7 < 3, 0, 255).astype(np.uint8)
    out["all zero"] = np.zeros((CHUNK + 5, 2), np.int16)
    out["boundaries"] = boundary_buffer(orc)
    return out


@pytest.fixture(scope="module")
def wants(inputs, oracle_mod):
    orc = oracle_mod.Oracle()
    return {name: ss.restated(orc, cs16_of(raw), raw, dtype()) for name, raw in inputs.items()}


def test_restatement_of_the_special_inputs(inputs, wants):
    """What the issue states about them, on the yardstick itself."""
    w = wants["all rails"]
    assert w["n_clipped"][0] == w["n_samples"][0] == CHUNK and w["peak"][0] == 65535 and w["n_strong"][0] == CHUNK
    w = wants["all rails cu8"]
    assert w["n_clipped"][0] == CHUNK
    w = wants["all zero"]
    assert list(w["n_samples"]) == [CHUNK, 5] and not w["sum_power"].any() and not w["peak"].any()
    assert list(w["hist"][:, 0]) == [CHUNK, 5]
    w = wants["boundaries"]
    assert (w["hist"][0][[b for b in range(60) if b not in (1, 5)]] >= 1).all() and w["n_strong"][0] >= 2 and w["peak"][0] == 65535
    assert wants["ragged"]["n_samples"][-1] % 4 == 1 and wants["ragged cu8"]["n_samples"][-1] % 4 == 3


def run_blocking(c, raw, how, dev=None):
    u8 = raw.dtype == np.uint8
    if how == "host":
        return (c.demod_iq_u8 if u8 else c.demod_iq)(raw, cap=1 << 20)
    if how == "device":
        return (c.demod_iq_device_u8 if u8 else c.demod_iq_device)(dev.data_ptr(), len(raw), cap=1 << 20)
    (c.submit_iq_device_u8 if u8 else c.submit_iq_device)(dev.data_ptr(), len(raw))
    return c.collect(cap=1 << 20)


@pytest.mark.parametrize("max_chunks", [16, 64])
def test_every_input_through_the_blocking_and_the_submitted_calls(hip_lib, inputs, wants, max_chunks):
    """adsb_demod_iq, adsb_demod_iq_device and submit / collect, CS16 and CU8: the records are the restatement's, the
    messages are those of the same call with the mode off, and only passes with the mode on launch the kernel.  (A
    context of 16 buffers takes the 64-buffer calls in four passes: the records of a call are those of all of them.)"""
    import torch
    from dump1090_rs_amd import Context
    with Context(0, max_chunks) as c:
        assert c._L.adsb_get_signal_stats(c._h) == 0 and launches(c) == 0
        for name, raw in inputs.items():
            want = wants[name]
            dev = torch.from_numpy(raw).cuda()
            torch.cuda.synchronize()
            hows = ["host", "device"] + (["submit"] if len(want) <= max_chunks else [])
            for how in hows:
                c.set_signal_stats(False)
                c.icao_flush()
                before = launches(c)
                off = [key(m) for m in run_blocking(c, raw, how, dev)]
                assert len(c.signal_stats()) == 0 and launches(c) == before, (name, how)
                c.set_signal_stats(True)
                assert c._L.adsb_get_signal_stats(c._h) == 1
                c.icao_flush()
                on = [key(m) for m in run_blocking(c, raw, how, dev)]
                assert on == off, (name, how)
                assert_records(c.signal_stats(), want, (name, how))
                assert launches(c) == before + (len(want) + max_chunks - 1) // max_chunks, (name, how)
        # a call of no samples: status OK, no records
        for raw in (np.zeros((0, 2), np.int16), np.zeros((0, 2), np.uint8)):
            assert run_blocking(c, raw, "host") == [] and len(c.signal_stats()) == 0
            d = torch.zeros(16, dtype=torch.uint8, device="cuda")
            assert run_blocking(c, raw, "device", d) == [] and len(c.signal_stats()) == 0
        # the caller's magnitudes are left alone
        c.demod_iq(inputs["all rails"])
        assert len(c.signal_stats()) == 1
        before = launches(c)
        c.demodulate2400(c.to_mag(inputs["all rails"]))
        assert len(c.signal_stats()) == 0 and launches(c) == before


def test_fetch_reports_the_full_count_when_the_array_is_smaller(hip_lib, inputs, wants):
    import ctypes as C
    from dump1090_rs_amd import Context, _lib
    with Context(0, 4) as c:
        c.set_signal_stats(True)
        c.demod_iq(inputs["ragged"])
        buf = np.zeros(2, dtype=dtype())
        n = C.c_size_t()
        assert c._L.adsb_fetch_signal_stats(c._h, buf.ctypes.data, 2, C.byref(n)) == _lib.ADSB_ERR_CAPACITY and n.value == 3
        assert_records(buf, wants["ragged"][:2])
        assert c._L.adsb_fetch_signal_stats(c._h, None, 0, C.byref(n)) == _lib.ADSB_ERR_CAPACITY and n.value == 3
        assert_records(c.signal_stats(), wants["ragged"])


@pytest.mark.parametrize("max_chunks", [16, 64])
def test_passes_in_flight_each_get_their_own_records(hip_lib, oracle_mod, inputs, max_chunks):
    """Eight (a context of 16 buffers) or four passes in flight, every one over a different input of a different
    length, the formats alternating: a record attributed to the wrong pass fails.  Setting the mode is refused while
    passes are pending."""
    import torch
    from dump1090_rs_amd import Context, _lib
    from dump1090_rs_amd._lib import AdsbError
    orc = oracle_mod.Oracle()
    stream = inputs["busy 64"]
    with Context(0, max_chunks) as c:
        depth = c.max_in_flight()
        assert depth == (8 if max_chunks == 16 else 4)
        cuts = [(k * 3 * CHUNK, k * 3 * CHUNK + (k % max_chunks % 5 + 1) * CHUNK - 1001 * k) for k in range(depth + 3)]
        raws = [quantise(stream[a:z]) if k % 2 else np.ascontiguousarray(stream[a:z]) for k, (a, z) in enumerate(cuts)]
        want = [ss.restated(orc, cs16_of(r), r, dtype()) for r in raws]
        assert len({len(r) for r in raws}) == len(raws)
        devs = [torch.from_numpy(r).cuda() for r in raws]
        torch.cuda.synchronize()
        c.set_signal_stats(True)
        c.icao_flush()
        got = []
        for k, r in enumerate(raws):
            if c.pending() == depth:
                c.collect(cap=1 << 20)
                got.append(c.signal_stats())
            (c.submit_iq_device_u8 if r.dtype == np.uint8 else c.submit_iq_device)(devs[k].data_ptr(), len(r))
        with pytest.raises(AdsbError) as e:
            c.set_signal_stats(False)
        assert e.value.status == _lib.ADSB_ERR_BUSY
        while c.pending():
            c.collect(cap=1 << 20)
            got.append(c.signal_stats())
        assert len(got) == len(raws) and launches(c) == len(raws)
        for k in range(len(raws)):
            assert_records(got[k], want[k], k)


@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
@pytest.mark.parametrize("per_slot_chunks", [1, 16])
def test_ring_slots_deliver_their_records(hip_lib, oracle_mod, inputs, fmt, per_slot_chunks):
    """The ring at one buffer per slot (read in place by its pass, and now a second time by the statistics) and at 16
    (copied first), both formats, every slot in flight.  The one-buffer stream keeps teaching the filter addresses, so
    some of its one-launch passes are redone through the three launches: their records are still there, computed once."""
    from dump1090_rs_amd import Context
    orc = oracle_mod.Oracle()
    per_slot = per_slot_chunks * CHUNK
    n_slots = 20 if per_slot_chunks == 1 else 4
    stream = inputs["busy 64"][: n_slots * per_slot - 1111]
    raw = quantise(stream) if fmt == "cu8" else stream
    parts = [raw[k * per_slot:(k + 1) * per_slot] for k in range(n_slots)]
    want = [ss.restated(orc, cs16_of(p), p, dtype()) for p in parts]
    with Context(0, 16) as c:
        (c.ring_create_u8 if fmt == "cu8" else c.ring_create)(per_slot)
        runs = {}
        for on in (False, True):
            c.set_signal_stats(on)
            c.icao_flush()
            before, before_rematches = launches(c), int(c._L.adsb_host_rematches(c._h))
            msgs, recs = [], []
            for part in parts:
                if c.pending() == c.max_in_flight():
                    msgs.append([key(m) for m in c.collect(cap=1 << 20)])
                    recs.append(c.signal_stats())
                buf = c.ring_acquire_u8() if fmt == "cu8" else c.ring_acquire()
                buf[: len(part)] = part
                c.ring_submit(len(part))
            while c.pending():
                msgs.append([key(m) for m in c.collect(cap=1 << 20)])
                recs.append(c.signal_stats())
            runs[on] = msgs
            assert launches(c) == before + (n_slots if on else 0)
            if per_slot_chunks == 1:
                assert int(c._L.adsb_host_rematches(c._h)) > before_rematches     # some passes did go twice
            for k in range(n_slots):
                assert_records(recs[k], want[k] if on else want[k][:0], (on, k))
        assert runs[True] == runs[False] and sum(len(m) for m in runs[True]) > 0


@pytest.mark.parametrize("max_chunks", [1, 4])
def test_overflow_fallback_still_delivers_the_records(hip_lib, oracle_mod, inputs, max_chunks):
    """A periodic stretch dense enough to overflow the lists of a context of one buffer and of four: the pass (of one
    buffer; of all three at once) is redone buffer by buffer through the reference-shaped kernel, and its records are
    those of its first enqueue."""
    from dump1090_rs_amd import Context
    iq = inputs["ragged"].copy()
    per = np.array(ADVERSARIAL_PERIODS[1], dtype=np.int16)
    a, z = CHUNK + 20000, CHUNK + 95000
    iq[a:z, 0] = np.tile(per, (z - a) // len(per) + 1)[: z - a]
    iq[a:z, 1] = 0
    orc = oracle_mod.Oracle()
    for raw in (iq, quantise(iq)):
        want = ss.restated(orc, cs16_of(raw), raw, dtype())
        ref, _ = oracle_mod.Oracle().demod_iq(cs16_of(raw), cap=1 << 20)
        with Context(0, max_chunks) as c:
            run = c.demod_iq_u8 if raw.dtype == np.uint8 else c.demod_iq
            c.icao_flush()
            off = [key(m) for m in run(raw, cap=1 << 20)]
            assert c.stats()["retries"] > 0
            c.set_signal_stats(True)
            c.icao_flush()
            on = [key(m) for m in run(raw, cap=1 << 20)]
            assert c.stats()["retries"] > 0            # the case really takes that path
            assert on == off and len(on) == len(ref)
            assert_records(c.signal_stats(), want)
            assert launches(c) == (len(want) + max_chunks - 1) // max_chunks     # one per pass, none for the redone ones


def test_carry_over_lead_in_is_not_counted(hip_lib, oracle_mod, inputs):
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    raw = inputs["ragged"]
    cuts = [0, CHUNK - 104, 2 * CHUNK + 304, len(raw)]
    orc, carry = oracle_mod.Oracle(), np.zeros((326, 2), np.int16)
    with Context(0, 4) as c:
        c.set_carry_over(True)
        c.set_signal_stats(True)
        c.icao_flush()
        for a, z in zip(cuts[:-1], cuts[1:]):
            part = np.ascontiguousarray(raw[a:z])
            want_msgs, _ = demod_iq_carry(orc, part, carry, cap=1 << 20)
            got = c.demod_iq(part, cap=1 << 20)
            assert [(m.chunk, m.j, m.try_phase, m.score, m.msg) for m in got] == \
                [(w["chunk"], w["j"], w["try_phase"], w["score"], w["msg"]) for w in want_msgs]
            assert_records(c.signal_stats(), ss.restated(orc, part, part, dtype()), (a, z))


def test_two_bit_repair_with_statistics_gives_the_frames_of_the_run_without(hip_lib, oracle_mod, inputs):
    from dump1090_rs_amd import Context, _lib
    raw = inputs["busy 64"][: 20 * CHUNK]
    want = ss.restated(oracle_mod.Oracle(), raw, raw, dtype())
    with Context(0, 64) as c:
        c.set_error_correction(_lib.ADSB_FIX_2BIT)
        c.icao_flush()
        off = [key(m) for m in c.demod_iq(raw, cap=1 << 20)]
        c.set_signal_stats(True)
        c.icao_flush()
        on = [key(m) for m in c.demod_iq(raw, cap=1 << 20)]
        assert on == off and len(on) > 0
        assert_records(c.signal_stats(), want)


def test_adsb_feed_stats_changes_stderr_only(hip_lib, golden, oracle_mod, fixture_iq):
    feed = ROOT / "dump1090_rs_amd" / "adsb_feed"
    fx = golden["fixtures"][1]
    raw = fixture_iq[fx["file"]]
    plain = subprocess.run([str(feed), "--buffers", "2", str(GOLDEN / fx["file"])], capture_output=True, timeout=120)
    assert plain.returncode == 0 and b"stats" not in plain.stderr
    want = ss.restated(oracle_mod.Oracle(), raw, raw, dtype())
    line = "adsb_feed: stats (whole input): " + ss.feed_line(ss.summary_of(want), len(want))
    for extra in (["--stats"], ["--stats", "0.5"]):
        r = subprocess.run([str(feed), "--buffers", "2", *extra, str(GOLDEN / fx["file"])], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == plain.stdout and r.stdout.decode().splitlines() == ["*" + f + ";" for f in fx["frames"]]
        assert r.stderr.decode().splitlines()[-1] == line

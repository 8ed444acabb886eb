"""k_scan_sparse on the device: the sparse stream's scan of a large context (more than 16 buffers) with the features such a
pass never uses folded out (adsb_scan_fast.hip: k_scan_sparse, sparse_scan_eligible).  Every list is compared with the
CPU oracle (oracle.binding; for the opt-in error correction, which the reference does not have, the oracle's restatement
with that mode, tests/fix2_support.py) -- never with what k_scan_fast returns.  The counter of the passes that ran the
new kernel (adsb_selftest_sparse_scans) says which kernel a pass took; adsb_selftest_set_sparse_scan switches it off.

Shapes: contexts of 17 to 34 buffers, just above the one-launch limit: a launch covers 289 to 578 tiles of 7712 positions
-- what can go wrong in the scan is at tile edges, buffer edges and the ragged end, not in how many rounds the persistent
grid takes."""
import numpy as np
import pytest

from dump1090_rs_amd import synth

pytestmark = pytest.mark.gpu

CHUNK = 131072
TILE = 7712           # adsb_scan_geometry.h: preamble positions of one workgroup's tile
REACH = 290           # the furthest sample a preamble at j touches

DF4 = bytes([0x20, 0x00, 0x05, 0x30])
DF5 = bytes([0x28, 0x00, 0x1A, 0x2B])
DF20 = bytes([0xA0, 0x00, 0x05, 0x30, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77])
DF21 = bytes([0xA8, 0x00, 0x1A, 0x2B, 0x70, 0x61, 0x52, 0x43, 0x34, 0x25, 0x16])


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msglen, m.msg, m.signal_level)


def want_key(w):
    return (w["chunk"], w["j"], w["try_phase"], w["score"], w["len"], w["msg"], w["signal_level"])


def ap_frame(first_bytes: bytes, icao: int) -> bytes:
    return first_bytes + (synth.crc24(first_bytes) ^ icao).to_bytes(3, "big")


def at(sample, k, frame, amp=20000):
    """`frame` starting at `sample` (sub-sample phase and carrier angle from k)"""
    return synth.Burst(5 * sample + k % 5, amp, k % 16, frame)


def sparse_scans(c) -> int:
    return int(c._L.adsb_selftest_sparse_scans(c._h))


def set_sparse_scan(c, on: bool) -> None:
    assert c._L.adsb_selftest_set_sparse_scan(c._h, 1 if on else 0) == 0


def oracle_passes(oracle_mod, caps, flush_before):
    """One oracle stream over the captures in order: its filter persists, flushed before the passes named."""
    orc = oracle_mod.Oracle()
    orc.icao_flush()
    want = []
    for k, iq in enumerate(caps):
        if k in flush_before:
            orc.icao_flush()
        want.append([want_key(w) for w in orc.demod_iq(iq, cap=1 << 18, threads=16)[0]])
    return want


def device_passes(c, devs, lens, flush_before, depth):
    """The captures in order, `depth` in flight (1: blocking calls); the context's filter is flushed first."""
    c.icao_flush()
    got = []
    for k, d in enumerate(devs):
        if k in flush_before:
            c.icao_flush()
        if depth == 1:
            got.append([key(m) for m in c.demod_iq_device(d.data_ptr(), lens[k], cap=1 << 18)])
            continue
        if c.pending() == depth:
            got.append([key(m) for m in c.collect(cap=1 << 18)])
        c.submit_iq_device(d.data_ptr(), lens[k])
    while c.pending():
        got.append([key(m) for m in c.collect(cap=1 << 18)])
    return got


def to_device(caps):
    import torch
    devs = [torch.from_numpy(np.ascontiguousarray(iq)).cuda() for iq in caps]
    torch.cuda.synchronize()
    return devs


def mismatches(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


# ----------------------------------------------------------------------------- 1. edge geometry
# A context of more than 16 buffers leaves the sparse path (host-ordered hits, the plain scan) for device-side ordering once
# a pass leaves 8 records per buffer or more (adsb_collect.cpp: dense_mode), and a frame leaves several records -- every
# trial phase and neighbouring position it decodes at.  The captures here stay far below that: a handful of frames on noise.
N_EDGE_CAPS = 5


def edge_captures(n_buf: int, n: int, seed: int) -> list:
    """N_EDGE_CAPS captures of n samples, noise plus frames of a few aircraft started around every kind of edge a tile
    has, dealt over the captures: DF17 and DF11 (which teach) and address/parity replies to the same aircraft (which
    the match finds, in the pass that taught them or a later one)."""
    pool = [0x4A0000 + q * 0x1111 for q in range(5)]
    frames = lambda k: (synth.df17_frame(pool[k % 5], 0x23456789ABCDE * (k + 1)), synth.df11_frame(pool[k % 5]),
                        ap_frame((DF4, DF20, DF5, DF21)[k % 4], pool[k % 5]))[k % 3]
    starts = []
    # across tile edges: the preamble on one side, the message (up to REACH samples) reaching into the next tile
    for t, d in enumerate((-289, -250, -170, -120, -60, -19, -8, -1, 0, 1, 7, 40), start=1):
        starts.append(CHUNK * (t % n_buf) + TILE * t + d)
    # ... the edge between the last whole tile of a buffer and its short seventeenth
    starts += [CHUNK * 2 + 16 * TILE - 100, CHUNK * 5 + 16 * TILE + 3]
    # across buffer edges, and in the last REACH positions of a buffer (the reference has no carry-over: it sees the
    # samples behind the buffer's end as zero; the oracle says what is left of such a frame)
    for b, d in ((1, -400), (2, -REACH), (3, -289), (4, -200), (6, -120), (7, -30), (8, -1), (9, 0), (10, 2)):
        starts.append(CHUNK * b + d)
    caps = []
    for i in range(N_EDGE_CAPS):
        iq = synth.noise_numpy(n, seed=seed + i)
        # the end of the capture itself, in every capture: the last positions of a full last buffer or of a ragged
        # one, and a frame the end cuts
        mine = starts[i::N_EDGE_CAPS] + [n - 700 - 40 * i, n - REACH - 10 + i, n - 150 - i]
        bursts = [at(s, k + i, frames(k + i), amp=15000 + 1000 * ((k + i) % 9)) for k, s in enumerate(mine) if 0 <= s < n - 20]
        # a frame well inside the first buffer, so that every capture of every length has one that decodes; in the
        # first capture a reply in front of the frame that teaches its address as well
        bursts.append(at(97000, 2, synth.df17_frame(0x4BEEF1, 0x600DF00D + i)))
        bursts.append(at(2600, 1, ap_frame(DF5, 0x4BEEF1)))
        synth.add_bursts(iq, bursts)
        caps.append(iq)
    return caps


EDGE_CASES = {
    # name: (buffers of the context, samples, profiling level)
    "full17": (17, 17 * CHUNK, 1),
    "ragged17": (17, 16 * CHUNK + 50001, 1),             # a last buffer that ends inside its seventh tile
    "ragged34_past_a_tile_edge": (34, 33 * CHUNK + 3 * TILE + 100, 1),
    "short_last_tile": (18, 17 * CHUNK + 3, 1),          # a last buffer of three samples
    # one buffer plus one sample: a pass this small goes out as ONE launch (k_scan_fast<.., FUSED>) at the default
    # profiling level; at level 2, which keeps the kernels of a pass apart, it is three launches and its scan -- 34
    # tiles, fewer workgroups than fit the device, tiles dealt round robin -- is the new kernel's
    "one_buffer_plus_one_sample": (17, CHUNK + 1, 2),
}


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_frames_at_tile_edges_buffer_edges_and_the_ragged_end(hip_lib, oracle_mod, case):
    from dump1090_rs_amd import Context
    n_buf, n, level = EDGE_CASES[case]
    caps = edge_captures(n_buf, n, seed=9300 + 10 * n_buf)
    flush_before = {0, 3}          # passes 1, 2 and 4 know the aircraft from the passes before them
    want = oracle_passes(oracle_mod, caps, flush_before)
    replies = lambda w: sum(m[5][0] >> 3 in (4, 5, 20, 21) for m in w)
    assert all(len(w) >= 2 for w in want) and replies(want[0]) < replies(want[1])   # (the reply in front of its teacher)
    devs = to_device(caps)
    with Context(0, n_buf) as c:
        c.set_profiling(level)
        for depth in (1, 4):
            before = sparse_scans(c)
            got = device_passes(c, devs, [n] * len(caps), flush_before, depth)
            assert got == want, (depth, mismatches(got, want))
            # every pass ran the new kernel (the records of the last one: far from 8 per buffer)
            assert sparse_scans(c) - before == len(caps), (depth, c.stats()["n_records"])
            assert c.stats()["retries"] == 0


# ----------------------------------------------------------------------------- 2. the filter from pass to pass
@pytest.mark.parametrize("n_buf", [17, 24])
def test_teach_then_replies_without_a_flush_then_a_flush(hip_lib, oracle_mod, n_buf):
    """Pass A teaches addresses (DF11 / DF17); pass B of the same context, no flush between, holds only address/parity
    replies (DF4 / 5 / 20 / 21) of those aircraft: the new kernel's scans set the bits and list the entries the match
    works on.  Then a flush and pass C: it starts on the next bitmap, and the clear of the retired one rides on it
    (ScanParams::clean_bitmap) -- B's replies are gone from it, the teachers it has are heard."""
    from dump1090_rs_amd import Context
    n = n_buf * CHUNK
    pool = [0x3C0000 + q * 0x2F1 for q in range(8)]
    a = synth.noise_numpy(n, seed=9400 + n_buf)
    synth.add_bursts(a, [at(CHUNK * (2 * k % n_buf) + 20000 + 3001 * k, k,
                            synth.df11_frame(pool[k]) if k % 3 == 0 else synth.df17_frame(pool[k], 0x1F2E3D4C5B * (k + 1)))
                         for k in range(8)])
    b = synth.noise_numpy(n, seed=9401 + n_buf)
    synth.add_bursts(b, [at(CHUNK * ((k + 1) % n_buf) + 9000 + 2503 * k, k, ap_frame((DF4, DF5, DF20, DF21)[k % 4], pool[k % 8]))
                         for k in range(12)])
    cc = b.copy()   # C: B's replies (nobody has taught their addresses any more) and a few teachers of its own
    synth.add_bursts(cc, [at(CHUNK * k + 100000, k, synth.df17_frame(pool[k % 8], 77 + k)) for k in range(0, n_buf, 6)])
    caps = [a, b, cc]
    flush_before = {2}
    want = oracle_passes(oracle_mod, caps, flush_before)
    replies = lambda w: sum(m[5][0] >> 3 in (4, 5, 20, 21) for m in w)
    assert len(want[0]) >= 7 and replies(want[0]) == 0 and replies(want[1]) >= 10
    assert replies(want[2]) < replies(want[1])               # the flush took the addresses away
    devs = to_device(caps)
    with Context(0, n_buf) as c:
        for depth in (1, 4):
            before = sparse_scans(c)
            got = device_passes(c, devs, [n] * 3, flush_before, depth)
            assert got == want, (depth, mismatches(got, want))
            assert sparse_scans(c) - before == 3, (depth, c.stats()["n_records"])
            assert c.stats()["retries"] == 0


# ----------------------------------------------------------------------------- 3. passes the new kernel must not take
N_INEL = 17


@pytest.fixture(scope="module")
def sparse17():
    """A sparse 17-buffer capture with a few teachers and replies (far from the 8 records per buffer at which a context
    turns to device-side ordering), shared read-only by the tests below."""
    n = N_INEL * CHUNK
    iq = synth.noise_numpy(n, seed=9500)
    pool = [0xA00000 + q * 0x101 for q in range(3)]
    synth.add_bursts(iq, [at(CHUNK * b + 30000 + 77 * k, k, synth.df11_frame(pool[k % 3]) if k == 2 else synth.df17_frame(pool[k % 3], 0xC0FFEE * (k + 1)))
                          for k, b in enumerate((0, 1, 4, 9, 15, 16))])
    synth.add_bursts(iq, [at(CHUNK * b + 70000 + 13 * k, k, ap_frame((DF4, DF21, DF20)[k % 3], pool[k % 3])) for k, b in enumerate((1, 6, 12))])
    iq.setflags(write=False)
    return iq


def test_carry_over_passes_stay_on_k_scan_fast(hip_lib, oracle_mod, sparse17):
    import torch
    from dump1090_rs_amd import Context
    from oracle.binding import demod_iq_carry
    n = len(sparse17)
    iq = np.array(sparse17)
    synth.add_bursts(iq, [at(CHUNK * b - 100, b, synth.df17_frame(0xABCDEF, 1000 + b)) for b in (3, 9)])   # heard only with the carry
    orc, carry = oracle_mod.Oracle(), np.zeros((326, 2), np.int16)
    want = [[want_key(w) for w in demod_iq_carry(orc, iq, carry, cap=1 << 18)[0]] for _ in range(2)]
    plain = [want_key(w) for w in oracle_mod.Oracle().demod_iq(iq, cap=1 << 18, threads=16)[0]]
    assert len(want[0]) > len(plain)
    dev = torch.from_numpy(iq).cuda()
    with Context(0, N_INEL) as c:
        c.set_carry_over(True)
        c.icao_flush()
        for k in range(2):    # (the second call's first buffer takes its lead-in from ScanParams::carry)
            assert [key(m) for m in c.demod_iq_device(dev.data_ptr(), n, cap=1 << 18)] == want[k], k
        assert sparse_scans(c) == 0
        c.set_carry_over(False)
        c.icao_flush()
        assert [key(m) for m in c.demod_iq_device(dev.data_ptr(), n, cap=1 << 18)] == plain
        assert sparse_scans(c) == 1


@pytest.mark.parametrize("mode", [1, 3])
def test_error_correcting_passes_stay_on_their_fix_kernels(hip_lib, sparse17, mode):
    import torch
    from dump1090_rs_amd import Context
    from tests import fix2_support as f2, fix_support as fs
    n = len(sparse17)
    iq = np.array(sparse17)
    icao = 0x71C0DE
    clean = synth.df17_frame(icao, 0x5A5A5A5A5A5A5)
    two = fs.flip(fs.flip(clean, 41), 77)
    synth.add_bursts(iq, [at(CHUNK * 2 + 5000, 1, clean), at(CHUNK * 6 + 5000, 2, fs.flip(clean, 50)), at(CHUNK * 11 + 5000, 3, two)])
    want = f2.Restated(mode).demod_iq(iq)
    # (mode 1 repairs the one-bit copy, mode 3 the two-bit copy as well)
    assert len(want) > len(f2.Restated(0 if mode == 1 else 1).demod_iq(iq))
    dev = torch.from_numpy(iq).cuda()
    with Context(0, N_INEL) as c:
        c.set_error_correction(mode)
        c.icao_flush()
        assert [fs.key(m) for m in c.demod_iq_device(dev.data_ptr(), n, cap=1 << 18)] == want
        assert sparse_scans(c) == 0


def test_cu8_passes_stay_on_the_cu8_kernel(hip_lib, oracle_mod, sparse17):
    import torch
    from dump1090_rs_amd import Context
    from tests.test_u8_cpu import t_soapy_numpy
    b = np.ascontiguousarray(np.clip(np.rint(sparse17 / 256.0 + 127.4), 0, 255).astype(np.uint8))
    wide = np.ascontiguousarray(t_soapy_numpy()[b.reshape(-1, 2)])
    want = [want_key(w) for w in oracle_mod.Oracle().demod_iq(wide, cap=1 << 18, threads=16)[0]]
    assert len(want) >= 5
    d8 = torch.from_numpy(b).cuda()
    with Context(0, N_INEL) as c:
        c.icao_flush()
        assert [key(m) for m in c.demod_iq_device_u8(d8.data_ptr(), len(b), cap=1 << 18)] == want
        assert sparse_scans(c) == 0


def test_a_dense_stream_leaves_the_new_kernel_when_the_device_orders_its_hits(hip_lib, oracle_mod):
    """The first pass of a dense stream is submitted in sparse mode (the new kernel, host-ordered); it switches the
    context to device-side ordering and scoring, and the passes behind it run the FIELDS instantiation of k_scan_fast."""
    import torch
    from dump1090_rs_amd import Context
    n = N_INEL * CHUNK
    iq = synth.make_iq(n, n_bursts=40 * N_INEL, seed=9600, n_icao=25, df11_every=4)
    want = oracle_passes(oracle_mod, [iq] * 3, {0})
    assert len(want[0]) > 8 * N_INEL
    dev = torch.from_numpy(iq).cuda()
    with Context(0, N_INEL) as c:
        c.icao_flush()
        for k in range(3):
            assert [key(m) for m in c.demod_iq_device(dev.data_ptr(), n, cap=1 << 18)] == want[k], k
            assert sparse_scans(c) == 1, k
        assert c.stats()["retries"] == 0


def test_caller_magnitudes_small_passes_small_contexts_and_the_self_test(hip_lib, oracle_mod, sparse17):
    import torch
    from dump1090_rs_amd import Context
    n = len(sparse17)
    dev = torch.from_numpy(np.array(sparse17)).cuda()
    orc = oracle_mod.Oracle()
    one = sparse17[CHUNK:2 * CHUNK]
    data, length = orc.to_mag(one)
    want_mag = [want_key(w) for w in orc.demodulate2400(data, length)[0]]
    want16 = [want_key(w) for w in oracle_mod.Oracle().demod_iq(sparse17[:16 * CHUNK], cap=1 << 18, threads=16)[0]]
    stages = oracle_mod.stage_lists(sparse17)
    assert len(want_mag) >= 1 and len(want16) >= 5
    with Context(0, N_INEL) as c:
        # a caller's MagnitudeBuffer (adsb_demodulate2400)
        c.icao_flush()
        mag = c.to_mag(one)
        assert np.array_equal(mag.data, data)
        assert [key(m) for m in c.demodulate2400(mag)] == want_mag
        assert sparse_scans(c) == 0
        # a pass of no more than 16 buffers in the large context: one launch
        c.icao_flush()
        assert [key(m) for m in c.demod_iq_device(dev.data_ptr(), 16 * CHUNK, cap=1 << 18)] == want16
        assert sparse_scans(c) == 0
        # the self-test's stage lists (the SELFTEST instantiation), over all seventeen buffers
        cand, ap = c.selftest_stage_lists(dev.data_ptr(), n)
        assert cand.tolist() == stages["cand"] and ap.tolist() == stages["ap"]
        pre, snr = c.selftest_gate_stages(dev.data_ptr(), n)
        assert pre.tolist() == stages["preamble"] and snr.tolist() == stages["snr"]
        assert sparse_scans(c) == 0
    with Context(0, 16) as c:   # a context for passes of a few buffers: folded bitmaps, one-launch passes
        c.icao_flush()
        assert [key(m) for m in c.demod_iq_device(dev.data_ptr(), 16 * CHUNK, cap=1 << 18)] == want16
        assert sparse_scans(c) == 0


# ----------------------------------------------------------------------------- 4. the switch
def test_the_switch_takes_the_same_stream_through_k_scan_fast(hip_lib, oracle_mod):
    import torch
    from dump1090_rs_amd import Context, _lib
    n_buf = 20
    n = n_buf * CHUNK - 4321
    caps = edge_captures(n_buf, n, seed=9700)[:4]
    flush_before = {0, 2}
    want = oracle_passes(oracle_mod, caps, flush_before)
    devs = to_device(caps)
    lists = {}
    with Context(0, n_buf) as c:
        for on in (False, True, False):
            set_sparse_scan(c, on)
            before = sparse_scans(c)
            for depth in (1, 4):
                got = device_passes(c, devs, [n] * 4, flush_before, depth)
                assert got == want, (on, depth, mismatches(got, want))
                lists.setdefault(on, got)
            assert sparse_scans(c) - before == (8 if on else 0), on
        assert lists[False] == lists[True]
        # the switch is refused while passes are in flight, like every other mode of a context
        c.submit_iq_device(devs[0].data_ptr(), n)
        assert c._L.adsb_selftest_set_sparse_scan(c._h, 0) == _lib.ADSB_ERR_BUSY
        c.collect(cap=1 << 18)
    assert hip_lib.adsb_selftest_set_sparse_scan(None, 1) == _lib.ADSB_ERR_INVALID and hip_lib.adsb_selftest_sparse_scans(None) == 0

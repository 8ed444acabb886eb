"""The tail of a sparse stream's three-launch pass in a large context (more than 16 buffers, host-ordered hits): the match
is k_match_sparse and the records kernel a small fixed grid (adsb_aux.hip: launch_match / launch_records, `sparse_fast`).
Everything against the CPU oracle, exactly: frames, order, (chunk, j, try_phase, score), signal_level bits; `retries == 0`
where the pass must not have been redone (the host found the records' checksum as the device summed it).

Shapes: 17 buffers is the smallest pass that is not one launch; 24 buffers for the hit counts around the records grid
(72 blocks: `per = ceil(hits / 72)` changes at 72 / 73 hits)."""
import numpy as np
import pytest

from dump1090_rs_amd import synth

pytestmark = pytest.mark.gpu

CHUNK = 131072
REC_BLOCKS = 72   # adsb_aux.hip: ADSB_REC_SPARSE_BLOCKS


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msg, m.signal_level)


def want_key(w):
    return (w["chunk"], w["j"], w["try_phase"], w["score"], w["msg"], w["signal_level"])


def ap_frame(first_bytes: bytes, icao: int) -> bytes:
    return first_bytes + (synth.crc24(first_bytes) ^ icao).to_bytes(3, "big")


DF4 = bytes([0x20, 0x00, 0x05, 0x30])
DF5 = bytes([0x28, 0x00, 0x1A, 0x2B])
DF20 = bytes([0xA0, 0x00, 0x05, 0x30, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77])
DF21 = bytes([0xA8, 0x00, 0x1A, 0x2B, 0x70, 0x61, 0x52, 0x43, 0x34, 0x25, 0x16])


def at(sample, k, frame, amp=20000):
    """`frame` starting at `sample` (sub-sample phase and carrier angle from k)"""
    return synth.Burst(5 * sample + k % 5, amp, k % 16, frame)


def oracle_passes(oracle_mod, caps, flush_before):
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
        if depth == 1 or lens[k] == 0:   # (no samples: nothing to submit -- the blocking call, behind what is in flight)
            while c.pending():
                got.append([key(m) for m in c.collect(cap=1 << 18)])
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
    devs = [torch.from_numpy(np.ascontiguousarray(iq)).cuda() if len(iq) else torch.zeros((8, 2), dtype=torch.int16, device="cuda")
            for iq in caps]
    torch.cuda.synchronize()
    return devs


def mismatches(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


# ----------------------------------------------------------------------------- plain sparse passes
@pytest.mark.parametrize("n_buf", [17, 18, 40])
def test_sparse_passes_blocking_and_in_flight_with_and_without_flushes(hip_lib, oracle_mod, n_buf):
    """Six passes over two captures whose address/parity replies need addresses their DF17 / DF11 frames teach: with an
    icao_flush before every pass (each clears the bitmap the flush before retired) and with none (the superset carries
    over and nothing is cleared), blocking and four in flight."""
    from dump1090_rs_amd import Context
    n = n_buf * CHUNK
    caps = []
    for s in range(2):
        iq = synth.make_iq(n, n_bursts=6 * n_buf, seed=7100 + 10 * n_buf + s, n_icao=9, df11_every=4)
        pool = [0xA00000 + q * 0x101 for q in range(9)]
        synth.add_bursts(iq, [at(CHUNK * (k % n_buf) + 50000 + 997 * k, k, ap_frame((DF4, DF20, DF5, DF21)[k % 4], pool[k % 9]))
                              for k in range(3 * n_buf)])
        caps.append(iq)
    caps = [caps[k % 2] for k in range(6)]
    devs, lens = to_device(caps), [n] * 6
    for flush_before in (set(range(6)), set()):
        want = oracle_passes(oracle_mod, caps, flush_before)
        assert any(len(w) > 3 * n_buf for w in want)
        with Context(0, n_buf) as c:
            for depth in (1, 4):
                got = device_passes(c, devs, lens, flush_before, depth)
                assert got == want, (sorted(flush_before), depth, mismatches(got, want))
                assert c.stats()["retries"] == 0


# ----------------------------------------------------------------------------- long and short entries, segment by segment
@pytest.mark.parametrize("kind", ["short", "long", "mixed"])
@pytest.mark.parametrize("background", ["quiet", "noise"])
def test_replies_whose_address_is_taught_elsewhere(hip_lib, oracle_mod, kind, background):
    """DF4 / DF5 (56-bit) and DF20 / DF21 (112-bit) replies whose address a DF17 teaches later in the same pass, in the
    last tile of the last buffer, and in an earlier pass still in flight.  On a quiet background the only list entries
    are the injected frames': a wave segment then holds short entries only, long ones only, or both (`kind`)."""
    from dump1090_rs_amd import Context
    n_buf = 18
    n = n_buf * CHUNK
    replies = {"short": (DF4, DF5), "long": (DF20, DF21), "mixed": (DF4, DF20, DF5, DF21)}[kind]
    a_early, a_late, a_last, a_prev = 0x4B1A2C, 0x3C6589, 0x7C0FFE, 0x89ABCD

    def base(seed):
        return synth.noise_numpy(n, seed=seed) if background == "noise" else np.zeros((n, 2), dtype=np.int16)

    first, second = base(8101), base(8102)
    # pass 0: teaches a_prev only
    synth.add_bursts(first, [at(3 * CHUNK + 4000, 1, synth.df17_frame(a_prev, 11)), at(9 * CHUNK + 70000, 2, synth.df17_frame(a_prev, 12))])
    # pass 1: replies for all four addresses spread over the buffers, the teachers of three of them inside it
    bursts = [at(2 * CHUNK + 30000, 3, synth.df17_frame(a_early, 21)),                 # early: the replies behind it decode
              at(13 * CHUNK + 90000, 4, synth.df17_frame(a_late, 22)),                 # late: only the replies behind this
              at(n - 1200, 5, synth.df17_frame(a_last, 23))]                           # the last tile of the last buffer
    k = 0
    for b in range(n_buf):
        for off in (1500, 41000, 77000, 120000):
            addr = (a_early, a_late, a_last, a_prev)[k % 4]
            bursts.append(at(b * CHUNK + off + 13 * k, k, ap_frame(replies[(k // 4) % len(replies)], addr)))
            k += 1
    synth.add_bursts(second, bursts)
    caps = [first, second, second]
    devs, lens = to_device(caps), [n] * 3
    want = oracle_passes(oracle_mod, caps, set())
    def decoded(w, addr):   # replies to `addr` among the messages (a message's bytes past its length are not the frame's)
        return sum(any(m[4][:len(r) + 3] == ap_frame(r, addr) for r in replies) for m in w)

    assert decoded(want[1], a_prev) > 10 and decoded(want[1], a_early) > decoded(want[1], a_late) > 0
    assert decoded(want[1], a_last) == 0 < decoded(want[2], a_last)   # (every reply lies before the last tile's DF17)
    assert len(want[2]) > len(want[1])            # the second time round every address is known from the start
    with Context(0, n_buf) as c:
        for depth in (1, 4):
            got = device_passes(c, devs, lens, set(), depth)
            assert got == want, (depth, mismatches(got, want))
            assert c.stats()["retries"] == 0


# ----------------------------------------------------------------------------- ragged and empty
def test_ragged_last_buffer_and_empty_passes(hip_lib, oracle_mod):
    """A last buffer of less than one tile, of a few tiles and a sample short of full, in passes of more than 16 buffers;
    passes of no samples and of less than one tile between them (one-launch passes of the same context: the slots'
    counters and the bitmaps go from one kind of pass to the other)."""
    from dump1090_rs_amd import Context
    full = synth.make_iq(18 * CHUNK, n_bursts=120, seed=8300, n_icao=7, df11_every=3)
    synth.add_bursts(full, [at(CHUNK * k + 60000, k, ap_frame((DF4, DF21)[k % 2], 0xA00000 + (k % 7) * 0x101)) for k in range(18)])
    lens = [17 * CHUNK + 1, 0, 17 * CHUNK + 3000, 700, 17 * CHUNK + 40000, 18 * CHUNK - 1, 0, 16 * CHUNK + 5, 18 * CHUNK]
    caps = [full[:m] for m in lens]
    devs = to_device(caps)
    for flush_before in (set(range(len(lens))), {0, 4}):
        want = oracle_passes(oracle_mod, caps, flush_before)
        assert want[1] == [] and len(want[-1]) > 100
        with Context(0, 18) as c:
            for depth in (1, 4):
                got = device_passes(c, devs, lens, flush_before, depth)
                assert got == want, (sorted(flush_before), depth, mismatches(got, want))
                assert c.stats()["retries"] == 0


# ----------------------------------------------------------------------------- hit counts around the records grid
N_GRID_BUF = 24


@pytest.fixture(scope="module")
def burst_pool(hip_lib):
    """Patches of a quiet 24-buffer capture, far apart -- 96 strong bursts, and 24 faint ones inside 2000 samples of noise,
    which decode at one or two phases only -- and the number of records (hits) each leaves when it is alone in the
    capture: the device's own count, used only to compose inputs with a wanted number of hits; what the passes over
    those inputs return is judged against the oracle.  (sample offset, samples) per patch."""
    import torch
    from dump1090_rs_amd import Context
    n = N_GRID_BUF * CHUNK
    pool = []
    for k in range(96):
        frame = synth.df11_frame(0x500000 + k * 0x10F) if k % 3 == 2 else synth.df17_frame(0x500000 + k * 0x10F, 0x1234567 * (k + 1))
        b = at(CHUNK * (k % N_GRID_BUF) + 9000 + 25000 * (k // N_GRID_BUF) + 17 * k, k, frame, amp=9000 + 2500 * (k % 8))
        patch = np.zeros((320, 2), dtype=np.int16)
        synth.add_bursts(patch, [b], first_sample=b.tick // 5)
        pool.append((b.tick // 5, patch))
    for b in range(N_GRID_BUF):   # (past every strong burst's place in the buffer)
        patch = synth.noise_numpy(2000, seed=9100 + b)
        synth.add_bursts(patch, [synth.Burst(5 * 800 + b % 5, 7000 + 200 * b, b % 16, synth.df17_frame(0x600000 + b * 0x111, 0xABCDEF123 * (b + 1)))])
        pool.append((CHUNK * b + 99000, patch))
    dev = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
    counts = []
    with Context(0, N_GRID_BUF) as c:
        for s0, patch in pool:
            dev[s0:s0 + len(patch)] = torch.from_numpy(patch).cuda()
            torch.cuda.synchronize()
            c.icao_flush()
            c.demod_iq_device(dev.data_ptr(), n)
            counts.append(int(c.stats()["n_records"]))
            dev[s0:s0 + len(patch)] = 0
    return pool, counts


def choose(counts, target):
    """indices of a subset of `counts` that sums to `target` (subset sum), or None"""
    reach = {0: []}
    for i, r in enumerate(counts):
        if r <= 0:
            continue
        for s, idx in list(reach.items()):
            if s + r <= target and s + r not in reach:
                reach[s + r] = idx + [i]
        if target in reach:
            return reach[target]
    return reach.get(target)


@pytest.mark.parametrize("hits", [0, 1, REC_BLOCKS - 1, REC_BLOCKS, REC_BLOCKS + 1])
def test_hit_counts_around_the_records_grid(hip_lib, oracle_mod, burst_pool, hits):
    """A pass that ends with exactly 0, 1, 71, 72 and 73 hits (72 blocks take ceil(hits / 72) each), in sparse mode; then
    five more passes, which come round to the same slot: its counters were left zero and -- a flush before each -- the
    bitmap it retired was cleared by the small grid."""
    import torch
    from dump1090_rs_amd import Context
    pool, counts = burst_pool
    n = N_GRID_BUF * CHUNK
    idx = choose(counts, hits)
    assert idx is not None, (hits, counts)
    iq = np.zeros((n, 2), dtype=np.int16)
    for i in idx:
        iq[pool[i][0]:pool[i][0] + len(pool[i][1])] = pool[i][1]
    follow = synth.make_iq(n, n_bursts=40, seed=8400 + hits, n_icao=5, df11_every=3)
    caps = [iq] + [follow, iq] * 3
    flush_before = set(range(len(caps)))
    want = oracle_passes(oracle_mod, caps, flush_before)
    devs = to_device([iq, follow])
    with Context(0, N_GRID_BUF) as c:
        c.icao_flush()
        got = [key(m) for m in c.demod_iq_device(devs[0].data_ptr(), n)]
        st = c.stats()
        assert st["n_records"] == hits and st["retries"] == 0
        assert got == want[0]
        for depth in (1, 4):
            got = device_passes(c, [devs[k % 2] for k in range(len(caps))], [n] * len(caps), flush_before, depth)
            assert got == want, (depth, mismatches(got, want))
            assert c.stats()["retries"] == 0


def test_two_thousand_hits_in_sparse_mode(hip_lib, oracle_mod):
    """About 2 000 hits in a pass submitted while the context is in sparse mode: runs of ~28 hits per block of the small
    grid; the passes behind it (the first of them device-ordered: the context has seen a dense pass) are right too."""
    from dump1090_rs_amd import Context
    n = N_GRID_BUF * CHUNK
    busy = synth.make_iq(n, n_bursts=700, seed=8500, n_icao=30, df11_every=4)
    quiet = synth.make_iq(n, n_bursts=12, seed=8501, n_icao=30)
    caps = [quiet, busy, quiet, quiet, busy, quiet, quiet]
    devs = to_device([quiet, busy])
    pick = [0, 1, 0, 0, 1, 0, 0]
    for flush_before in (set(range(len(caps))), {0}):
        want = oracle_passes(oracle_mod, caps, flush_before)
        with Context(0, N_GRID_BUF) as c:
            c.icao_flush()
            c.demod_iq_device(devs[0].data_ptr(), n)
            c.icao_flush()
            c.demod_iq_device(devs[1].data_ptr(), n)
            st = c.stats()
            assert 1000 <= st["n_records"] <= 5000 and st["retries"] == 0, st   # ("about 2 000": 14 to 70 per block)
            for depth in (1, 4):
                got = device_passes(c, [devs[k] for k in pick], [n] * len(caps), flush_before, depth)
                assert got == want, (sorted(flush_before), depth, mismatches(got, want))
                assert c.stats()["retries"] == 0


# ----------------------------------------------------------------------------- overflow
def test_more_hits_than_the_list_holds_redoes_the_pass(hip_lib, oracle_mod):
    """Seventeen buffers of frames back to back leave more hits than hits_cap (4096 + 17 * 1024): k_match_sparse and the
    scan flag the overflow, the pass is redone buffer by buffer, and the pass behind it starts from clean counters."""
    from dump1090_rs_amd import Context
    n_buf = 17
    n = n_buf * CHUNK
    iq = synth.noise_numpy(n, seed=8600)
    bursts = []
    for k in range(n // 300 - 2):
        icao = 0x400000 + (k % 37) * 0x101
        kind = k % 4
        frame = (synth.df17_frame(icao, k) if kind in (0, 1) else synth.df11_frame(icao) if kind == 2 else ap_frame(DF4, icao))
        bursts.append(synth.Burst(5 * (300 * k + 40) + k % 5, 18000 + 500 * (k % 9), k, frame))
    synth.add_bursts(iq, bursts)
    quiet = synth.make_iq(n, n_bursts=30, seed=8601, n_icao=5, df11_every=3)
    caps = [quiet, iq, quiet]
    want = oracle_passes(oracle_mod, caps, {0, 1, 2})
    assert len(want[1]) > 300 * n_buf
    devs = to_device(caps)
    with Context(0, n_buf) as c:
        c.icao_flush()
        assert [key(m) for m in c.demod_iq_device(devs[0].data_ptr(), n)] == want[0]
        c.icao_flush()
        got = [key(m) for m in c.demod_iq_device(devs[1].data_ptr(), n, cap=1 << 18)]
        assert c.stats()["retries"] > 0           # (the context was in sparse mode: the host-ordered tail overflowed)
        assert got == want[1]
        c.icao_flush()
        assert [key(m) for m in c.demod_iq_device(devs[2].data_ptr(), n)] == want[2]
        assert c.stats()["retries"] == 0

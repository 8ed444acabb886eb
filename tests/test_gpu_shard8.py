"""BASELINE config 4 on the GPU: ONE capture cut EIGHT ways.

The reference's loop (dump1090_rs/src/main.rs:161-167) is one stream with one process-global ICAO
filter (src/icao_filter.rs:8-9) -- the only thing that couples the shards.  Here eight contexts on the
one GPU of the test box stand in for eight GPUs: uneven contiguous buffer ranges (38 buffers as
5,5,5,5,5,5,4,4, the last buffer ragged), addresses learned in one shard that frames in other shards
need, and a filter that is not empty when the capture starts.  Every result is compared with the CPU
oracle over the whole capture AND with the single-stream GPU result.
"""
import os
import sys

import numpy as np
import pytest

from dump1090_rs_amd import sharding, synth
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK = 131072
WORLD = 8
PIPELINE_RANKS = 4                   # rank processes of the gloo test, each with the GPU open
N_SAMPLES = 37 * CHUNK + 4321        # 38 buffers, the last one ragged
ICAO_A, ICAO_B, ICAO_C = 0x4840D6, 0x3C6589, 0x7C1B2A


def _ap_frame(first_bytes: bytes, icao: int) -> bytes:
    """An address/parity frame (mode_s/mod.rs:56-72, 110-135): parity = CRC of the body XOR the address."""
    return first_bytes + (synth.crc24(first_bytes) ^ icao).to_bytes(3, "big")


DF4_A = _ap_frame(bytes([0x20, 0x00, 0x05, 0x30]), ICAO_A)
DF4_B = _ap_frame(bytes([0x20, 0x00, 0x07, 0x11]), ICAO_B)
DF20_C = _ap_frame(bytes([0xA0, 0x00, 0x05, 0x30, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77]), ICAO_C)


def coupled_capture8(seed: int = 4108):
    """38 buffers whose result depends on the filter across shard boundaries (ranges 5,5,5,5,5,5,4,4:
    shard r starts at buffer 0,5,10,15,20,25,30,34):
      A  taught by a DF17 in buffer 7 (shard 1).  Its DF4 in buffer 2 (shard 0, too early: dropped),
         buffer 8 (shard 1), buffer 31 (shard 6) and the ragged buffer 37 (shard 7);
      B  already in the filter when the capture starts (the preface).  Its DF4 in buffers 0 and 27;
      C  taught by a DF11 with IID 0 in buffer 16 (shard 3).  A 112-bit DF20 for it in buffer 12 (shard
         2, too early) and buffer 22 (shard 4)."""
    iq = synth.make_iq(N_SAMPLES, n_bursts=300, seed=seed, n_icao=12, df11_every=4)
    at = lambda chunk, j: 5 * (chunk * CHUNK + j)
    synth.add_bursts(iq, [
        synth.Burst(at(0, 3000), 21000, 4, DF4_B),
        synth.Burst(at(2, 20000), 22000, 1, DF4_A),
        synth.Burst(at(7, 60000) + 2, 22000, 2, synth.df17_frame(ICAO_A, 77)),
        synth.Burst(at(8, 90000) + 1, 22000, 5, DF4_A),
        synth.Burst(at(12, 40000) + 3, 23000, 6, DF20_C),
        synth.Burst(at(16, 1000) + 4, 23000, 7, synth.df11_frame(ICAO_C)),
        synth.Burst(at(22, 100000), 23000, 8, DF20_C),
        synth.Burst(at(27, 130000), 21000, 9, DF4_B),
        synth.Burst(at(31, 5000) + 2, 22000, 9, DF4_A),
        synth.Burst(at(37, 1000) + 1, 22000, 3, DF4_A)])
    return iq


def preface_capture():
    """One buffer that teaches B before the capture starts (the filter is never flushed in between,
    as in main.rs:154-167)."""
    iq = synth.make_iq(CHUNK, n_bursts=0, seed=91)
    synth.add_bursts(iq, [synth.Burst(5 * 50000 + 3, 24000, 2, synth.df17_frame(ICAO_B, 5))])
    return iq


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msg, m.signal_level)


def want_key(w):
    return (w["chunk"], w["j"], w["try_phase"], w["score"], w["msg"], w["signal_level"])


def test_eight_way_shard_with_a_preloaded_filter_equals_single_stream_and_oracle(hip_lib, oracle_mod):
    """adsb_shard_scan on eight shards -> union of the learned addresses (+ what the filter already
    holds) -> adsb_shard_finish -> adsb_replay_records once, in global order, through the pre-loaded
    filter table."""
    import torch
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import replay_records

    iq, pre = coupled_capture8(), preface_capture()
    orc = oracle_mod.Oracle()
    orc.demod_iq(pre)
    want, _ = orc.demod_iq(iq)                       # the filter persists from the preface
    dev, dev_pre = torch.from_numpy(iq).cuda(), torch.from_numpy(pre).cuda()
    spans = [sharding.sample_range(N_SAMPLES, WORLD, r) for r in range(WORLD)]
    assert [(b - a + CHUNK - 1) // CHUNK for a, b in spans] == [5, 5, 5, 5, 5, 5, 4, 4]

    # single stream on the GPU
    with Context(0, 8) as solo:
        solo.icao_flush()
        solo.demod_iq_device(dev_pre.data_ptr(), CHUNK)
        single = solo.demod_iq_device(dev.data_ptr(), N_SAMPLES)
    assert [key(m) for m in single] == [want_key(w) for w in want]

    ctxs = [Context(0, 5) for _ in range(WORLD)]
    try:
        # the filter as the preface leaves it: table A of src/icao_filter.rs:8, 4096 u32
        table = np.zeros(4096, dtype=np.uint32)
        ctxs[0].icao_flush()
        ctxs[0].shard_scan(dev_pre.data_ptr(), CHUNK)
        replay_records(ctxs[0].shard_finish(np.zeros(0, np.uint32)), table)
        assert ICAO_B in table.tolist() and np.count_nonzero(table) == 1

        ptr = lambda a: dev.data_ptr() + 4 * a
        for c in ctxs:
            c.icao_flush()
        learned = [c.shard_scan(ptr(a), b - a) for c, (a, b) in zip(ctxs, spans)]
        assert ICAO_A in learned[1].tolist() and ICAO_C in learned[3].tolist()
        assert all(ICAO_A not in l.tolist() for r, l in enumerate(learned) if r != 1)
        union = np.unique(np.concatenate(learned + [table[table != 0] & np.uint32(0xFFFFFF)]))
        records = [c.shard_finish(union) for c in ctxs]
        merged = sharding.merge_records(records, [a // CHUNK for a, _ in spans])
        got = replay_records(merged, table)
        assert [key(m) for m in got] == [want_key(w) for w in want]
        assert [key(m) for m in got] == [key(m) for m in single]
        # the couplings really are in the capture
        chunks_of = lambda frame: sorted({m.chunk for m in got if m.buffer() == frame})
        assert chunks_of(DF4_A) == [8, 31, 37]          # not 2: A is not known yet
        assert chunks_of(DF4_B) == [0, 27]              # only because the filter held B already
        assert chunks_of(DF20_C) == [22]                # not 12
        assert ICAO_A in table.tolist() and ICAO_C in table.tolist()
        # without the preface the two B frames are lost, with an empty union A's and C's too
        for c in ctxs:
            c.icao_flush()
        learned = [c.shard_scan(ptr(a), b - a) for c, (a, b) in zip(ctxs, spans)]
        records = [c.shard_finish(np.unique(np.concatenate(learned))) for c in ctxs]
        cold = replay_records(sharding.merge_records(records, [a // CHUNK for a, _ in spans]))
        cold_want, _ = oracle_mod.Oracle().demod_iq(iq)
        assert [key(m) for m in cold] == [want_key(w) for w in cold_want]
        assert not [m for m in cold if m.buffer() == DF4_B]
    finally:
        for c in ctxs:
            c.close()


def test_shard_calls_from_a_worker_thread_use_the_contexts_device(hip_lib, oracle_mod):
    """sharding.ShardPipeline runs adsb_shard_finish on a worker thread, whose current HIP device is
    whatever the runtime defaults to: the entry points must select the context's device themselves
    (the advisor's round-3 finding; on this one-GPU box device 0 is the only one, so the check is that
    both phases work from threads that never touched HIP before)."""
    import threading
    import torch
    from dump1090_rs_amd import Context
    from dump1090_rs_amd.context import replay_records

    iq = synth.make_iq(3 * CHUNK - 777, n_bursts=40, seed=515, n_icao=6, df11_every=4)
    want, _ = oracle_mod.Oracle().demod_iq(iq)
    dev = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    box = {}
    with Context(0, 4) as c:
        c.icao_flush()

        def scan():
            box["learned"] = c.shard_scan(dev.data_ptr(), len(iq))

        def finish():
            box["records"] = c.shard_finish(box["learned"])

        for fn in (scan, finish):
            t = threading.Thread(target=fn)
            t.start()
            t.join(120)
            assert not t.is_alive()
        assert [key(m) for m in replay_records(box["records"])] == [want_key(w) for w in want]


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pipeline_rank(rank, world, port, seeds, q):
    """One of the ranks that share the GPU: sharding.ShardPipeline over its contiguous range of each
    capture (scan + address exchange on the main thread, finish + record gather + replay on the worker
    thread, two gloo host groups)."""
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    from dump1090_rs_amd import Context
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        a, b = sharding.sample_range(N_SAMPLES, world, rank)
        devs = [torch.from_numpy(np.ascontiguousarray(coupled_capture8(s)[a:b])).cuda() for s in seeds]
        torch.cuda.synchronize()
        ctxs = [Context(0, (b - a + CHUNK - 1) // CHUNK) for _ in range(2)]   # sized for this rank's range
        pipe = sharding.ShardPipeline(ctxs, dist)
        out = [pipe.submit(d.data_ptr(), b - a, a // CHUNK) for d in devs]
        out = out[2:] + pipe.drain()
        pipe.close()
        for c in ctxs:
            c.close()
        res = None if rank else [[key(m) for m in msgs] for msgs in out]
        q.put((rank, (a, b), res))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_four_ranks_over_gloo_through_the_shard_pipeline(hip_lib, oracle_mod):
    """Four processes, one GPU: the N = 4 form of `bench.py --workload shard` -- ShardPipeline, the
    address exchange and the record gather over gloo host groups -- on three captures, each result on
    rank 0 equal to the oracle's single stream (a flushed filter per capture).  Ranges 10,10,9,9, the
    last buffer ragged: A is learned in shard 0 and needed in shard 3, C learned in shard 1 and needed
    in shard 2.  (Four ranks, not eight: every rank and the test's own process hold the device open at
    once, and the suite keeps the processes on one GPU few; eight contexts in one process are the test
    above.)"""
    import queue
    import time
    import torch.multiprocessing as mp
    seeds = [4108, 4109, 4110]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_pipeline_rank, args=(r, PIPELINE_RANKS, port, seeds, q)) for r in range(PIPELINE_RANKS)]
    for p in procs:
        p.start()
    got = []
    try:
        deadline = time.monotonic() + 600
        while len(got) < len(procs) and time.monotonic() < deadline:
            try:
                got.append(q.get(timeout=2))
            except queue.Empty:
                # a rank that failed leaves the others waiting in a collective: stop here, not at the deadline
                if any(p.exitcode not in (None, 0) for p in procs):
                    break
    finally:
        for p in procs:
            p.join(timeout=120 if len(got) == len(procs) else 5)
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0] * len(procs) and len(got) == len(procs)
    got.sort()
    spans = [sharding.sample_range(N_SAMPLES, PIPELINE_RANKS, r) for r in range(PIPELINE_RANKS)]
    assert [(b - a + CHUNK - 1) // CHUNK for a, b in spans] == [10, 10, 9, 9]
    assert [g[1] for g in got] == spans
    assert all(g[2] is None for g in got[1:]) and len(got[0][2]) == len(seeds)
    for s, res in zip(seeds, got[0][2]):
        want, _ = oracle_mod.Oracle().demod_iq(coupled_capture8(s))
        assert res == [want_key(w) for w in want]
        assert sorted({k[0] for k, w in zip(res, want) if w["buffer"] == DF4_A}) == [8, 31, 37]

"""One fixed walk through every branch of the host side of a pass (csrc/adsb_pass.cpp: enqueue_pass and its steps).

    rocprofv3 --hip-trace --stats -d out -- python tools/pass_calls.py

Fixed pass counts and seeds: which branches a pass takes depends on host-side state and on the data, not on timing,
so two libraries that enqueue the same work show the same per-API call counts in the trace's statistics (polling calls
such as hipEventQuery / hipStreamQuery excepted).  Per leg it prints the frames and the context's host-side counters
(adsb_host_rematches / _sorts / _replays): a lost cross-stream edge shows there before it shows as a wrong frame.
Not a test; the library under the package directory is the one that runs.
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from dump1090_rs_amd import Context, MagnitudeBuffer, synth  # noqa: E402
from dump1090_rs_amd._lib import AdsbMsg  # noqa: E402

CHUNK = 131072
CAP = 1 << 20
OUT = (AdsbMsg * CAP)()
PERIOD = [18143, 6637, 18778, 14788, 3662, 8402, 2882, 16543]   # tests/test_gpu_parity.py: 25 % of all positions pass every gate


def report(leg, ctx, frames):
    L, h = ctx._L, ctx._h
    print(f"{leg}: {frames} frames, rematches {L.adsb_host_rematches(h)}, host sorts {L.adsb_host_sorts(h)}, "
          f"host replays {L.adsb_host_replays(h)}", flush=True)


def pipelined(ctx, submit, passes, depth=3, flush_each=False):
    frames = inflight = 0
    for i in range(passes):
        if flush_each:
            ctx.icao_flush()
        submit(i)
        inflight += 1
        if inflight >= depth:
            frames += ctx.collect_raw(OUT, CAP)
            inflight -= 1
    for _ in range(inflight):
        frames += ctx.collect_raw(OUT, CAP)
    return frames


def resident(chunks, passes, bursts, flush_each, profiling=1, u8=False, carry=False):
    n = chunks * CHUNK
    bufs = [synth.make_iq_torch(n, n_bursts=bursts, seed=synth.SEED_DEFAULT + k, device="cuda") for k in range(3)]
    if u8:
        bufs = [((b.to(torch.int32) >> 8) + 128).to(torch.uint8).contiguous() for b in bufs]
    torch.cuda.synchronize()
    with Context(0, chunks) as ctx:
        ctx.set_profiling(profiling)
        ctx.set_carry_over(carry)
        ctx.icao_flush()
        sub = ctx.submit_iq_device_u8 if u8 else ctx.submit_iq_device
        frames = pipelined(ctx, lambda i: sub(bufs[i % 3].data_ptr(), n), passes, flush_each=flush_each)
        report(f"resident {chunks} x {passes}, {bursts} bursts, flush {flush_each}, profiling {profiling}, u8 {u8}, carry {carry}", ctx, frames)


def ring(chunks, passes, profiling=1):
    n = chunks * CHUNK
    iq = [synth.make_iq(n, n_bursts=max(1, chunks // 8), seed=synth.SEED_DEFAULT + k) for k in range(2)]
    with Context(0, chunks) as ctx:
        ctx.ring_create(n)
        ctx.set_profiling(profiling)
        ctx.icao_flush()

        def submit(i):
            ctx.ring_acquire()[:] = iq[i % 2]
            ctx.ring_submit(n)
        report(f"ring {chunks} x {passes}, profiling {profiling}", ctx, pipelined(ctx, submit, passes))


def host_calls():
    iq = synth.make_iq(6 * CHUNK, n_bursts=30, seed=5150)
    iq[4 * CHUNK:5 * CHUNK, 0] = np.tile(np.array(PERIOD, dtype=np.int16), CHUNK // 8)   # periodic from end to end
    iq[4 * CHUNK:5 * CHUNK, 1] = 0
    for chunks, carry in ((8, False), (1, False), (1, True)):
        with Context(0, chunks) as ctx:
            ctx.set_carry_over(carry)
            ctx.icao_flush()
            report(f"adversarial host stream, context of {chunks}, carry {carry}", ctx, len(ctx.demod_iq(iq, cap=CAP)))
    with Context(0, 1) as ctx:
        frames = 0
        for k in (4, 0):   # the caller's own MagnitudeBuffer: one that overflows the fast scan's lists and a plain one
            mag = ctx.to_mag(iq[k * CHUNK:(k + 1) * CHUNK])
            mb = MagnitudeBuffer()
            mb.data[:] = mag.data
            mb.length = mag.length
            ctx.icao_flush()
            frames += len(ctx.demodulate2400(mb, cap=1 << 18))
        report("caller-supplied MagnitudeBuffer", ctx, frames)


if __name__ == "__main__":
    for flush_each in (False, True):
        resident(1, 2000, 1, flush_each)
    ring(1, 2000)
    ring(4, 2000)
    ring(1, 500, profiling=2)
    resident(1, 500, 1, True, profiling=2)
    for bursts in (64, 5000):
        resident(512, 16, bursts, True)
    resident(32, 24, 400, False, carry=True)
    resident(1, 500, 1, False, u8=True)
    resident(32, 24, 400, True, u8=True)
    host_calls()

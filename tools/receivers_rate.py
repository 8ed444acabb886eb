"""What "many receivers, one pass" (adsb_set_receivers, include/adsb_hip.h) buys and costs, measured on the box it runs on.

    python tools/receivers_rate.py [--out DIR] [--label TEXT] [--only SHAPE] [--steps K] [--parent-tree DIR]

Without --only this is a driver: every shape runs in a process of its own under its own `timeout`, one after the other,
and the chain stops at the first one that fails.  One JSON line per result goes to stdout and, with --out, is appended
to DIR/receivers_rate.jsonl.

Shapes:
  batch_sparse / batch_dense
            512 receivers, one 131072-sample buffer each per pass, resident IQ (bench.py's headline input: 64 bursts
            per 512 buffers; dense: 5000).  One context of 512 buffers with 512 receivers, four passes in flight,
            against the only route without the feature: 512 contexts of one buffer each, round-robin submit / collect,
            each kept as full as it allows (eight in flight).  ms per pass (512 buffers) and Gsample/s for both, and
            their ratio.  Both routes are driven from Python through ctypes: the per-call overhead of the binding is
            part of the 512-context figure (1024 calls per pass against 2).
  union_64 / union_512
            what the union superset costs: n_records of the batch pass minus the sum of n_records of the same buffers
            run per receiver (a context of the same size, flushed between receivers), with every receiver's filter
            taught first -- the false superset hits.  Receivers that share all aircraft (one pool: a reply of an
            aircraft this receiver has not heard but another has) and that share none.
  replay_dense / replay_fill
            the host replay of one pass, one walk over the records against the receivers dealt to the pool's threads:
            the host clock around adsb_collect of a pass whose kernels have all finished (the device is synchronised
            first), so that the time is checksum + replay.  5000-burst input with 512 receivers; formats_support.
            fill_capture (thousands of new aircraft) with 16.
  off       no cost when off: `python bench.py` in --parent-tree (a checkout of the parent commit with its library
            built) and in this tree, back to back, three times alternating; headline ms_per_step and kernel_avg_ms of
            each, and whether this build's median lies inside the spread of the parent's own ms_per_step_blocks.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CHUNK = 131072
SHAPES = {"batch_sparse": 420, "batch_dense": 420, "union_64": 300, "union_512": 420, "replay_dense": 300, "replay_fill": 300,
          "off": 900}


def emit(args, rec):
    rec = dict(rec, label=args.label, lib=version())
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        Path(args.out).mkdir(parents=True, exist_ok=True)
        with open(Path(args.out) / "receivers_rate.jsonl", "a") as f:
            f.write(line + "\n")


def version():
    from dump1090_rs_amd import _lib
    return _lib.lib().adsb_version().decode()


def keys(msgs):
    return [(int(m.chunk), int(m.j), int(m.try_phase), int(m.score), m.buffer(), float(m.signal_level)) for m in msgs]


# ------------------------------------------------------------------------------------------------- 1. the batch
def batch(args, n_bursts):
    import ctypes as C
    import numpy as np
    import torch
    from dump1090_rs_amd import Context, synth
    from dump1090_rs_amd._lib import AdsbMsg
    R, n = 512, 512 * CHUNK
    bufs = [synth.make_iq_torch(n, n_bursts=n_bursts, seed=synth.SEED_DEFAULT + b, device="cuda") for b in range(4)]
    torch.cuda.synchronize()
    cap = 1 << 16
    out, cnt = (AdsbMsg * cap)(), C.c_size_t()
    m = np.arange(R, dtype=np.uint32)
    steps = args.steps
    res = {}
    # one context, 512 receivers, four passes in flight
    with Context(0, R) as c:
        c.set_receivers(R)
        L, h = c._L, c._h
        frames = 0
        for phase, k_steps in (("warm", 8), ("timed", steps)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(k_steps):
                if c.pending() == 4:
                    assert L.adsb_collect(h, out, cap, C.byref(cnt)) == 0
                    frames += cnt.value
                assert L.adsb_submit_iq_device_rx(h, C.c_void_p(bufs[s % 4].data_ptr()), n, m.ctypes.data) == 0
            while c.pending():
                assert L.adsb_collect(h, out, cap, C.byref(cnt)) == 0
                frames += cnt.value
            dt = time.perf_counter() - t0
        res["one_context"] = {"ms_per_pass": 1e3 * dt / steps, "gsample_per_s": steps * n / dt / 1e9, "frames": frames,
                              "host_replays": int(L.adsb_host_replays(h)), "pooled_passes": c.selftest_rx_counters()["pooled_passes"]}
    # 512 contexts of one buffer, round-robin, eight in flight each
    ctxs = [Context(0, 1) for _ in range(R)]
    try:
        L = ctxs[0]._L
        hs = [c._h for c in ctxs]
        ptrs = [[C.c_void_p(b.data_ptr() + 4 * r * CHUNK) for r in range(R)] for b in bufs]
        pend = [0] * R
        frames = 0
        few = max(8, steps // 8)   # (1024 calls a pass: fewer passes say the same)
        for phase, k_steps in (("warm", 8), ("timed", few)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(k_steps):
                row = ptrs[s % 4]
                for r in range(R):
                    if pend[r] == 8:
                        assert L.adsb_collect(hs[r], out, cap, C.byref(cnt)) == 0
                        frames += cnt.value
                        pend[r] -= 1
                    assert L.adsb_submit_iq_device(hs[r], row[r], CHUNK) == 0
                    pend[r] += 1
            for r in range(R):
                while pend[r]:
                    assert L.adsb_collect(hs[r], out, cap, C.byref(cnt)) == 0
                    frames += cnt.value
                    pend[r] -= 1
            dt = time.perf_counter() - t0
        res["contexts_512"] = {"ms_per_pass": 1e3 * dt / few, "gsample_per_s": few * n / dt / 1e9, "frames": frames, "passes": few}
    finally:
        for c in ctxs:
            c.close()
    res["ratio"] = res["contexts_512"]["ms_per_pass"] / res["one_context"]["ms_per_pass"]
    emit(args, {"shape": "batch", "n_bursts_per_512": n_bursts, "receivers": R, "steps": steps, **res})


# ------------------------------------------------------------------------------------------------- 2. the union
def union_input(R, shared, seed):
    """One buffer per receiver: DF17s of eight aircraft and address/parity replies of eight more, all out of one pool of
    64 (`shared`) or out of a pool of the receiver's own."""
    import numpy as np
    from dump1090_rs_amd import synth
    from tests import formats_support as F
    rng = np.random.default_rng([0x0410, seed, R])
    common = [0x400000 + int(v) for v in rng.choice(1 << 20, size=64, replace=False)]
    iq = synth.noise_numpy(R * CHUNK, seed=0xA660 + seed)
    bursts = []
    for r in range(R):
        pool = common if shared else [0x800000 + 64 * r + k for k in range(64)]
        pick = rng.permutation(64)
        slot = CHUNK // 17
        for q in range(16):
            a = pool[int(pick[q])]
            f = synth.df17_frame(a, int(rng.integers(0, 1 << 56))) if q < 8 else F.ap_frame(int(rng.choice([4, 5, 20, 21])), a, int(rng.integers(0, 1 << 60)))
            s = r * CHUNK + 400 + q * slot + int(rng.integers(0, slot - 400))
            bursts.append(synth.Burst(5 * s + q % 5, 22000 + 300 * (q % 7), q % 16, f))
    synth.add_bursts(iq, bursts)
    return iq


def union(args, R):
    import numpy as np
    import torch
    from dump1090_rs_amd import Context
    m = np.arange(R, dtype=np.uint32)
    for shared in (True, False):
        iq = union_input(R, shared, 1)
        d = torch.from_numpy(iq).cuda()
        torch.cuda.synchronize()
        with Context(0, R) as c:
            per_records, per_msgs = 0, []
            for r in range(R):
                c.icao_flush()
                c.demod_iq_device(d.data_ptr() + 4 * r * CHUNK, CHUNK)            # (teaches the filter)
                got = c.demod_iq_device(d.data_ptr() + 4 * r * CHUNK, CHUNK)
                per_records += c.stats()["n_records"]
                per_msgs += [(r,) + k[1:] for k in keys(got)]
            c.set_receivers(R)
            c.demod_iq_device_rx(d.data_ptr(), R * CHUNK, m, cap=1 << 18)
            got = keys(c.demod_iq_device_rx(d.data_ptr(), R * CHUNK, m, cap=1 << 18))
            batch_records = c.stats()["n_records"]
            assert got == per_msgs, "the batch pass and the per-receiver passes differ"
        emit(args, {"shape": "union", "receivers": R, "aircraft": "shared by all" if shared else "shared by none",
                    "records_batch": batch_records, "records_per_receiver_sum": per_records, "false_superset_hits": batch_records - per_records,
                    "messages": len(got), "false_hits_per_buffer": (batch_records - per_records) / R})


# ------------------------------------------------------------------------------------------------- 3. the host replay
def replay(args, which):
    import zlib
    import numpy as np
    import torch
    from dump1090_rs_amd import Context, synth
    from dump1090_rs_amd._lib import AdsbMsg
    if which == "dense":
        R, n_buf = 512, 512
        d = synth.make_iq_torch(n_buf * CHUNK, n_bursts=5000, seed=synth.SEED_DEFAULT + 5, device="cuda")
    else:
        from tests import formats_support as F
        R, n_buf = 16, 64
        d = torch.from_numpy(F.fill_capture(77, n_buf, per_buffer=80)).cuda()
    torch.cuda.synchronize()
    m = (np.arange(n_buf) % R).astype(np.uint32)
    res = {}
    cap = 1 << 18
    out = (AdsbMsg * cap)()
    with Context(0, n_buf) as c:
        c.set_receivers(R)
        lists = {}
        for name, threshold in (("one_walk", 1 << 30), ("pooled", 1), ("one_walk_again", 1 << 30), ("pooled_again", 1)):
            c.selftest_rx_tune(threshold)
            times = []
            for rep in range(args.steps // 4 + 5):
                c.icao_flush()
                c.submit_iq_device_rx(d.data_ptr(), n_buf * CHUNK, m)
                torch.cuda.synchronize()      # every kernel of the pass has finished: what is left is the host's
                t0 = time.perf_counter()
                got = c.collect_raw(out, cap)
                times.append(time.perf_counter() - t0)
                lists.setdefault(name, (got, zlib.crc32(memoryview(out).cast("B")[: 40 * got])))
            res[name] = {"us_median": 1e6 * statistics.median(times[3:]), "us_min": 1e6 * min(times[3:]), "us_max": 1e6 * max(times[3:])}
        assert len(set(lists.values())) == 1, lists
        st = c.stats()
        emit(args, {"shape": "replay", "input": which, "receivers": R, "buffers": n_buf, "records": st["n_records"], "messages": st["n_messages"],
                    "clock": "host clock around adsb_collect, device synchronised first", "pool_threads": "up to 6 + the caller",
                    "pooled_passes": c.selftest_rx_counters()["pooled_passes"], **res})


# ------------------------------------------------------------------------------------------------- 4. off means off
def off(args):
    if not args.parent_tree or not (Path(args.parent_tree) / "bench.py").exists():
        print("off: needs --parent-tree (a checkout of the parent commit with its library built)", file=sys.stderr)
        return 2
    runs = {"parent": [], "this": []}
    for rep in range(3):
        for name, tree in (("parent", Path(args.parent_tree)), ("this", ROOT)):
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "bench.py", "--gpus", "1", "--no-cpu-baseline", "--no-also"],
                               cwd=str(tree), capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stderr[-2000:], file=sys.stderr)
                return 1
            d = json.loads(r.stdout.strip().splitlines()[-1])
            runs[name].append({"ms_per_step": d["ms_per_step"], "blocks": d.get("ms_per_step_blocks"), "kernel_avg_ms": d["roofline"]["kernel_avg_ms"]})
    med = {k: statistics.median(x["ms_per_step"] for x in v) for k, v in runs.items()}
    lo = min(min(x["blocks"]["all"]) for x in runs["parent"] if x["blocks"])
    hi = max(max(x["blocks"]["all"]) for x in runs["parent"] if x["blocks"])
    emit(args, {"shape": "off", "runs": runs, "median_ms_per_step": med, "parent_block_spread": [lo, hi],
                "inside_parent_spread": lo <= med["this"] <= hi})
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--label", default="")
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--parent-tree")
    args = ap.parse_args()
    if not args.only:
        for shape, limit in SHAPES.items():
            if shape == "off" and not args.parent_tree:
                continue
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, __file__, "--only", shape, "--steps", str(args.steps), "--label", args.label]
            cmd += (["--out", args.out] if args.out else []) + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
            rc = subprocess.run(cmd).returncode
            if rc != 0:      # (a step that failed, hung or faulted: nothing more is started on the device)
                print(f"{shape}: exit status {rc}; stopping", file=sys.stderr)
                return rc
        return 0
    if args.only.startswith("batch"):
        batch(args, 64 if args.only == "batch_sparse" else 5000)
    elif args.only.startswith("union"):
        union(args, int(args.only.split("_")[1]))
    elif args.only.startswith("replay"):
        replay(args, args.only.split("_")[1])
    else:
        return off(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())

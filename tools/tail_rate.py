"""What a change to the tail of a pass (match, records) does to the step: the parent commit's library against this
build's, both loaded into one process through the bare C ABI, alternating block by block on the same samples; every
collected step compared with the CPU oracle's demodulation of its buffer.

    python tools/tail_rate.py --parent-lib PATH [--lib NAME=PATH ...] [--rounds 7] [--out DIR] [--label TEXT]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/tail_rate.py --kernel-only PATH|this

Without --round-child this is a driver: R rounds, each a process of its own under its own `timeout`, one after the other
(the chain stops at the first that fails), then one summary line per library.  Legs of a round (bench.py's shapes):
  sparse    bench.py's headline: icao_flush + one pass over 512 resident buffers (64 bursts), four in flight, three
            buffers rotated over, the scan stamped by its own launch (profiling level 1), a clock ramp first; blocks of 20
            steps between device fences.  ms_per_step = the first block, ms_per_step_median = the median interval between
            its collects, ms_per_step_blocks = the five blocks behind it -- the libraries take turns block by block;
  dense     the same on 5000 bursts per 512 buffers (`also.config5_dense`: device-ordered, device-scored passes);
  unordered blocking passes over the 5000-burst buffer in a context that is in sparse mode when they are submitted (a
            sparse pass between them switches it back): the host-ordered tail at 17 000 hits, ms per pass.
  alone     blocking sparse passes (bench.py --sync's shape): a scan launch on its own, timed by the launch's own events
            (adsb_stats.ms_scan); kernel_avg_ms = the mean over a block of 20, the libraries taking turns block by block.
The summary: per library and leg the median over the rounds and their min-max; for every library but the parent the fall
of its median against the parent's and whether that clears the parent's own min-max spread over its rounds
(`clears_parent_spread`).  Lines go to stdout and, with --out, are appended to DIR/tail_rate.jsonl.
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
PER_BLOCK, BLOCKS, DEPTH = 20, 6, 4


def oracle_frames(iq):
    from oracle import binding
    want, _ = binding.Oracle().demod_iq(iq, cap=1 << 20, threads=16)
    return [(w["buffer"], int(w["score"]), int(w["j"]), int(w["try_phase"]), int(w["chunk"]), float(w["signal_level"])) for w in want]


def got_frames(m, n):
    return [(bytes(m[i].msg[: m[i].len]), int(m[i].score), int(m[i].j), int(m[i].try_phase), int(m[i].chunk), float(m[i].signal_level))
            for i in range(n)]


def load(path):
    import ctypes as C
    from dump1090_rs_amd import _lib
    L = _lib.lib() if path is None else C.CDLL(str(path))
    L.adsb_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_size_t]
    L.adsb_submit_iq_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.adsb_demod_iq_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.adsb_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.adsb_icao_flush.argtypes = [C.c_void_p]
    L.adsb_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.adsb_destroy.argtypes = [C.c_void_p]
    L.adsb_destroy.restype = None
    L.adsb_version.restype = C.c_char_p
    L.adsb_get_stats.argtypes = [C.c_void_p, C.c_void_p]
    return L


def pipelined(torch, libs, n_bursts, settle):
    """The pipelined step on every library in turn, block by block.  `settle`: untimed steps first (a dense stream's
    switch to device-side ordering belongs to the warm-up)."""
    import ctypes as C
    from dump1090_rs_amd import synth
    from dump1090_rs_amd._lib import AdsbMsg
    n = 512 * CHUNK
    bufs = [synth.make_iq_torch(n, n_bursts=n_bursts, seed=synth.SEED_DEFAULT + b, device="cuda") for b in range(3)]
    want = [oracle_frames(b.cpu().numpy()) for b in bufs]
    torch.cuda.synchronize()
    cap = 1 << 16
    outs = [(AdsbMsg * cap)() for _ in range(PER_BLOCK)]
    counts = [C.c_size_t() for _ in range(PER_BLOCK)]
    ctx = {}
    for name, L in libs.items():
        h = C.c_void_p()
        assert L.adsb_create(C.byref(h), 0, 512) == 0
        assert L.adsb_set_profiling(h, 1) == 0
        ctx[name] = h

    def block(name, first):
        L, h = libs[name], ctx[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done, stamps = 0, []
        for k in range(PER_BLOCK):
            assert L.adsb_icao_flush(h) == 0
            assert L.adsb_submit_iq_device(h, C.c_void_p(bufs[(first + k) % 3].data_ptr()), n) == 0
            if k >= DEPTH - 1:
                assert L.adsb_collect(h, outs[done], cap, C.byref(counts[done])) == 0
                stamps.append(time.perf_counter())
                done += 1
        while done < PER_BLOCK:
            assert L.adsb_collect(h, outs[done], cap, C.byref(counts[done])) == 0
            stamps.append(time.perf_counter())
            done += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        good = all(got_frames(outs[k], counts[k].value) == want[(first + k) % 3] for k in range(PER_BLOCK))
        return dt / PER_BLOCK * 1e3, statistics.median(b - a for a, b in zip(stamps, stamps[1:])) * 1e3, good

    ok = {k: True for k in libs}
    for name in libs:   # settle, then the clock ramp: untimed blocks until 120 ms have gone by
        for _ in range(settle):
            ok[name] = block(name, 0)[2] and ok[name]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.12:
            for k in range(PER_BLOCK):
                assert libs[name].adsb_icao_flush(ctx[name]) == 0
                assert libs[name].adsb_submit_iq_device(ctx[name], C.c_void_p(bufs[k % 3].data_ptr()), n) == 0
                assert libs[name].adsb_collect(ctx[name], outs[0], cap, C.byref(counts[0])) == 0
    t = {k: [] for k in libs}
    med = {}
    for b in range(BLOCKS):
        for name in libs:
            ms, iv, good = block(name, b * PER_BLOCK)
            ok[name] = ok[name] and good
            t[name].append(ms)
            med.setdefault(name, iv)
    for name, L in libs.items():
        L.adsb_destroy(ctx[name])
    return {name: {"ms_per_step": round(t[name][0], 4), "ms_per_step_median": round(med[name], 4),
                   "ms_per_step_blocks": [round(x, 4) for x in t[name][1:]], "parity": ok[name]} for name in libs}


def unordered(torch, libs, passes=8):
    import ctypes as C
    from dump1090_rs_amd import synth
    from dump1090_rs_amd._lib import AdsbMsg
    n = 512 * CHUNK
    dense = synth.make_iq_torch(n, n_bursts=5000, seed=synth.SEED_DEFAULT, device="cuda")
    sparse = synth.make_iq_torch(n, n_bursts=64, seed=synth.SEED_DEFAULT, device="cuda")
    want = oracle_frames(dense.cpu().numpy())
    torch.cuda.synchronize()
    cap = 1 << 16
    out, cnt = (AdsbMsg * cap)(), C.c_size_t()
    res = {}
    t, ok, ctx = {k: [] for k in libs}, {k: True for k in libs}, {}
    for name, L in libs.items():
        h = C.c_void_p()
        assert L.adsb_create(C.byref(h), 0, 512) == 0
        ctx[name] = h
    for i in range(passes + 1):
        for name, L in libs.items():
            h = ctx[name]
            assert L.adsb_icao_flush(h) == 0   # (a sparse pass: the context is in sparse mode for the pass behind it)
            assert L.adsb_demod_iq_device(h, C.c_void_p(sparse.data_ptr()), n, out, cap, C.byref(cnt)) == 0
            assert L.adsb_icao_flush(h) == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert L.adsb_demod_iq_device(h, C.c_void_p(dense.data_ptr()), n, out, cap, C.byref(cnt)) == 0
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                t[name].append(dt)
            ok[name] = ok[name] and got_frames(out, cnt.value) == want
    for name, L in libs.items():
        L.adsb_destroy(ctx[name])
        res[name] = {"ms_per_pass": round(statistics.median(t[name]), 4), "spread": [round(min(t[name]), 4), round(max(t[name]), 4)],
                     "parity": ok[name]}
    return res


def alone(torch, libs, blocks=4):
    """Blocking sparse passes, a launch on its own: per library the scan's duration by its own launch's events."""
    import ctypes as C
    from dump1090_rs_amd import synth
    from dump1090_rs_amd._lib import AdsbMsg, AdsbStats
    n = 512 * CHUNK
    bufs = [synth.make_iq_torch(n, n_bursts=64, seed=synth.SEED_DEFAULT + b, device="cuda") for b in range(3)]
    want = [oracle_frames(b.cpu().numpy()) for b in bufs]
    torch.cuda.synchronize()
    cap = 1 << 16
    out, cnt, st = (AdsbMsg * cap)(), C.c_size_t(), AdsbStats()
    ctx, t, ok = {}, {k: [] for k in libs}, {k: True for k in libs}
    for name, L in libs.items():
        h = C.c_void_p()
        assert L.adsb_create(C.byref(h), 0, 512) == 0 and L.adsb_set_profiling(h, 1) == 0
        ctx[name] = h
    for b in range(blocks + 1):   # (the first block of each library: warm-up and clock ramp, not counted)
        for name, L in libs.items():
            ms = []
            for k in range(PER_BLOCK):
                assert L.adsb_icao_flush(ctx[name]) == 0
                assert L.adsb_demod_iq_device(ctx[name], C.c_void_p(bufs[k % 3].data_ptr()), n, out, cap, C.byref(cnt)) == 0
                assert L.adsb_get_stats(ctx[name], C.byref(st)) == 0
                ms.append(float(st.ms_scan))
                ok[name] = ok[name] and got_frames(out, cnt.value) == want[k % 3]
            if b:
                t[name].append(statistics.mean(ms))
    for name, L in libs.items():
        L.adsb_destroy(ctx[name])
    return {name: {"kernel_avg_ms": round(statistics.mean(t[name]), 5), "kernel_avg_ms_blocks": [round(x, 5) for x in t[name]],
                   "parity": ok[name]} for name in libs}


def kernel_only(path):
    """12 pipelined blocks of 20 sparse steps, then 30 blocking passes, on one library, unchecked: the run to put under
    `rocprofv3 --kernel-trace` for tools/tail_trace.py (the tail kernels beside a scan, and alone)."""
    import ctypes as C
    import torch
    from dump1090_rs_amd import synth
    from dump1090_rs_amd._lib import AdsbMsg
    L = load(None if path == "this" else path)
    n = 512 * CHUNK
    bufs = [synth.make_iq_torch(n, n_bursts=64, seed=synth.SEED_DEFAULT + b, device="cuda") for b in range(3)]
    torch.cuda.synchronize()
    h = C.c_void_p()
    assert L.adsb_create(C.byref(h), 0, 512) == 0 and L.adsb_set_profiling(h, 1) == 0
    cap = 1 << 16
    out, cnt = (AdsbMsg * cap)(), C.c_size_t()
    for _ in range(12):
        torch.cuda.synchronize()
        done = 0
        for k in range(PER_BLOCK):
            if k >= DEPTH:
                assert L.adsb_collect(h, out, cap, C.byref(cnt)) == 0
                done += 1
            assert L.adsb_icao_flush(h) == 0 and L.adsb_submit_iq_device(h, C.c_void_p(bufs[k % 3].data_ptr()), n) == 0
        while done < PER_BLOCK:
            assert L.adsb_collect(h, out, cap, C.byref(cnt)) == 0
            done += 1
    torch.cuda.synchronize()
    for k in range(30):
        assert L.adsb_icao_flush(h) == 0
        assert L.adsb_demod_iq_device(h, C.c_void_p(bufs[k % 3].data_ptr()), n, out, cap, C.byref(cnt)) == 0
    L.adsb_destroy(h)
    print("ok", L.adsb_version().decode())
    return 0


def round_child(a, libs_spec):
    import torch
    libs = {name: load(path) for name, path in libs_spec}
    ver = {name: L.adsb_version().decode() for name, L in libs.items()}
    lines = []
    legs = [("sparse", lambda: pipelined(torch, libs, 64, 0)), ("dense", lambda: pipelined(torch, libs, 5000, 2)),
            ("unordered", lambda: unordered(torch, libs)), ("alone", lambda: alone(torch, libs))]
    for leg, run in legs:
        if a.only and leg != a.only:
            continue
        res = run()
        for name in libs:
            lines.append({"leg": leg, "library": name, "version": ver[name], "round": a.round_child, **res[name]})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    return 0 if all(ln["parity"] for ln in lines) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libadsb_hip.so, built on this box")
    ap.add_argument("--kernel-only", default=None, metavar="PATH|this", help="pipelined and blocking sparse passes on one library, for a kernel trace")
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="a further build to take turns with the two")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None)
    ap.add_argument("--only", default=None, help="one leg: sparse, dense, unordered, alone")
    ap.add_argument("--round-child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernel_only:
        return kernel_only(a.kernel_only)
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    spec = [("parent", a.parent_lib), ("this", None)] + [tuple(s.split("=", 1)) for s in a.lib]
    if a.round_child is not None:
        return round_child(a, spec)
    lines = []
    for r in range(a.rounds):
        cmd = ["timeout", "-k", "10", "240", sys.executable, str(Path(__file__).resolve()), "--parent-lib", a.parent_lib,
               "--round-child", str(r)] + [x for s in a.lib for x in ("--lib", s)] + (["--only", a.only] if a.only else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        got = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
        lines += got
        for ln in got:
            print(json.dumps(ln), flush=True)
        if p.returncode != 0:
            print(json.dumps({"error": "round %d ended with status %d" % (r, p.returncode)}), flush=True)
            return 1   # (nothing more is started on the device behind a failed round)
    summary = []
    for leg in ("sparse", "dense", "unordered", "alone"):
        fig = {"unordered": "ms_per_pass", "alone": "kernel_avg_ms"}.get(leg, "ms_per_step")
        per = {}
        for ln in lines:
            if ln["leg"] == leg:
                per.setdefault(ln["library"], []).append(ln)
        if "parent" not in per:
            continue
        pv = [ln[fig] for ln in per["parent"]]
        for name, rows in per.items():
            v = [ln[fig] for ln in rows]
            s = {"summary": leg, "library": name, "version": rows[0]["version"], "rounds": len(v), fig: statistics.median(v),
                 "spread": [min(v), max(v)], "parity": all(ln["parity"] for ln in rows)}
            if leg in ("sparse", "dense"):
                s["ms_per_step_median"] = statistics.median(ln["ms_per_step_median"] for ln in rows)
                s["ms_per_step_blocks_median"] = statistics.median(x for ln in rows for x in ln["ms_per_step_blocks"])
            if name != "parent":
                fall = statistics.median(pv) - statistics.median(v)
                s["fall_vs_parent_ms"] = round(fall, 5)
                s["fall_vs_parent_pct"] = round(100.0 * fall / statistics.median(pv), 2)
                s["parent_spread_ms"] = round(max(pv) - min(pv), 5)
                s["clears_parent_spread"] = fall > max(pv) - min(pv)
            summary.append(s)
    if a.label:
        lines = [{**ln, "build": a.label} for ln in lines]
        summary = [{**ln, "build": a.label} for ln in summary]
    for ln in summary:
        print(json.dumps(ln), flush=True)
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "tail_rate.jsonl", "a") as f:
            for ln in lines + summary:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

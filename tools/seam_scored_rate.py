"""What receiver seams scored on the device (include/adsb_hip.h, "Receiver seams, scored on the device") cost and gain, and
that the single modes and a context with both off cost what the parent commit's did.

    python tools/seam_scored_rate.py [--parent-lib PATH] [--out DIR] [--blocks 5] [--per-block 4] [--label TEXT]

tools/seam_rate.py's protocol and input: passes of 512 buffers (a context of 512, four in flight, 8 passes a run) with 512
receivers and with 8, round robin, resident CS16, on a sparse sky (8 frames a buffer) and a busy one (120 a buffer); pass p
gives buffer b of the pass buffer (p + b) % 8 of one continuous stream.  With 512 receivers each hears that stream one buffer a
pass and its seams are real; with 8 receivers, receiver r's 64 buffers of a pass are 64 copies of one buffer of the stream:
only the seam from its last buffer of a pass to its first of the next continues the stream, the 63 seams inside the pass
join a buffer's end to its own start (the seam kernels do the same work, the frames found across them are not a live
stream's).  One process; a run is a pipelined
loop of submit / collect with the pipeline full, timed by the host clock from its first submit to its last collect;
variants in interleaved blocks of --per-block runs after one untimed block:
  neither, carry, scoring, both     this build, receivers on: both modes off, adsb_set_receiver_carry alone (today's
                host-scored seam pass), adsb_set_receiver_scoring alone, adsb_set_receiver_carry_scoring
  parent_neither, parent_carry, parent_scoring and each again as *_again   (--parent-lib: the parent commit's
                libadsb_hip.so loaded beside this one) two contexts of the parent's library per single mode
(a) both / carry: what scoring the seam pass on the device gains.  (b) both / scoring: what seams cost on the scored path.
(c) neither, carry and scoring over the parent's, each with the spread of the parent's own two contexts beside it; a ratio
outside that spread is named as such ("outside_parent_spread").  Per variant the step, the host CPU per pass (process time
of the loop) and the counters that say who scored: passes taken from the device / refused, host replays, merged passes,
seam records merged, passes that declared themselves unscored.
The merge kernels' own device time comes from a kernel trace of one variant's loop alone:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/seam_scored_rate.py --profile 512,busy,both
    python tools/seam_scored_rate.py --kernels DIR/.../t_kernel_stats.csv --kernels-of 512,busy,both --out DIR
One JSON line per (receivers, sky) goes to stdout and, with --out, is appended to DIR/seam_scored_rate.jsonl.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
CHUNK = 131072
N_BUFFERS, PASSES = 512, 8
RECEIVERS = [512, 8]
SKIES = [("sparse", 8), ("busy", 120)]
MODES = ("neither", "carry", "scoring", "both")


def bind(L):
    import seam_rate
    seam_rate.bind(L)
    vp = C.c_void_p
    L.adsb_set_receiver_carry.argtypes = [vp, C.c_int]
    L.adsb_set_receiver_scoring.argtypes = [vp, C.c_int]
    L.adsb_selftest_rx_score_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.adsb_host_replays.argtypes = [vp]
    L.adsb_host_replays.restype = C.c_uint64
    return L


class Loop:
    """A receivers context of `lib` in one of MODES and its pipelined submit / collect loop over one resident input."""

    def __init__(self, lib, n_receivers, mode, has_combined):
        from dump1090_rs_amd import _lib
        self.lib, self.ctx, self.mode, self.has_combined = lib, C.c_void_p(), mode, has_combined
        assert lib.adsb_create(C.byref(self.ctx), 0, N_BUFFERS) == 0
        assert lib.adsb_set_receivers(self.ctx, n_receivers) == 0
        if mode == "carry":
            assert lib.adsb_set_receiver_carry(self.ctx, 1) == 0
        elif mode == "scoring":
            assert lib.adsb_set_receiver_scoring(self.ctx, 1) == 0
        elif mode == "both":
            assert lib.adsb_set_receiver_carry_scoring(self.ctx, 1) == 0
        self.depth = lib.adsb_max_in_flight(self.ctx)
        self.out = (_lib.AdsbMsg * (1 << 18))()
        self.n_out = C.c_size_t()

    def run(self, ptr, n_samples, rx_map):
        lib, ctx = self.lib, self.ctx
        lib.adsb_icao_flush(ctx)
        pending = msgs = 0
        t0, c0 = time.perf_counter(), time.process_time()
        for k in range(PASSES):
            if pending == self.depth:
                assert lib.adsb_collect(ctx, self.out, len(self.out), C.byref(self.n_out)) == 0
                msgs += self.n_out.value
                pending -= 1
            assert lib.adsb_submit_iq_device_rx(ctx, ptr + (k % 8) * CHUNK * 4, n_samples, rx_map.ctypes.data) == 0
            pending += 1
        while pending:
            assert lib.adsb_collect(ctx, self.out, len(self.out), C.byref(self.n_out)) == 0
            msgs += self.n_out.value
            pending -= 1
        return (time.perf_counter() - t0) * 1e3 / PASSES, (time.process_time() - c0) * 1e3 / PASSES, msgs

    def counters(self):
        out = (C.c_uint64 * 4)()
        assert self.lib.adsb_selftest_rx_score_counters(self.ctx, out) == 0
        k = {"taken": int(out[0]), "refused": int(out[1]), "rebuilds": int(out[2]), "replays": int(self.lib.adsb_host_replays(self.ctx))}
        if self.has_combined:
            assert self.lib.adsb_selftest_rx_seam_score_counters(self.ctx, out) == 0
            k.update(merged_passes=int(out[0]), seam_records_merged=int(out[1]), dropped_on_device=int(out[2]), unscored=int(out[3]))
        return k

    def close(self):
        self.lib.adsb_destroy(self.ctx)


def case(np, torch, libs, n_receivers, sky, per_buffer, blocks, per_block):
    import seam_rate
    iq = seam_rate.make_input(torch, N_BUFFERS, per_buffer)
    rx_map = (np.arange(N_BUFFERS) % n_receivers).astype(np.uint32)
    # (contexts are created, and run within a block, in this order: the parent's two of a mode bracket this build's)
    loops = {}
    singles = ("neither", "carry", "scoring")
    for mode in singles:
        if "parent" in libs:
            loops["parent_" + mode] = Loop(libs["parent"], n_receivers, mode, False)
        loops[mode] = Loop(libs["this"], n_receivers, mode, True)
        if "parent" in libs:
            loops["parent_" + mode + "_again"] = Loop(libs["parent"], n_receivers, mode, False)
    loops["both"] = Loop(libs["this"], n_receivers, "both", True)
    step = {name: [] for name in loops}
    cpu = {name: [] for name in loops}
    msgs, before = {}, {}
    for b in range(blocks + 1):
        if b == 1:
            before = {name: loop.counters() for name, loop in loops.items()}
        for name, loop in loops.items():
            t, c = [], []
            for _ in range(per_block):
                ms, cms, n = loop.run(iq.data_ptr(), N_BUFFERS * CHUNK, rx_map)
                t.append(ms), c.append(cms)
                msgs[name] = n
            if b:
                step[name].append(t), cpu[name].append(c)
    after = {name: loop.counters() for name, loop in loops.items()}
    for loop in loops.values():
        loop.close()
    timed_passes = blocks * per_block * PASSES
    med = {name: statistics.median(v for blk in t for v in blk) for name, t in step.items()}
    spread = {name: [min(statistics.median(blk) for blk in t), max(statistics.median(blk) for blk in t)] for name, t in step.items()}
    line = {"shape": "seam_scored", "receivers": n_receivers, "buffers_per_pass": N_BUFFERS, "passes_per_run": PASSES, "sky": sky,
            "frames_per_buffer": per_buffer, "runs": blocks * per_block, "step_ms": med, "block_spread_ms": spread,
            "host_cpu_ms_per_pass": {name: statistics.median(v for blk in t for v in blk) for name, t in cpu.items()},
            "messages_per_run": msgs,
            "per_pass": {name: {k: (after[name][k] - before[name][k]) / timed_passes for k in after[name]} for name in loops},
            "both_over_carry": med["both"] / med["carry"], "both_over_scoring": med["both"] / med["scoring"],
            "parity_both_carry": msgs["both"] == msgs["carry"]}
    if "parent" in libs:
        for mode in singles:
            p, again = "parent_" + mode, "parent_" + mode + "_again"
            lo, hi = (f(spread[p][i], spread[again][i]) for i, f in ((0, min), (1, max)))
            line[mode + "_over_parent"] = med[mode] / med[p]
            line[mode + "_parent_again_over_parent"] = med[again] / med[p]
            line[mode + "_outside_parent_spread"] = not (lo <= med[mode] <= hi)
            line[mode + "_parity_parent"] = msgs[mode] == msgs[p]
    return line


def profiled(np, torch, lib, spec):
    """--profile R,sky,mode: that one variant's loop alone, 12 runs, for a kernel trace of it."""
    import seam_rate
    r, sky, mode = spec.split(",")
    iq = seam_rate.make_input(torch, N_BUFFERS, dict(SKIES)[sky])
    rx_map = (np.arange(N_BUFFERS) % int(r)).astype(np.uint32)
    loop = Loop(lib, int(r), mode, True)
    for _ in range(12):
        loop.run(iq.data_ptr(), N_BUFFERS * CHUNK, rx_map)
    loop.close()


def kernel_lines(csv_path, spec):
    """seam_rate.kernel_lines, with the merge kernels' share of all device time beside the seam kernels'"""
    import seam_rate
    line = seam_rate.kernel_lines(csv_path, spec)[0]
    total = sum(e["total_us"] for e in line["kernels"].values())
    merge = sum(e["total_us"] for name, e in line["kernels"].items() if name.startswith(("k_seam_mark", "k_seam_prefix", "k_seam_place")))
    line.update(shape="seam_scored_kernels", merge_share_of_device_time=merge / total if total else None)
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libadsb_hip.so, built on this machine")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4)
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    ap.add_argument("--profile", default=None, help="R,sky,mode (512,busy,both): that variant's loop alone, for a kernel trace")
    ap.add_argument("--kernels", default=None, help="a kernel-statistics CSV of a --profile run: its line (with --kernels-of R,sky,mode)")
    ap.add_argument("--kernels-of", default=None)
    a = ap.parse_args()
    import numpy as np
    lines = []
    if a.kernels:
        lines = kernel_lines(a.kernels, a.kernels_of)
        print(json.dumps(lines[0]), flush=True)
    else:
        import torch
        from dump1090_rs_amd import _lib
        this = _lib.lib()   # (bound by the package)
        if a.profile:
            profiled(np, torch, this, a.profile)
            return 0
        libs = {"this": this}
        if a.parent_lib:
            libs["parent"] = bind(C.CDLL(str(a.parent_lib)))
        for n_receivers in RECEIVERS:
            for sky, per_buffer in SKIES:
                line = case(np, torch, libs, n_receivers, sky, per_buffer, a.blocks, a.per_block)
                lines.append(line)
                print(json.dumps(line), flush=True)
                torch.cuda.empty_cache()
    if a.label:
        for line in lines:
            line["build"] = a.label
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "seam_scored_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

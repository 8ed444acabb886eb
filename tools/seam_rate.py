"""What receiver seams (include/adsb_hip.h, "Receiver seams") cost, and that a context with the mode off costs what the
parent commit's did.

    python tools/seam_rate.py [--parent-lib PATH] [--out DIR] [--blocks 5] [--per-block 4] [--label TEXT] [--no-gain]

Two shapes -- 512 receivers, passes of 512 buffers (a context of 512, four in flight, 8 passes a run) and 8 receivers,
passes of 8 buffers (a context of 8, eight in flight, 64 passes a run) -- round robin, resident CS16, on a sparse sky (8
frames a buffer) and a busy one (120 a buffer).  Eight distinct buffers of one continuous stream; pass p gives
receiver b buffer (p + b) % 8 of it, so each receiver hears that stream one buffer a pass and its seams are real.  One process; a run is a pipelined loop
of submit / collect with the pipeline full, timed from its first submit to its last collect; variants in interleaved
blocks of --per-block runs after one untimed block:
  off           this build, receivers on, the mode off
  on            ... the mode on: step time, host CPU per pass (process time of the loop), seam records per pass, records
                of the pass dropped, seam steps redone (the counters of adsb_selftest_rx_seam_counters)
  parent, parent_again   (--parent-lib: the parent commit's libadsb_hip.so loaded beside this one) two contexts of the
                parent's library, receivers on.  (a) off / parent, expected inside the spread of the parent's own two
                contexts, which the same run records.
  plain, plain_carry   this build, a plain context (no receivers) without and with adsb_set_carry_over: the control for
                the stream rule -- carry-over orders every pass on one scan stream, as the seam mode does, and launches
                none of the seam kernels.  on / off against plain_carry / plain separates that rule from the kernels.
The passes run on the library's own streams, so a step is host wall-clock over a full pipeline, not an event pair.  The
kernels' own device time comes from a kernel trace of one variant's loop alone:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/seam_rate.py --profile 512,sparse,on
    python tools/seam_rate.py --kernels DIR/.../t_kernel_stats.csv --kernels-of 512,sparse,on --out DIR
one line per variant: launches and mean microseconds of every kernel, and the seam kernels' share of all device time.
(c) the frames carry-over gains on the three reference captures cut into buffers at awkward places comes from the CPU
oracle alone and is a property of the input: one line per capture and cut.
One JSON line per (shape, sky) and per capture goes to stdout and, with --out, is appended to DIR/seam_rate.jsonl.
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
CHUNK = 131072
SHAPES = [(512, 512, 8), (8, 8, 64)]      # receivers, buffers per pass (= max_chunks), passes per run
SKIES = [("sparse", 8), ("busy", 120)]    # frames per buffer


def bind(L):
    vp, sz = C.c_void_p, C.c_size_t
    L.adsb_create.argtypes = [C.POINTER(vp), C.c_int, sz]
    L.adsb_destroy.argtypes = [vp]
    L.adsb_destroy.restype = None
    L.adsb_set_receivers.argtypes = [vp, C.c_uint32]
    L.adsb_submit_iq_device_rx.argtypes = [vp, vp, sz, vp]
    L.adsb_submit_iq_device.argtypes = [vp, vp, sz]
    L.adsb_set_carry_over.argtypes = [vp, C.c_int]
    L.adsb_collect.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.adsb_icao_flush.argtypes = [vp]
    L.adsb_max_in_flight.argtypes = [vp]
    return L


class Loop:
    """A receivers context of `lib` and its pipelined submit / collect loop over one resident pass-sized input."""

    def __init__(self, lib, n_receivers, n_buffers, seam, plain_carry=None):
        """plain_carry None: a receivers context; False / True: a plain context, adsb_set_carry_over off / on (the control
        for the stream rule: all passes on one scan stream, no seam kernels)."""
        from dump1090_rs_amd import _lib
        self.lib, self.ctx = lib, C.c_void_p()
        self.plain = plain_carry is not None
        assert lib.adsb_create(C.byref(self.ctx), 0, n_buffers) == 0
        if self.plain:
            assert lib.adsb_set_carry_over(self.ctx, 1 if plain_carry else 0) == 0
        else:
            assert lib.adsb_set_receivers(self.ctx, n_receivers) == 0
        if seam:
            assert lib.adsb_set_receiver_carry(self.ctx, 1) == 0
        self.depth = lib.adsb_max_in_flight(self.ctx)
        self.out = (_lib.AdsbMsg * (1 << 18))()
        self.n_out = C.c_size_t()
        self.seam = seam

    def run(self, ptr, n_samples, rx_map, passes):
        lib, ctx = self.lib, self.ctx
        lib.adsb_icao_flush(ctx)
        pending = msgs = 0
        t0, c0 = time.perf_counter(), time.process_time()
        for k in range(passes):
            if pending == self.depth:
                assert lib.adsb_collect(ctx, self.out, len(self.out), C.byref(self.n_out)) == 0
                msgs += self.n_out.value
                pending -= 1
            at = ptr + (k % 8) * CHUNK * 4
            assert (lib.adsb_submit_iq_device(ctx, at, n_samples) if self.plain else
                    lib.adsb_submit_iq_device_rx(ctx, at, n_samples, rx_map.ctypes.data)) == 0
            pending += 1
        while pending:
            assert lib.adsb_collect(ctx, self.out, len(self.out), C.byref(self.n_out)) == 0
            msgs += self.n_out.value
            pending -= 1
        return (time.perf_counter() - t0) * 1e3 / passes, (time.process_time() - c0) * 1e3 / passes, msgs

    def counters(self):
        out = (C.c_uint64 * 4)()
        if self.plain or not self.seam:
            return [0, 0, 0, 0]
        assert self.lib.adsb_selftest_rx_seam_counters(self.ctx, out) == 0
        return [int(v) for v in out]

    def close(self):
        self.lib.adsb_destroy(self.ctx)


def case(np, torch, libs, n_receivers, n_buffers, passes, sky, per_buffer, blocks, per_block):
    # (synth.plan_bursts keeps every burst inside its slot, and a buffer is a whole number of slots: the buffers are cut 777
    # samples into the stream instead, so that frames straddle their ends at the rate a live stream's would; buffer b of
    # pass p is buffer (p + b) % 8 of the block: every receiver hears the block as a continuous stream, one buffer a pass,
    # so frames that straddle the block's buffer ends are real seam frames, and neighbouring receivers hear different buffers)
    iq = make_input(torch, n_buffers, per_buffer)
    rx_map = (np.arange(n_buffers) % n_receivers).astype(np.uint32)
    # (contexts are created, and run within a block, in this order: the parent's two bracket this build's)
    loops = {}
    if "parent" in libs:
        loops["parent"] = Loop(libs["parent"], n_receivers, n_buffers, False)
    loops["off"] = Loop(libs["this"], n_receivers, n_buffers, False)
    loops["on"] = Loop(libs["this"], n_receivers, n_buffers, True)
    if "parent" in libs:
        loops["parent_again"] = Loop(libs["parent"], n_receivers, n_buffers, False)
    loops["plain"] = Loop(libs["this"], 0, n_buffers, False, plain_carry=False)
    loops["plain_carry"] = Loop(libs["this"], 0, n_buffers, False, plain_carry=True)
    step = {name: [] for name in loops}
    cpu = {name: [] for name in loops}
    msgs = {}
    before = loops["on"].counters()
    on_passes = 0
    for b in range(blocks + 1):
        for name, loop in loops.items():
            t, c = [], []
            for _ in range(per_block):
                ms, cms, n = loop.run(iq.data_ptr(), n_buffers * CHUNK, rx_map, passes)
                t.append(ms), c.append(cms)
                msgs[name] = n
                on_passes += passes if name == "on" else 0
            if b:
                step[name].append(t), cpu[name].append(c)
    after = loops["on"].counters()
    for loop in loops.values():
        loop.close()
    med = {name: statistics.median(v for blk in t for v in blk) for name, t in step.items()}
    spread = {name: [min(statistics.median(blk) for blk in t), max(statistics.median(blk) for blk in t)] for name, t in step.items()}
    line = {"shape": "seam", "receivers": n_receivers, "buffers_per_pass": n_buffers, "passes_per_run": passes, "sky": sky,
            "frames_per_buffer": per_buffer, "runs": blocks * per_block, "step_ms": med, "block_spread_ms": spread,
            "host_cpu_ms_per_pass": {name: statistics.median(v for blk in t for v in blk) for name, t in cpu.items()},
            "messages_per_run": msgs, "on_over_off": med["on"] / med["off"],
            "plain_carry_over_plain": med["plain_carry"] / med["plain"] if "plain_carry" in med and "plain" in med else None,
            "seam_records_per_pass": (after[1] - before[1]) / on_passes, "pass_records_dropped_per_pass": (after[2] - before[2]) / on_passes,
            "seam_steps_redone": after[3] - before[3]}
    if "parent" in med:
        line["off_over_parent"] = med["off"] / med["parent"]
        line["parent_again_over_parent"] = med["parent_again"] / med["parent"]
        lo, hi = (f(spread["parent"][i], spread["parent_again"][i]) for i, f in ((0, min), (1, max)))
        line["off_inside_parent_spread"] = lo <= med["off"] <= hi
        line["parity_off_parent"] = msgs["off"] == msgs["parent"]
    return line


def make_input(torch, n_buffers, per_buffer):
    from dump1090_rs_amd import synth
    block = synth.make_iq_torch(9 * CHUNK, 9 * per_buffer, seed=0x5EA0 + per_buffer, n_icao=60, df11_every=5, device="cuda")[777:777 + 8 * CHUNK]
    iq = block.repeat(n_buffers // 8 + 1, 1).contiguous()
    torch.cuda.synchronize()
    return iq


def profiled(np, torch, lib, spec):
    """--profile R,sky,variant: that one variant's loop alone, 12 runs, for a kernel trace of it (the kernels' own device
    time: rocprofv3 --kernel-trace --stats -- python tools/seam_rate.py --profile ...; --kernels reads the statistics)."""
    r, sky, variant = spec.split(",")
    n_receivers, n_buffers, passes = next(sh for sh in SHAPES if sh[0] == int(r))
    iq = make_input(torch, n_buffers, dict(SKIES)[sky])
    rx_map = (np.arange(n_buffers) % n_receivers).astype(np.uint32)
    loop = Loop(lib, n_receivers, n_buffers, variant == "on", plain_carry={"plain": False, "plain_carry": True}.get(variant))
    for _ in range(12):
        loop.run(iq.data_ptr(), n_buffers * CHUNK, rx_map, passes)
    loop.close()


def kernel_lines(csv_path, spec):
    """The device time of every kernel of one variant's loop from a kernel-statistics CSV (Name, Calls, TotalDurationNs,
    AverageNs, ...), one line: per kernel its launches and mean microseconds, the seam kernels' share of all device time."""
    import csv
    r, sky, variant = spec.split(",")
    per, total, seam = {}, 0.0, 0.0
    with open(csv_path) as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("adsb::", "").split("(")[0]
            if not name.startswith("k_"):
                continue
            e = per.setdefault(name, {"launches": 0, "total_us": 0.0})
            e["launches"] += int(row["Calls"])
            e["total_us"] += float(row["TotalDurationNs"]) / 1e3
    for name, e in per.items():
        e["mean_us"] = e["total_us"] / e["launches"]
        total += e["total_us"]
        seam += e["total_us"] if name.startswith(("k_rx_lead", "k_rx_carry_update", "k_seam_")) else 0.0
    return [{"shape": "seam_kernels", "receivers": int(r), "sky": sky, "variant": variant, "kernels": per,
             "seam_share_of_device_time": seam / total if total else None}]


def gains(np):
    """(c): per reference capture and per cut (primes: the captures hold five or six frames, a short buffer puts a cut
    through some of them), the frames the CPU oracle finds buffer by buffer with carry-over against without."""
    from oracle import binding
    binding.build()
    golden = json.loads((ROOT / "tests" / "golden" / "reference_frames.json").read_text())
    lines = []
    for fx in golden["fixtures"]:
        raw = np.fromfile(ROOT / "tests" / "golden" / fx["file"], dtype="<i2").reshape(-1, 2)
        iq = np.ascontiguousarray(raw[:, ::-1])
        whole = len(binding.Oracle().demod_iq(iq)[0])
        for cut in (1021, 2039, 4099, 9973):
            with_c, without = binding.Oracle(), binding.Oracle()
            carry = np.zeros((326, 2), dtype=np.int16)
            n_with = n_without = 0
            for a in range(0, len(iq), cut):
                part = np.ascontiguousarray(iq[a:a + cut])
                n_with += len(binding.demod_iq_carry(with_c, part, carry)[0])
                n_without += len(without.demod_iq(part)[0])
            lines.append({"shape": "seam_gain", "capture": fx["file"], "cut": cut, "frames_whole": whole, "frames_with_carry": n_with,
                          "frames_without": n_without, "gained": n_with - n_without})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libadsb_hip.so, built on this machine")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4)
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    ap.add_argument("--no-gain", action="store_true")
    ap.add_argument("--only-gain", action="store_true", help="(c) alone: needs no device")
    ap.add_argument("--profile", default=None, help="R,sky,variant (512,sparse,on): that variant's loop alone, for a kernel trace")
    ap.add_argument("--kernels", default=None, help="a kernel-statistics CSV of a --profile run: its line (with --kernels-of R,sky,variant)")
    ap.add_argument("--kernels-of", default=None)
    a = ap.parse_args()
    import numpy as np
    lines = []
    if a.profile:
        import torch
        from dump1090_rs_amd import _lib
        profiled(np, torch, _lib.lib(), a.profile)
        return 0
    if a.kernels:
        lines = kernel_lines(a.kernels, a.kernels_of)
        print(json.dumps(lines[0]), flush=True)
    elif not a.only_gain:
        import torch
        from dump1090_rs_amd import _lib
        libs = {"this": _lib.lib()}
        if a.parent_lib:
            libs["parent"] = bind(C.CDLL(str(a.parent_lib)))
        for n_receivers, n_buffers, passes in SHAPES:
            for sky, per_buffer in SKIES:
                line = case(np, torch, libs, n_receivers, n_buffers, passes, sky, per_buffer, a.blocks, a.per_block)
                lines.append(line)
                print(json.dumps(line), flush=True)
                torch.cuda.empty_cache()
    if not a.no_gain and not a.kernels:
        for line in gains(np):
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.label:
        for line in lines:
            line["build"] = a.label
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "seam_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

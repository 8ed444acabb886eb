"""What the resampler (adsb_resamp_run_device; include/adsb_hip.h, "Resampling") costs.

    python tools/resamp_rate.py [--out DIR] [--runs N] [--buffers B] [--ratios 6/5,24/25,2/5,6/25,3/25] [--label TEXT]

Per ratio L/M and input format (CS16, 8-bit), with the default taps (8 max(L, M) + 1 of them, shift 14):
  kernel   adsb_resamp_run_device over the input of B (default 512) output buffers, device memory to device memory,
           timed with HIP events on the stream the context orders its input behind; after 3 warm-up runs, N (default 20,
           at least 20) runs; the median, the spread, and the bytes moved per second -- (4 or 2) M / L read and 4 written
           per output -- beside the 6.29 TB/s an HBM copy reaches on an MI355X;
  step     icao_flush + run_device + adsb_submit_iq_device + adsb_collect per step against icao_flush + submit +
           collect on the same resampled samples, same process, same context, alternating in blocks of 10 steps; ms per step.
  versus   the yardstick: the resampler at L = 1, M = 2, 5, 10 against adsb_decim_run_device (k_decim) with the same taps
           (the decimator's defaults, shift 15), same process, same input, runs alternating; both outputs equal.
Every case first checks the head of its output against the numpy restatement (tests/resamp_support.py).
One JSON line per case goes to stdout and, with --out, is appended to DIR/resamp_rate.jsonl.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CHUNK = 131072
HBM_COPY_TBPS = 6.29
CS16, U8 = 0, 1


def t_soapy(np):
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


def inputs_for(n_out, L, M):
    return ((n_out - 1) * M) // L + 1


def make_input(torch, n_out, L, M, fmt):
    """The inputs of n_out outputs on the device: input m holds sample ceil(m L / M) of a synthetic 2.4 MS/s stream."""
    from dump1090_rs_amd import synth
    base = synth.make_iq_torch(n_out + 1, n_bursts=64, device="cuda")
    if fmt == U8:
        base = torch.clamp(torch.round(base.to(torch.float32) / 256.0 + 127.4), 0, 255).to(torch.uint8)
    m = torch.arange(inputs_for(n_out, L, M), device="cuda", dtype=torch.int64)
    x = base[(m * L + (M - 1)) // M].contiguous()
    del m
    torch.cuda.synchronize()
    return x


def head_ok(np, torch, x, y, taps, shift, L, M, fmt, n_check=4096):
    from tests import resamp_support as rs
    head = x[: inputs_for(n_check, L, M)].cpu().numpy()
    if fmt == U8:
        head = t_soapy(np)[head.reshape(-1, 2)]
    return bool(np.array_equal(y[:n_check].cpu().numpy(), rs.resample(head, taps, L, M, shift)[:n_check]))


def timed(torch, stream, call):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    n = call()
    stop.record(stream)
    stop.synchronize()
    return n, start.elapsed_time(stop)


def kernel_case(np, torch, L, M, fmt, buffers, runs):
    from dump1090_rs_amd import Context, default_resampler_taps
    n_out = buffers * CHUNK
    x = make_input(torch, n_out, L, M, fmt)
    y = torch.empty((n_out + 8, 2), dtype=torch.int16, device="cuda")
    taps, shift = default_resampler_taps(L, M)
    stream = torch.cuda.Stream()
    ms = []
    with Context(0, buffers) as c, c.resampler(L, M) as res:
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            for k in range(3 + runs):
                res.reset()
                n, t = timed(torch, stream, lambda: res.run_device(x.data_ptr(), x.shape[0], y.data_ptr(), n_out + 8, format=fmt))
                assert n_out <= n <= n_out + 1
                if k >= 3:
                    ms.append(t)
        ok = head_ok(np, torch, x, y, taps, shift, L, M, fmt)
        torch.cuda.synchronize()
    med = statistics.median(ms)
    bytes_moved = x.shape[0] * (2 if fmt == U8 else 4) + n_out * 4
    tbps = bytes_moved / (med * 1e-3) / 1e12
    return {"shape": "kernel", "ratio": f"{L}/{M}", "format": "8bit" if fmt == U8 else "cs16", "n_taps": len(taps),
            "phase_taps": -(-len(taps) // L), "out_buffers": buffers, "ms": med, "spread": [min(ms), max(ms)], "runs": len(ms),
            "tb_per_s": tbps, "of_hbm_copy": tbps / HBM_COPY_TBPS, "gsample_in_per_s": x.shape[0] / (med * 1e-3) / 1e9, "parity": ok}


def step_case(np, torch, L, M, fmt, buffers, blocks=5, per_block=10):
    from dump1090_rs_amd import Context, default_resampler_taps
    n_out = buffers * CHUNK
    x = make_input(torch, n_out, L, M, fmt)
    x = x[: n_out * M // L] if L > M else x   # (where L > M: n_out outputs at most, the pass holds no more)
    y = torch.empty((n_out, 2), dtype=torch.int16, device="cuda")
    taps, shift = default_resampler_taps(L, M)
    t = {"resamp": [], "plain": []}
    with Context(0, buffers) as c, c.resampler(L, M) as res:
        n = res.out_count(x.shape[0])
        assert n_out - 1 <= n <= n_out

        def step(with_resamp):
            c.icao_flush()
            if with_resamp:
                res.reset()
                assert res.run_device(x.data_ptr(), x.shape[0], y.data_ptr(), n_out, format=fmt) == n
            c.submit_iq_device(y.data_ptr(), n)
            return c.collect(cap=1 << 16)
        first = step(True)
        ok = head_ok(np, torch, x, y, taps, shift, L, M, fmt)
        ok = ok and [m.buffer() for m in step(False)] == [m.buffer() for m in first]
        for b in range(blocks + 1):
            for name in ("resamp", "plain"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_block):
                    step(name == "resamp")
                if b:
                    t[name].append((time.perf_counter() - t0) / per_block * 1e3)
    return {"shape": "step", "ratio": f"{L}/{M}", "format": "8bit" if fmt == U8 else "cs16", "out_buffers": buffers,
            "ms_per_step_resamp": statistics.median(t["resamp"]), "spread_resamp": [min(t["resamp"]), max(t["resamp"])],
            "ms_per_step_plain": statistics.median(t["plain"]), "spread_plain": [min(t["plain"]), max(t["plain"])],
            "steps": blocks * per_block, "frames": len(first), "parity": ok}


def versus_case(np, torch, M, fmt, buffers, runs):
    """k_resamp at 1/M against k_decim at D = M: the same taps, the same input, runs alternating."""
    from dump1090_rs_amd import Context, default_taps
    n_out = buffers * CHUNK
    x = make_input(torch, n_out, 1, M, fmt)
    y = {name: torch.empty((n_out, 2), dtype=torch.int16, device="cuda") for name in ("resamp", "decim")}
    taps, shift = default_taps(M)
    stream = torch.cuda.Stream()
    ms = {"resamp": [], "decim": []}
    with Context(0, buffers) as c, c.resampler(1, M, taps, shift) as res, c.decimator(M, taps, shift) as dec:
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            for k in range(3 + runs):
                for name, h in (("resamp", res), ("decim", dec)):
                    h.reset()
                    n, t = timed(torch, stream, lambda: h.run_device(x.data_ptr(), x.shape[0], y[name].data_ptr(), n_out, format=fmt))
                    assert n == n_out
                    if k >= 3:
                        ms[name].append(t)
        ok = head_ok(np, torch, x, y["resamp"], taps, shift, 1, M, fmt) and bool(torch.equal(y["resamp"], y["decim"]))
        torch.cuda.synchronize()
    med = {name: statistics.median(v) for name, v in ms.items()}
    return {"shape": "versus", "ratio": f"1/{M}", "format": "8bit" if fmt == U8 else "cs16", "n_taps": len(taps), "out_buffers": buffers,
            "ms_resamp": med["resamp"], "spread_resamp": [min(ms["resamp"]), max(ms["resamp"])],
            "ms_decim": med["decim"], "spread_decim": [min(ms["decim"]), max(ms["decim"])],
            "resamp_over_decim": med["resamp"] / med["decim"], "runs": len(ms["resamp"]), "parity": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=512)
    ap.add_argument("--ratios", default="6/5,24/25,2/5,6/25,3/25")
    ap.add_argument("--versus", default="2,5,10", help="the factors of the comparison with k_decim ('' for none)")
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    ap.add_argument("--no-steps", action="store_true", help="the kernel cases alone")
    a = ap.parse_args()
    import numpy as np
    import torch
    lines = []

    def add(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()
    for L, M in (tuple(int(v) for v in r.split("/")) for r in a.ratios.split(",") if r):
        for fmt in (CS16, U8):
            add(kernel_case(np, torch, L, M, fmt, a.buffers, max(a.runs, 20)))
            if not a.no_steps:
                add(step_case(np, torch, L, M, fmt, a.buffers))
    for M in (int(f) for f in a.versus.split(",") if f):
        for fmt in (CS16, U8):
            add(versus_case(np, torch, M, fmt, a.buffers, max(a.runs, 20)))
    if a.label:
        lines = [{**ln, "build": a.label} for ln in lines]
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "resamp_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

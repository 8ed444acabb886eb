"""What the decimator (adsb_decim_run_device; include/adsb_hip.h, "Decimation") costs.

    python tools/decim_rate.py [--out DIR] [--runs N] [--buffers B] [--factors 2,5,10] [--label TEXT]

Per factor D and input format (CS16, 8-bit), with the default taps (8 D + 1 of them, shift 15):
  kernel   adsb_decim_run_device over the input of B (default 512) output buffers, device memory to device memory,
           timed with HIP events on the stream the context orders its input behind; after 3 warm-up runs, N (default 20,
           at least 20) runs; the median, the spread, and the bytes moved per second -- (4 or 2) D read and 4 written per
           output -- beside the 6.29 TB/s an HBM copy reaches on an MI355X;
  step     icao_flush + run_device + adsb_submit_iq_device + adsb_collect per step against icao_flush + submit +
           collect on the same decimated samples, same process, same context, alternating in blocks of 10 steps; ms per step.
Every case first checks the head of its output against the numpy restatement (tests/decim_support.py).
One JSON line per case goes to stdout and, with --out, is appended to DIR/decim_rate.jsonl.
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


def make_input(torch, n_out, D, fmt):
    """n_out * D samples on the device: a synthetic 2.4 MS/s stream with every sample repeated D times."""
    from dump1090_rs_amd import synth
    base = synth.make_iq_torch(n_out, n_bursts=64, device="cuda")
    if fmt == U8:
        base = torch.clamp(torch.round(base.to(torch.float32) / 256.0 + 127.4), 0, 255).to(torch.uint8)
    x = torch.repeat_interleave(base, D, dim=0).contiguous()
    torch.cuda.synchronize()
    return x


def head_ok(np, torch, x, y, taps, shift, D, fmt, n_check=4096):
    from tests import decim_support as ds
    head = x[: n_check * D].cpu().numpy()
    if fmt == U8:
        head = t_soapy(np)[head.reshape(-1, 2)]
    return bool(np.array_equal(y[:n_check].cpu().numpy(), ds.decimate(head, taps, D, shift)))


def kernel_case(np, torch, D, fmt, buffers, runs):
    from dump1090_rs_amd import Context, default_taps
    n_out = buffers * CHUNK
    x = make_input(torch, n_out, D, fmt)
    y = torch.empty((n_out, 2), dtype=torch.int16, device="cuda")
    taps, shift = default_taps(D)
    stream = torch.cuda.Stream()
    ms = []
    with Context(0, buffers) as c, c.decimator(D) as dec:
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            for k in range(3 + runs):
                dec.reset()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                n = dec.run_device(x.data_ptr(), x.shape[0], y.data_ptr(), n_out, format=fmt)
                stop.record(stream)
                stop.synchronize()
                assert n == n_out
                if k >= 3:
                    ms.append(start.elapsed_time(stop))
        ok = head_ok(np, torch, x, y, taps, shift, D, fmt)
        torch.cuda.synchronize()
    med = statistics.median(ms)
    bytes_moved = n_out * ((2 if fmt == U8 else 4) * D + 4)
    tbps = bytes_moved / (med * 1e-3) / 1e12
    return {"shape": "kernel", "factor": D, "format": "8bit" if fmt == U8 else "cs16", "n_taps": len(taps), "out_buffers": buffers,
            "ms": med, "spread": [min(ms), max(ms)], "runs": len(ms), "tb_per_s": tbps, "of_hbm_copy": tbps / HBM_COPY_TBPS,
            "gsample_in_per_s": n_out * D / (med * 1e-3) / 1e9, "parity": ok}


def step_case(np, torch, D, fmt, buffers, blocks=5, per_block=10):
    from dump1090_rs_amd import Context, default_taps
    n_out = buffers * CHUNK
    x = make_input(torch, n_out, D, fmt)
    y = torch.empty((n_out, 2), dtype=torch.int16, device="cuda")
    taps, shift = default_taps(D)
    t = {"decim": [], "plain": []}
    with Context(0, buffers) as c, c.decimator(D) as dec:
        def step(with_decim):
            c.icao_flush()
            if with_decim:
                dec.reset()
                assert dec.run_device(x.data_ptr(), x.shape[0], y.data_ptr(), n_out, format=fmt) == n_out
            c.submit_iq_device(y.data_ptr(), n_out)
            return c.collect(cap=1 << 16)
        first = step(True)
        ok = head_ok(np, torch, x, y, taps, shift, D, fmt)
        ok = ok and [m.buffer() for m in step(False)] == [m.buffer() for m in first]
        for b in range(blocks + 1):
            for name in ("decim", "plain"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_block):
                    step(name == "decim")
                if b:
                    t[name].append((time.perf_counter() - t0) / per_block * 1e3)
    return {"shape": "step", "factor": D, "format": "8bit" if fmt == U8 else "cs16", "out_buffers": buffers,
            "ms_per_step_decim": statistics.median(t["decim"]), "spread_decim": [min(t["decim"]), max(t["decim"])],
            "ms_per_step_plain": statistics.median(t["plain"]), "spread_plain": [min(t["plain"]), max(t["plain"])],
            "steps": blocks * per_block, "frames": len(first), "parity": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=512)
    ap.add_argument("--factors", default="2,5,10")
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    ap.add_argument("--no-steps", action="store_true", help="the kernel cases alone")
    a = ap.parse_args()
    import numpy as np
    import torch
    lines = []
    for D in (int(f) for f in a.factors.split(",")):
        for fmt in (CS16, U8):
            lines.append(kernel_case(np, torch, D, fmt, a.buffers, max(a.runs, 20)))
            print(json.dumps(lines[-1]), flush=True)
            if not a.no_steps:
                lines.append(step_case(np, torch, D, fmt, a.buffers))
                print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.label:
        lines = [{**ln, "build": a.label} for ln in lines]
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "decim_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

"""What CF32 and REAL16 input cost in the decimator and the resampler (include/adsb_hip.h, "Sample formats"), and that
CS16 and 8-bit input cost what the parent commit's did.

    python tools/formats_in_rate.py [--parent-lib PATH] [--out DIR] [--blocks 5] [--per-block 4] [--buffers 512] [--label TEXT]

Per case -- k_decim at D = 2, 5, 10 and k_resamp at 6/5, 24/25, 6/25, 3/25, the mixer off and on with adsb_mix_table(1, 4),
the default taps, the input of B (default 512) output buffers, device memory to device memory -- one process times
*_run_device with HIP events on the stream the contexts order their input behind, in interleaved blocks of --per-block
runs, after one untimed block:
  cs16, 8bit, cf32, real16   this build, one handle per format (the same 2.4 MS/s synthetic stream under all four: cf32
                             is cs16 / 32768, real16 its real part);
  parent_cs16, parent_8bit   the parent commit's library loaded beside this one (--parent-lib: its libadsb_hip.so, built
                             on this machine), and parent_cs16_again, a second handle of it: what two handles of ONE
                             library differ by.
A line holds each variant's median over all its runs, its min-max spread over its blocks' medians, cs16 / parent_cs16 and
8bit / parent_8bit with `inside_parent_spread` (the expectation: no change beyond the parent's own run-to-run spread), and
cf32 / cs16, real16 / cs16: the new formats' cost at the same D or ratio, an observation.  Parity: cs16 and 8bit equal the
parent's output, cf32 equals cs16's output (q brings the samples back exactly), and the head of real16's output equals
the numpy restatement (tests/formats_in_support.py, tests/mix_support.py).  One JSON line per case goes to stdout and,
with --out, is appended to DIR/formats_in_rate.jsonl.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CHUNK = 131072
CS16, U8, CF32, REAL16 = 0, 1, 2, 3
CASES = [("decim", 1, 2), ("decim", 1, 5), ("decim", 1, 10), ("resamp", 6, 5), ("resamp", 24, 25), ("resamp", 6, 25), ("resamp", 3, 25)]


def real_head_ok(np, x, y, h, kind, L, M, n_check=4096):
    from tests import formats_in_support as fi
    from tests import mix_support as ms
    from tools.resamp_rate import inputs_for
    head = fi.real_to_cs16(x[: inputs_for(n_check, L, M)].cpu().numpy())
    want = ms.decimate(head, h.taps, M, h.shift, h.table) if kind == "decim" else ms.resample(head, h.taps, L, M, h.shift, h.table)
    return bool(np.array_equal(y[:n_check].cpu().numpy(), want[:n_check]))


def case(np, torch, libs, kind, L, M, period, buffers, blocks, per_block):
    from tools.mix_rate import Handle
    from tools.resamp_rate import make_input, timed
    n_out = buffers * CHUNK
    x = {CS16: make_input(torch, n_out, L, M, CS16), U8: make_input(torch, n_out, L, M, U8)}
    x[CF32] = (x[CS16].to(torch.float32) / 32768.0).contiguous()
    x[REAL16] = x[CS16][:, 0].contiguous()
    stream = torch.cuda.Stream()
    variants = {}   # name -> (handle, format)
    if "parent" in libs:
        variants["parent_cs16"] = (Handle(np, libs["parent"], kind, L, M, stream.cuda_stream, period), CS16)
        variants["parent_8bit"] = (Handle(np, libs["parent"], kind, L, M, stream.cuda_stream, period), U8)
    for name, fmt in (("cs16", CS16), ("8bit", U8), ("cf32", CF32), ("real16", REAL16)):
        variants[name] = (Handle(np, libs["this"], kind, L, M, stream.cuda_stream, period), fmt)
    if "parent" in libs:
        variants["parent_cs16_again"] = (Handle(np, libs["parent"], kind, L, M, stream.cuda_stream, period), CS16)
    y = {name: torch.empty((n_out + 8, 2), dtype=torch.int16, device="cuda") for name in variants}
    ms_blocks = {name: [] for name in variants}
    with torch.cuda.stream(stream):
        for b in range(blocks + 1):
            for name, (h, fmt) in variants.items():
                t = []
                for _ in range(per_block):
                    h.reset()
                    n, dt = timed(torch, stream, lambda: h.run(x[fmt], y[name], fmt))
                    assert n_out <= n <= n_out + 1
                    t.append(dt)
                if b:
                    ms_blocks[name].append(t)
    torch.cuda.synchronize()
    ok = bool(torch.equal(y["cf32"][:n_out], y["cs16"][:n_out])) and real_head_ok(np, x[REAL16], y["real16"], variants["real16"][0], kind, L, M)
    ok = ok and not torch.equal(y["real16"][:n_out], y["cs16"][:n_out])
    if "parent" in libs:
        ok = ok and bool(torch.equal(y["cs16"][:n_out], y["parent_cs16"][:n_out])) and bool(torch.equal(y["8bit"][:n_out], y["parent_8bit"][:n_out]))
    n_taps = len(variants["cs16"][0].taps)
    for h, _ in variants.values():
        h.close()
    med = {name: statistics.median(v for blk in t for v in blk) for name, t in ms_blocks.items()}
    spread = {name: [min(statistics.median(blk) for blk in t), max(statistics.median(blk) for blk in t)] for name, t in ms_blocks.items()}
    line = {"shape": "formats_in", "kernel": "k_decim" if kind == "decim" else "k_resamp", "ratio": f"{L}/{M}", "mixer_period": period,
            "n_taps": n_taps, "out_buffers": buffers, "runs": blocks * per_block, "ms": med, "block_spread_ms": spread,
            "gsample_in_per_s": {name: x[variants[name][1]].shape[0] / (v * 1e-3) / 1e9 for name, v in med.items()},
            "gbyte_in_per_s": {name: x[variants[name][1]].shape[0] * (8, 4, 2, 2)[(CF32, CS16, U8, REAL16).index(variants[name][1])] / (v * 1e-3) / 1e9
                               for name, v in med.items()},
            "cf32_over_cs16": med["cf32"] / med["cs16"], "real16_over_cs16": med["real16"] / med["cs16"], "parity": ok}
    if "parent" in libs:
        line["cs16_over_parent"] = med["cs16"] / med["parent_cs16"]
        line["8bit_over_parent"] = med["8bit"] / med["parent_8bit"]
        line["parent_again_over_parent"] = med["parent_cs16_again"] / med["parent_cs16"]
        lo, hi = (f(spread["parent_cs16"][i], spread["parent_cs16_again"][i]) for i, f in ((0, min), (1, max)))
        line["cs16_inside_parent_spread"] = lo <= med["cs16"] <= hi
        line["8bit_inside_parent_spread"] = spread["parent_8bit"][0] <= med["8bit"] <= spread["parent_8bit"][1]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libadsb_hip.so, built on this machine")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4)
    ap.add_argument("--buffers", type=int, default=512)
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    a = ap.parse_args()
    import numpy as np
    import torch
    from tools.mix_rate import load
    libs = {"this": load(None)}
    if a.parent_lib:
        import ctypes as C
        libs["parent"] = load(a.parent_lib)
        # (the parent's handles carry the mixer here too, which tools/mix_rate.py never asked of it)
        libs["parent"].adsb_mix_table.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int16), C.c_size_t]
        for kind in ("decim", "resamp"):
            getattr(libs["parent"], f"adsb_mix_set_{kind}").argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lines = []
    for kind, L, M in CASES:
        for period in (0, 4):
            line = case(np, torch, libs, kind, L, M, period, a.buffers, a.blocks, a.per_block)
            if a.label:
                line["build"] = a.label
            lines.append(line)
            print(json.dumps(line), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "formats_in_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

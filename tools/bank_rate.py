"""What a resampler bank (include/adsb_hip.h, "Resampler banks") buys over one resampler per receiver, what its batch
dimension costs, and that the single resampler costs what the parent commit's did.

    python tools/bank_rate.py [--parent-lib PATH] [--out DIR] [--blocks 5] [--per-block 4] [--streams 8,64,512] [--label TEXT]

Per case -- 1/5, 6/25 and 3/25 in CS16, 6/25 in CF32, 6/25 in CS16 with the mixer adsb_mix_table(1, 4), the default taps --
and per R of --streams, every stream is given the inputs of exactly one 131072-sample output buffer, device memory to
device memory.  One process times, with HIP events on the stream the contexts order their input behind, in interleaved
blocks of --per-block runs after one untimed block (every stream is reset in front of a run, outside the timed span):
  bank      one adsb_bank_run_device call on a bank of R streams;
  handles   R adsb_resamp_run_device calls on R handles of one context, one behind the other: what a host had to do
            before.  (a) handles / bank is the figure the bank exists for.
At the largest R, over the same R x 131072 outputs in ONE call of one stream:
  single    one adsb_resamp handle of this build.  (b) bank / single is the price of the batch dimension;
  parent, parent_again   (--parent-lib: the parent commit's libadsb_hip.so, built on this machine, loaded beside this one)
            two handles of the parent's library.  (c) single / parent, expected inside the spread of the parent's own two
            handles, which the same run records.
A line holds each variant's median over all its runs and its min-max spread over its blocks' medians.  Parity: every
stream of the bank equals its handle's output byte for byte, the head of stream 0 equals the numpy restatement
(tests/resamp_support.py, tests/mix_support.py), and `single` equals the parent's output.  One JSON line per (case, R) goes
to stdout and, with --out, is appended to DIR/bank_rate.jsonl.
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
CS16, CF32 = 0, 2
CASES = [(1, 5, CS16, 0), (6, 25, CS16, 0), (3, 25, CS16, 0), (6, 25, CF32, 0), (6, 25, CS16, 4)]


def head_ok(np, x0, y0, taps, shift, table, L, M, fmt, n_check=4096):
    from tests import formats_in_support as fi
    from tests import mix_support as ms
    from tools.resamp_rate import inputs_for
    head = fi.to_cs16(x0[: inputs_for(n_check, L, M)].cpu().numpy(), fmt)
    return bool(np.array_equal(y0[:n_check].cpu().numpy(), ms.resample(head, taps, L, M, shift, table)[:n_check]))


def case(np, torch, libs, L, M, fmt, period, R, with_single, blocks, per_block):
    from dump1090_rs_amd import Context, default_resampler_taps, mixer_table
    from tools.mix_rate import Handle
    from tools.resamp_rate import inputs_for, make_input, timed
    n_i = inputs_for(CHUNK, L, M)
    stride = (n_i + 3) & ~3   # every stream's inputs start on 16 bytes
    x = make_input(torch, R * CHUNK + 8 * R + 8, L, M, CS16)
    assert x.shape[0] >= R * stride and x.shape[0] >= inputs_for(R * CHUNK, L, M)
    if fmt == CF32:
        x = (x.to(torch.float32) / 32768.0).contiguous()
    bps = x.element_size() * 2
    taps, shift = default_resampler_taps(L, M)
    table = mixer_table(1, period) if period else None
    stream = torch.cuda.Stream()
    y = {name: torch.empty((R * CHUNK + 8, 2), dtype=torch.int16, device="cuda") for name in ("bank", "handles")}
    streams = np.arange(R, dtype=np.uint32)
    p_in = x.data_ptr() + np.arange(R, dtype=np.int64) * (stride * bps)
    p_out = {name: y[name].data_ptr() + np.arange(R, dtype=np.int64) * (CHUNK * 4) for name in y}
    counts, caps = np.full(R, n_i), np.full(R, CHUNK)
    ctx = Context(0, 1)
    ctx.set_stream(stream.cuda_stream)
    bank = ctx.resampler_bank(R, L, M, taps, shift)
    handles = [ctx.resampler(L, M, taps, shift) for _ in range(R)]
    for h in [bank] + handles:
        if period:
            h.set_mixer(table)
    single = {}
    if with_single:
        single["single"] = Handle(np, libs["this"], "resamp", L, M, stream.cuda_stream, period)
        if "parent" in libs:
            single["parent"] = Handle(np, libs["parent"], "resamp", L, M, stream.cuda_stream, period)
            single["parent_again"] = Handle(np, libs["parent"], "resamp", L, M, stream.cuda_stream, period)
        for name in single:
            y[name] = torch.empty((R * CHUNK + 8, 2), dtype=torch.int16, device="cuda")
    x_single = x[: inputs_for(R * CHUNK, L, M)]

    def run_bank():
        n = bank.run_device(streams, p_in, counts, p_out["bank"], caps, format=fmt)
        return int(n.sum())

    def run_handles():
        return sum(h.run_device(int(p_in[r]), n_i, int(p_out["handles"][r]), CHUNK, format=fmt) for r, h in enumerate(handles))

    variants = {"bank": (bank.reset, run_bank), "handles": (lambda: [h.reset() for h in handles], run_handles)}
    for name, h in single.items():
        variants[name] = (h.reset, lambda h=h, name=name: min(h.run(x_single, y[name], fmt), R * CHUNK))
    ms_blocks = {name: [] for name in variants}
    with torch.cuda.stream(stream):
        for b in range(blocks + 1):
            for name, (reset, run) in variants.items():
                t = []
                for _ in range(per_block):
                    reset()
                    n, dt = timed(torch, stream, run)
                    assert n == R * CHUNK, (name, n)
                    t.append(dt)
                if b:
                    ms_blocks[name].append(t)
    torch.cuda.synchronize()
    ok = bool(torch.equal(y["bank"][: R * CHUNK], y["handles"][: R * CHUNK]))
    ok = ok and head_ok(np, x[: n_i], y["bank"], taps, shift, table, L, M, fmt)
    if "parent" in single:
        ok = ok and bool(torch.equal(y["single"][: R * CHUNK], y["parent"][: R * CHUNK]))
    for h in [bank] + handles:
        h.close()
    for h in single.values():
        h.close()
    ctx.close()
    med = {name: statistics.median(v for blk in t for v in blk) for name, t in ms_blocks.items()}
    spread = {name: [min(statistics.median(blk) for blk in t), max(statistics.median(blk) for blk in t)] for name, t in ms_blocks.items()}
    line = {"shape": "bank", "ratio": f"{L}/{M}", "format": "cf32" if fmt == CF32 else "cs16", "mixer_period": period, "streams": R,
            "n_taps": len(taps), "runs": blocks * per_block, "ms": med, "block_spread_ms": spread,
            "goutput_per_s": {name: R * CHUNK / (v * 1e-3) / 1e9 for name, v in med.items()},
            "handles_over_bank": med["handles"] / med["bank"], "parity": ok}
    if "single" in med:
        line["bank_over_single"] = med["bank"] / med["single"]
    if "parent" in med:
        line["single_over_parent"] = med["single"] / med["parent"]
        line["parent_again_over_parent"] = med["parent_again"] / med["parent"]
        lo, hi = (f(spread["parent"][i], spread["parent_again"][i]) for i, f in ((0, min), (1, max)))
        line["single_inside_parent_spread"] = lo <= med["single"] <= hi
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libadsb_hip.so, built on this machine")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4)
    ap.add_argument("--streams", default="8,64,512")
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    a = ap.parse_args()
    import numpy as np
    import torch
    from tools.mix_rate import load
    libs = {"this": load(None)}
    if a.parent_lib:
        import ctypes as C
        libs["parent"] = load(a.parent_lib)
        libs["parent"].adsb_mix_table.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int16), C.c_size_t]
        libs["parent"].adsb_mix_set_resamp.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    widths = sorted(int(v) for v in a.streams.split(",") if v)
    lines = []
    for L, M, fmt, period in CASES:
        for R in widths:
            line = case(np, torch, libs, L, M, fmt, period, R, R == widths[-1], a.blocks, a.per_block)
            if a.label:
                line["build"] = a.label
            lines.append(line)
            print(json.dumps(line), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "bank_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

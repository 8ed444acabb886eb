"""What the input statistics of a decimator, a resampler or a bank (include/adsb_hip.h, "Input statistics") cost, how near
k_instat comes to a plain copy of the same bytes, and that a handle with the mode off costs what the parent commit's did.

    python tools/instat_rate.py [--parent-lib PATH] [--out DIR] [--blocks 5] [--per-block 4] [--buffers 512] [--streams 512] [--label TEXT]

Per case -- k_decim at D = 2, 10 and k_resamp at 6/25, 3/25, in CS16, 8-bit, CF32 and REAL16, the default taps, the input
of B (default 512) output buffers, device memory to device memory -- one process times with HIP events on the stream the
contexts order their input behind, in interleaved blocks of --per-block runs after one untimed block:
  copy     a device-to-device copy of the call's input bytes: the "HBM copy rate" the decimator and resampler rows quote;
  off      *_run_device of this build with the mode off: the launches the parent made;
  on       the same with the mode on: k_instat in front of the filter's launch, on the same stream.
           (b) on / off is what the mode costs a call.  (a) k_instat alone is on - off -- the two launches run one behind
           the other, and no entry point launches k_instat by itself -- against `copy`: instat_over_copy;
  parent, parent_again   (--parent-lib: the parent commit's libadsb_hip.so, built on this machine, loaded beside this one)
           two handles of the parent's library.  (c) off / parent, expected inside the spread of the parent's own two
           handles, which the same run records.
(d) per resampler ratio, in CS16: one adsb_bank_run_device call over --streams streams of one output buffer each, mode on
against off.
A line holds each variant's median over all its runs and its min-max spread over its blocks' medians.  Parity: `on`, `off`
and the parent give the same output bytes, and the record `on` fetches equals the numpy restatement
(tests/instat_support.py) over the head of the input, and its n_samples the whole input times the runs it counted.  One JSON line per case goes to stdout and,
with --out, is appended to DIR/instat_rate.jsonl.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CHUNK = 131072
CS16, U8, CF32, REAL16 = 0, 1, 2, 3
NAMES = {CS16: "cs16", U8: "8bit", CF32: "cf32", REAL16: "real16"}
CASES = [("decim", 1, 2), ("decim", 1, 10), ("resamp", 6, 25), ("resamp", 3, 25)]


def make_input(torch, n_out, L, M, fmt):
    from tools.resamp_rate import make_input as base
    if fmt in (CS16, U8):
        return base(torch, n_out, L, M, fmt)
    x = base(torch, n_out, L, M, CS16)
    if fmt == CF32:
        return (x.to(torch.float32) / 32768.0).contiguous()
    return x[:, 0].contiguous()


def record_ok(np, x, fmt, got, runs):
    """`got` (one adsb_input_stats as a numpy record) is `runs` times the restatement's record of x."""
    from tests import instat_support as ist
    from tools.resamp_rate import t_soapy
    want = ist.record(x.cpu().numpy(), fmt, table=t_soapy(np))
    ok = int(got["peak"]) == int(want["peak"])
    for name in ist.DTYPE.names:
        if name not in ("peak", "reserved"):
            ok = ok and np.array_equal(np.asarray(got[name]).astype(np.int64), np.asarray(want[name]).astype(np.int64) * runs)
    return bool(ok)


def summarise(ms_blocks):
    med = {name: statistics.median(v for blk in t for v in blk) for name, t in ms_blocks.items()}
    spread = {name: [min(statistics.median(blk) for blk in t), max(statistics.median(blk) for blk in t)] for name, t in ms_blocks.items()}
    return med, spread


def case(np, torch, libs, kind, L, M, fmt, buffers, blocks, per_block):
    from dump1090_rs_amd import _lib
    from tools.mix_rate import Handle
    from tools.resamp_rate import timed
    n_out = buffers * CHUNK
    x = make_input(torch, n_out, L, M, fmt)
    scratch = torch.empty_like(x)
    stream = torch.cuda.Stream()
    variants = {}
    if "parent" in libs:
        variants["parent"] = Handle(np, libs["parent"], kind, L, M, stream.cuda_stream)
    variants["off"] = Handle(np, libs["this"], kind, L, M, stream.cuda_stream)
    variants["on"] = Handle(np, libs["this"], kind, L, M, stream.cuda_stream)
    if "parent" in libs:
        variants["parent_again"] = Handle(np, libs["parent"], kind, L, M, stream.cuda_stream)
    this = libs["this"]
    assert getattr(this, f"adsb_instat_set_{kind}")(variants["on"].h, 1) == 0
    y = {name: torch.empty((n_out + 8, 2), dtype=torch.int16, device="cuda") for name in variants}
    ms_blocks = {name: [] for name in list(variants) + ["copy"]}
    counted = 0
    with torch.cuda.stream(stream):
        for b in range(blocks + 1):
            for name in ms_blocks:
                t = []
                for _ in range(per_block):
                    if name == "copy":
                        _, dt = timed(torch, stream, lambda: scratch.copy_(x, non_blocking=True))
                    else:
                        h = variants[name]
                        h.reset()
                        n, dt = timed(torch, stream, lambda: h.run(x, y[name], fmt))
                        assert n_out <= n <= n_out + 1
                        counted += name == "on"
                    t.append(dt)
                if b:
                    ms_blocks[name].append(t)
    torch.cuda.synchronize()
    from dump1090_rs_amd.context import INPUT_STATS_DTYPE
    ok = bool(torch.equal(y["on"][:n_out], y["off"][:n_out]))

    def fetch():
        rec = _lib.AdsbInputStats()
        assert getattr(this, f"adsb_instat_fetch_{kind}")(variants["on"].h, C.byref(rec)) == 0
        return np.frombuffer(bytes(rec), dtype=INPUT_STATS_DTYPE)[0]
    # every timed run counted the whole input; then the head of it once more, against the restatement field by field
    ok = ok and int(fetch()["n_samples"]) == counted * x.shape[0]
    head = x[: min(x.shape[0], 1 << 20)]
    with torch.cuda.stream(stream):
        variants["on"].run(head, y["on"], fmt)
    ok = ok and record_ok(np, head, fmt, fetch(), 1)
    counted += 1
    if "parent" in variants:
        ok = ok and bool(torch.equal(y["off"][:n_out], y["parent"][:n_out]))
    launches = {name: int(getattr(this, f"adsb_instat_selftest_launches_{kind}")(variants[name].h)) for name in ("off", "on")}
    ok = ok and launches == {"off": 0, "on": counted}
    for h in variants.values():
        h.close()
    med, spread = summarise(ms_blocks)
    in_bytes = x.numel() * x.element_size()
    instat_ms = med["on"] - med["off"]
    line = {"shape": "instat", "kernel": "k_decim" if kind == "decim" else "k_resamp", "ratio": f"{L}/{M}", "format": NAMES[fmt],
            "out_buffers": buffers, "in_bytes": in_bytes, "runs": blocks * per_block, "ms": med, "block_spread_ms": spread,
            "copy_gb_per_s": in_bytes / (med["copy"] * 1e-3) / 1e9, "instat_ms_on_minus_off": instat_ms,
            "instat_gb_per_s": in_bytes / (instat_ms * 1e-3) / 1e9 if instat_ms > 0 else None,
            "instat_over_copy": instat_ms / med["copy"], "on_over_off": med["on"] / med["off"], "parity": ok}
    if "parent" in med:
        line["off_over_parent"] = med["off"] / med["parent"]
        line["parent_again_over_parent"] = med["parent_again"] / med["parent"]
        lo, hi = (f(spread["parent"][i], spread["parent_again"][i]) for i, f in ((0, min), (1, max)))
        line["off_inside_parent_spread"] = lo <= med["off"] <= hi
    return line


def bank_case(np, torch, L, M, R, blocks, per_block):
    from dump1090_rs_amd import Context, default_resampler_taps
    from tests import instat_support as ist
    from tools.resamp_rate import inputs_for, make_input as base, timed
    n_i = inputs_for(CHUNK, L, M)
    stride = (n_i + 3) & ~3
    x = base(torch, R * CHUNK + 8 * R + 8, L, M, CS16)
    assert x.shape[0] >= R * stride
    taps, shift = default_resampler_taps(L, M)
    stream = torch.cuda.Stream()
    streams = np.arange(R, dtype=np.uint32)
    p_in = x.data_ptr() + np.arange(R, dtype=np.int64) * (stride * 4)
    counts, caps = np.full(R, n_i), np.full(R, CHUNK)
    ctx = Context(0, 1)
    ctx.set_stream(stream.cuda_stream)
    banks = {name: ctx.resampler_bank(R, L, M, taps, shift) for name in ("off", "on")}
    banks["on"].set_input_stats(True)
    y = {name: torch.empty((R * CHUNK + 8, 2), dtype=torch.int16, device="cuda") for name in banks}
    p_out = {name: y[name].data_ptr() + np.arange(R, dtype=np.int64) * (CHUNK * 4) for name in banks}
    ms_blocks = {name: [] for name in banks}
    counted = 0
    with torch.cuda.stream(stream):
        for b in range(blocks + 1):
            for name, bank in banks.items():
                t = []
                for _ in range(per_block):
                    bank.reset()
                    n, dt = timed(torch, stream, lambda: int(bank.run_device(streams, p_in, counts, p_out[name], caps).sum()))
                    assert n == R * CHUNK
                    counted += name == "on"
                    t.append(dt)
                if b:
                    ms_blocks[name].append(t)
    torch.cuda.synchronize()
    got = banks["on"].input_stats()
    ok = bool(torch.equal(y["on"][: R * CHUNK], y["off"][: R * CHUNK]))
    for r in (0, R // 2, R - 1):
        want = ist.record(x[r * stride: r * stride + n_i].cpu().numpy(), CS16)
        ok = ok and int(got[r]["n_samples"]) == counted * n_i and int(got[r]["sum_re2"]) == counted * int(want["sum_re2"])
        ok = ok and np.array_equal(got[r]["hist"], want["hist"] * counted) and int(got[r]["peak"]) == int(want["peak"])
    for bank in banks.values():
        bank.close()
    ctx.close()
    med, spread = summarise(ms_blocks)
    return {"shape": "instat_bank", "ratio": f"{L}/{M}", "format": "cs16", "streams": R, "runs": blocks * per_block, "ms": med,
            "block_spread_ms": spread, "on_over_off": med["on"] / med["off"], "parity": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libadsb_hip.so, built on this machine")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4)
    ap.add_argument("--buffers", type=int, default=512)
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    a = ap.parse_args()
    import numpy as np
    import torch
    from tools.mix_rate import load
    libs = {"this": load(None)}
    if a.parent_lib:
        libs["parent"] = load(a.parent_lib)
    lines = []

    def add(line):
        if a.label:
            line["build"] = a.label
        lines.append(line)
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()
    for kind, L, M in CASES:
        for fmt in (CS16, U8, CF32, REAL16):
            add(case(np, torch, libs, kind, L, M, fmt, a.buffers, a.blocks, a.per_block))
    for kind, L, M in CASES:
        if kind == "resamp":
            add(bank_case(np, torch, L, M, a.streams, a.blocks, a.per_block))
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "instat_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

"""What the mixer of the decimator and the resampler (include/adsb_hip.h, "Frequency shift") costs, and that the kernels
without it cost what the parent commit's did.

    python tools/mix_rate.py [--parent-lib PATH] [--out DIR] [--blocks 5] [--per-block 4] [--buffers 512] [--label TEXT]

Per case -- k_decim at D = 2, 5, 10 and k_resamp at 24/25, 6/25, 3/25, CS16 and 8-bit input, the default taps, the input of
B (default 512) output buffers, device memory to device memory -- one process times *_run_device with HIP events on the
stream the contexts order their input behind, in interleaved blocks of --per-block runs, after one untimed block:
  parent   the parent commit's library loaded beside this one (--parent-lib: its libadsb_hip.so, built on this machine);
  off      this build, no mixer: the instantiations the parent had;
  n4, n125 this build, the mixer on with adsb_mix_table(1, 4) and adsb_mix_table(1, 125);
  parent_again  a second handle of the parent's library with an output buffer of its own: what two handles of ONE library
           differ by, by their place in memory and in the block alone.
A line holds each variant's median over all its runs, its min-max spread over its blocks' medians, off / parent with
`off_inside_parent_spread` (the expectation: no change beyond the parent's own run-to-run spread -- the blocks of both of
its handles), and n4 / off, n125 / off:
the mixer's cost, an observation.  Parity: `off` equals the parent's output, and the head of every mixed output equals the
numpy restatement (tests/mix_support.py).  One JSON line per case goes to stdout and, with --out, is appended to
DIR/mix_rate.jsonl.
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
CS16, U8 = 0, 1
CASES = [("decim", 1, 2), ("decim", 1, 5), ("decim", 1, 10), ("resamp", 24, 25), ("resamp", 6, 25), ("resamp", 3, 25)]


def load(path):
    from dump1090_rs_amd import _lib
    if path is None:
        return _lib.lib()
    L = C.CDLL(str(path))
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    i16p, u32p = C.POINTER(C.c_int16), C.POINTER(u32)
    L.adsb_create.argtypes = [C.POINTER(vp), C.c_int, sz]
    L.adsb_destroy.argtypes = [vp]
    L.adsb_destroy.restype = None
    L.adsb_set_stream.argtypes = [vp, vp]
    L.adsb_decim_create.argtypes = [vp, u32, vp, u32, u32, C.POINTER(vp)]
    L.adsb_resamp_create.argtypes = [vp, u32, u32, vp, u32, u32, C.POINTER(vp)]
    L.adsb_decim_default_taps.argtypes = [u32, i16p, sz, u32p, u32p]
    L.adsb_resamp_default_taps.argtypes = [u32, u32, i16p, sz, u32p, u32p]
    for kind in ("decim", "resamp"):
        getattr(L, f"adsb_{kind}_destroy").argtypes = [vp]
        getattr(L, f"adsb_{kind}_destroy").restype = None
        getattr(L, f"adsb_{kind}_reset").argtypes = [vp]
        getattr(L, f"adsb_{kind}_run_device").argtypes = [vp, C.c_int, vp, sz, vp, sz, C.POINTER(sz)]
    return L


class Handle:
    """A context and one decimator or resampler with its default taps, through the bare C ABI of `lib`."""

    def __init__(self, np, lib, kind, L, M, stream, mixer_period=0):
        self.lib, self.kind = lib, kind
        self.ctx, self.h = C.c_void_p(), C.c_void_p()
        assert lib.adsb_create(C.byref(self.ctx), 0, 1) == 0
        assert lib.adsb_set_stream(self.ctx, C.c_void_p(stream)) == 0
        taps = np.zeros(8 * 128 + 1, np.int16)
        n, shift = C.c_uint32(), C.c_uint32()
        tp = taps.ctypes.data_as(C.POINTER(C.c_int16))
        if kind == "decim":
            assert lib.adsb_decim_default_taps(M, tp, taps.size, C.byref(n), C.byref(shift)) == 0
            assert lib.adsb_decim_create(self.ctx, M, taps.ctypes.data, n.value, shift.value, C.byref(self.h)) == 0
        else:
            assert lib.adsb_resamp_default_taps(L, M, tp, taps.size, C.byref(n), C.byref(shift)) == 0
            assert lib.adsb_resamp_create(self.ctx, L, M, taps.ctypes.data, n.value, shift.value, C.byref(self.h)) == 0
        self.taps, self.shift, self.table = taps[: n.value].copy(), shift.value, None
        if mixer_period:
            self.table = np.zeros((mixer_period, 2), np.int16)
            assert lib.adsb_mix_table(1, mixer_period, self.table.ctypes.data_as(C.POINTER(C.c_int16)), mixer_period) == 0
            assert getattr(lib, f"adsb_mix_set_{kind}")(self.h, self.table.ctypes.data, mixer_period) == 0
        self._reset = getattr(lib, f"adsb_{kind}_reset")
        self._run = getattr(lib, f"adsb_{kind}_run_device")

    def reset(self):
        assert self._reset(self.h) == 0

    def run(self, x, y, fmt):
        n = C.c_size_t()
        assert self._run(self.h, fmt, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(y.data_ptr()), y.shape[0], C.byref(n)) == 0
        return n.value

    def close(self):
        getattr(self.lib, f"adsb_{self.kind}_destroy")(self.h)
        self.lib.adsb_destroy(self.ctx)


def head_ok(np, x, y, h, kind, L, M, fmt, n_check=4096):
    from tests import mix_support as ms
    from tools.resamp_rate import inputs_for, t_soapy
    head = x[: inputs_for(n_check, L, M)].cpu().numpy()
    if fmt == U8:
        head = t_soapy(np)[head.reshape(-1, 2)]
    want = ms.decimate(head, h.taps, M, h.shift, h.table) if kind == "decim" else ms.resample(head, h.taps, L, M, h.shift, h.table)
    return bool(np.array_equal(y[:n_check].cpu().numpy(), want[:n_check]))


def case(np, torch, libs, kind, L, M, fmt, buffers, blocks, per_block):
    from tools.resamp_rate import make_input, timed
    n_out = buffers * CHUNK
    x = make_input(torch, n_out, L, M, fmt)
    stream = torch.cuda.Stream()
    variants = {}
    if "parent" in libs:
        variants["parent"] = Handle(np, libs["parent"], kind, L, M, stream.cuda_stream)
    for name, period in (("off", 0), ("n4", 4), ("n125", 125)):
        variants[name] = Handle(np, libs["this"], kind, L, M, stream.cuda_stream, period)
    if "parent" in libs:
        variants["parent_again"] = Handle(np, libs["parent"], kind, L, M, stream.cuda_stream)
    y = {name: torch.empty((n_out + 8, 2), dtype=torch.int16, device="cuda") for name in variants}
    ms_blocks = {name: [] for name in variants}
    with torch.cuda.stream(stream):
        for b in range(blocks + 1):
            for name, h in variants.items():
                t = []
                for _ in range(per_block):
                    h.reset()
                    n, dt = timed(torch, stream, lambda: h.run(x, y[name], fmt))
                    assert n_out <= n <= n_out + 1
                    t.append(dt)
                if b:
                    ms_blocks[name].append(t)
    torch.cuda.synchronize()
    ok = all(head_ok(np, x, y[name], h, kind, L, M, fmt) for name, h in variants.items())
    if "parent" in variants:
        ok = ok and bool(torch.equal(y["off"][:n_out], y["parent"][:n_out]))
    ok = ok and not torch.equal(y["off"][:n_out], y["n4"][:n_out])
    for h in variants.values():
        h.close()
    med = {name: statistics.median(v for blk in t for v in blk) for name, t in ms_blocks.items()}
    spread = {name: [min(statistics.median(blk) for blk in t), max(statistics.median(blk) for blk in t)] for name, t in ms_blocks.items()}
    line = {"shape": "mix", "kernel": "k_decim" if kind == "decim" else "k_resamp", "ratio": f"{L}/{M}", "format": "8bit" if fmt == U8 else "cs16",
            "n_taps": len(variants["off"].taps), "out_buffers": buffers, "runs": blocks * per_block, "ms": med, "block_spread_ms": spread,
            "gsample_in_per_s": {name: x.shape[0] / (v * 1e-3) / 1e9 for name, v in med.items()},
            "n4_over_off": med["n4"] / med["off"], "n125_over_off": med["n125"] / med["off"], "parity": ok}
    if "parent" in med:
        line["off_over_parent"] = med["off"] / med["parent"]
        line["parent_again_over_parent"] = med["parent_again"] / med["parent"]
        lo, hi = (f(spread["parent"][i], spread["parent_again"][i]) for i, f in ((0, min), (1, max)))
        line["off_inside_parent_spread"] = lo <= med["off"] <= hi
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
    libs = {"this": load(None)}
    if a.parent_lib:
        libs["parent"] = load(a.parent_lib)
    lines = []
    for kind, L, M in CASES:
        for fmt in (CS16, U8):
            line = case(np, torch, libs, kind, L, M, fmt, a.buffers, a.blocks, a.per_block)
            if a.label:
                line["build"] = a.label
            lines.append(line)
            print(json.dumps(line), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "mix_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

"""What scoring per receiver on the device (adsb_set_receiver_scoring, include/adsb_hip.h) does to a dense many-receiver
step, against the parent commit's library, whose host-pooled replay is the yardstick.

    python tools/receivers_scored_rate.py --parent-lib PATH [--blocks 6] [--out DIR] [--label TEXT] [--parent-scoring]

One process, three contexts of 512 buffers with receivers on, driven through the bare C ABI: the parent commit's library
(PATH: its libadsb_hip.so, built on this box), this build with scoring on, and this build with scoring off.  (--order: another
order, or a second context of the parent's library as `parent_again`.  --parent-scoring: the parent's contexts score on
the device too -- for a commit that changes the scoring kernels and not what they do: `on_inside_parent_spread` then says
whether this build's step with scoring on lies inside the spread of the parent's own blocks.)  The input
is one resident 512-buffer dense pass (5000 bursts: bench.py's config-5 input); the step is adsb_icao_flush + submit with
four passes in flight, in blocks of 20 steps between device fences, and the three take turns block by block.  Twice: with
a map of 512 receivers (one buffer each) and one of 8.

Every collected list is compared with a reference list of its map that was itself compared, message by message, with
tests/receivers_support.py's Model (one CPU oracle per receiver).

Per map one JSON line (stdout and, with --out, appended to DIR/receivers_scored_rate.jsonl): per context ms per step of
every block (the first block is warm-up and is left out of the medians), host CPU time per pass (process time over the
block, all threads: the pooled replay's threads count), adsb_host_replays, and the summary -- the step with scoring on
against the parent's with the parent's own min-max spread over its blocks (`gain_shown`: the gain is larger than that
spread), and whether the step with scoring off lies inside that spread (`off_inside_parent_spread`).
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
N_BUF, PER_BLOCK, DEPTH = 512, 20, 4


def load(path):
    from dump1090_rs_amd import _lib
    L = _lib.lib() if path is None else C.CDLL(str(path))
    vp, sz = C.c_void_p, C.c_size_t
    L.adsb_create.argtypes = [C.POINTER(vp), C.c_int, sz]
    L.adsb_set_receivers.argtypes = [vp, C.c_uint32]
    L.adsb_submit_iq_device_rx.argtypes = [vp, vp, sz, vp]
    L.adsb_demod_iq_device_rx.argtypes = [vp, vp, sz, vp, vp, sz, C.POINTER(sz)]
    L.adsb_collect.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.adsb_icao_flush.argtypes = [vp]
    L.adsb_host_replays.argtypes = [vp]
    L.adsb_host_replays.restype = C.c_uint64
    L.adsb_destroy.argtypes = [vp]
    L.adsb_destroy.restype = None
    L.adsb_version.restype = C.c_char_p
    return L


def as_records(np, out, n):
    """the messages as a structured array, the bytes behind a short message's seven masked"""
    dt = np.dtype([("msg", "u1", 14), ("len", "u1"), ("try_phase", "u1"), ("score", "<i4"), ("j", "<u4"), ("chunk", "<u8"),
                   ("signal_level", "<f8")])
    a = np.frombuffer(out, dtype=dt, count=n).copy()
    a["msg"][a["len"] == 7, 7:] = 0
    return a


def run(args, n_receivers):
    import numpy as np
    import torch
    from dump1090_rs_amd import synth
    from dump1090_rs_amd._lib import AdsbMsg
    from tests import receivers_support as RS
    n = N_BUF * CHUNK
    d = synth.make_iq_torch(n, n_bursts=5000, seed=synth.SEED_DEFAULT + 5, device="cuda")
    torch.cuda.synchronize()
    m = (np.arange(N_BUF) % n_receivers).astype(np.uint32)
    want = RS.Model(n_receivers).feed(d.cpu().numpy(), m)
    cap = 1 << 16
    out, cnt = (AdsbMsg * cap)(), C.c_size_t()
    parent, this = load(args.parent_lib), load(None)
    libs = {name: (parent if name.startswith("parent") else this) for name in args.order.split(",")}
    assert {"parent", "scoring_on", "scoring_off"} <= set(libs), args.order
    ctx, reference, ok = {}, None, {}
    for name, L in libs.items():
        h = C.c_void_p()
        assert L.adsb_create(C.byref(h), 0, N_BUF) == 0
        assert L.adsb_set_receivers(h, n_receivers) == 0
        if name == "scoring_on" or (args.parent_scoring and name.startswith("parent")):
            assert L.adsb_set_receiver_scoring(h, 1) == 0
        ctx[name] = h
        # into dense mode (one blocking pass), and the reference list: equal to the model, message by message
        assert L.adsb_demod_iq_device_rx(h, C.c_void_p(d.data_ptr()), n, m.ctypes.data, out, cap, C.byref(cnt)) == 0
        got = [RS.key_of(x.chunk, x.j, x.try_phase, x.score, bytes(x.msg), x.len, x.signal_level) for x in out[: cnt.value]]
        ok[name] = got == want
        if reference is None:
            reference = as_records(np, out, cnt.value)

    def block(name):
        L, h = libs[name], ctx[name]
        torch.cuda.synchronize()
        good, collected = True, 0
        cpu0, t0 = time.process_time(), time.perf_counter()
        for k in range(PER_BLOCK + DEPTH - 1):
            if k < PER_BLOCK:
                assert L.adsb_icao_flush(h) == 0
                assert L.adsb_submit_iq_device_rx(h, C.c_void_p(d.data_ptr()), n, m.ctypes.data) == 0
            if k >= DEPTH - 1:
                assert L.adsb_collect(h, out, cap, C.byref(cnt)) == 0
                collected += 1
                # (the comparison is the consumer's work and is inside the step for all three alike)
                a = as_records(np, out, cnt.value)
                good = good and len(a) == len(reference) and bool((a == reference).all())
        torch.cuda.synchronize()
        dt, cpu = time.perf_counter() - t0, time.process_time() - cpu0
        assert collected == PER_BLOCK
        return 1e3 * dt / PER_BLOCK, 1e6 * cpu / PER_BLOCK, good

    res = {name: {"ms_per_step_blocks": [], "host_cpu_us_per_pass_blocks": []} for name in libs}
    before = {name: int(L.adsb_host_replays(ctx[name])) for name, L in libs.items()}
    for b in range(args.blocks + 1):
        for name in libs:
            ms, cpu, good = block(name)
            ok[name] = ok[name] and good
            if b:   # (block 0: warm-up -- the clock ramp, the first rebuild of the keyed set)
                res[name]["ms_per_step_blocks"].append(round(ms, 4))
                res[name]["host_cpu_us_per_pass_blocks"].append(round(cpu, 1))
    for name, L in libs.items():
        r = res[name]
        r["ms_per_step"] = round(statistics.median(r["ms_per_step_blocks"]), 4)
        r["host_cpu_us_per_pass"] = round(statistics.median(r["host_cpu_us_per_pass_blocks"]), 1)
        r["host_replays"] = int(L.adsb_host_replays(ctx[name])) - before[name]
        r["parity"] = ok[name]
        r["lib"] = L.adsb_version().decode()
        L.adsb_destroy(ctx[name])
    p = res["parent"]["ms_per_step_blocks"]
    spread = max(p) - min(p)
    gain = res["parent"]["ms_per_step"] - res["scoring_on"]["ms_per_step"]
    rec = {"tool": "receivers_scored_rate", "label": args.label, "receivers": n_receivers, "buffers": N_BUF, "messages": len(want),
           "steps_per_block": PER_BLOCK, "in_flight": DEPTH, **res,
           "order": list(libs), "parent_spread_ms": [min(p), max(p)], "gain_ms": round(gain, 4), "gain_shown": gain > spread,
           "off_inside_parent_spread": min(p) <= res["scoring_off"]["ms_per_step"] <= max(p),
           "parent_scoring": args.parent_scoring, "on_inside_parent_spread": min(p) <= res["scoring_on"]["ms_per_step"] <= max(p)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        Path(args.out).mkdir(parents=True, exist_ok=True)
        with open(Path(args.out) / "receivers_scored_rate.jsonl", "a") as f:
            f.write(line + "\n")
    return all(ok.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libadsb_hip.so, built on this box")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--order", default="parent,scoring_on,scoring_off",
                    help="the contexts in the order they are created and take their turns; `parent_again`: a second context of "
                         "the parent's library (what two contexts of ONE library differ by, by their place alone)")
    ap.add_argument("--parent-scoring", action="store_true", help="scoring on in the parent's contexts too")
    ap.add_argument("--out")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    good = True
    for n_receivers in (512, 8):
        good = run(args, n_receivers) and good
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())

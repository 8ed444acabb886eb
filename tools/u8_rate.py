"""CU8 (8-bit RTL-SDR IQ) against CS16 on the same samples, each result checked against the CPU oracle on widen(b).

    python tools/u8_rate.py [--out DIR] [--rounds R] [--seconds S] [--legs resident,ring,host]

Three legs, each run for both formats in the same process, alternating CS16 / CU8 round by round (R rounds, the
median reported, the spread kept):
  resident  BASELINE config 2's step: icao_flush + one pass over 512 device-resident buffers (sparse sky), three
            passes in flight; ms per step, and the scan kernel's own time from its launch events (ms_scan);
  ring      BASELINE config 3: a pinned ring of 1, 4, 16 and 64 buffers per slot, filled once, submitted and
            collected for S seconds; Gsample/s of host-resident IQ demodulated;
  host      adsb_demod_iq(_u8) of one 131072-sample buffer from host memory, blocking; us per call.
The CU8 bytes are the CS16 samples quantised (b = clip(rint(x / 256 + 127.4))), the CS16 leg runs on widen(b) --
the very samples the CU8 leg means -- so the two legs demodulate identical input.  One JSON line per leg and
size goes to stdout and, with --out, is appended to DIR/u8_rate.jsonl (profiles/u8_rate.jsonl holds such a run).
"""
from __future__ import annotations

import argparse
import gc
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CHUNK = 131072


def t_soapy() -> np.ndarray:
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


T = t_soapy()


def quantise(iq: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def widen(b: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(T[b.reshape(-1, 2)])


def same(msgs, want) -> bool:
    return [(m.chunk, m.j, m.try_phase, m.score, m.msglen, m.msg.hex(), m.signal_level) for m in msgs] == \
           [(w["chunk"], w["j"], w["try_phase"], w["score"], w["len"], w["msg"].hex(), w["signal_level"]) for w in want]


def resident_leg(torch, orc_mod, rounds: int, steps: int) -> dict:
    from dump1090_rs_amd import Context, synth
    from dump1090_rs_amd._lib import AdsbMsg
    n = 512 * CHUNK
    b = [quantise(synth.make_iq_torch(n, n_bursts=64, seed=synth.SEED_DEFAULT + k, device="cuda").cpu().numpy())
         for k in range(2)]
    d8 = [torch.from_numpy(x).cuda() for x in b]
    d16 = [torch.from_numpy(widen(x)).cuda() for x in b]
    torch.cuda.synchronize()
    cap = 1 << 20
    out = (AdsbMsg * cap)()
    ctx = Context(0, 512)
    depth = 3
    # parity: one step of each format against the oracle on the widened samples
    want, _ = orc_mod.Oracle().demod_iq(widen(b[0]), cap=cap)
    ctx.icao_flush()
    p16 = same(ctx.demod_iq_device(d16[0].data_ptr(), n, cap=cap), want)
    ctx.icao_flush()
    p8 = same(ctx.demod_iq_device_u8(d8[0].data_ptr(), n, cap=cap), want)

    def run(fmt: str, count: int):
        submit = ctx.submit_iq_device_u8 if fmt == "cu8" else ctx.submit_iq_device
        bufs = d8 if fmt == "cu8" else d16
        scan = 0.0
        for i in range(count):
            ctx.icao_flush()
            submit(bufs[i % 2].data_ptr(), n)
            if i >= depth - 1:
                ctx.collect_raw(out, cap)
                scan += ctx.stats_raw().ms_scan
        for _ in range(min(count, depth - 1)):
            ctx.collect_raw(out, cap)
            scan += ctx.stats_raw().ms_scan
        return scan / count

    res = {"cs16": [], "cu8": []}
    scans = {"cs16": [], "cu8": []}
    for fmt in ("cs16", "cu8"):
        run(fmt, 20)   # warm-up
    gc.collect()
    gc.disable()
    for _ in range(rounds):
        for fmt in ("cs16", "cu8"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scans[fmt].append(run(fmt, steps))
            torch.cuda.synchronize()
            res[fmt].append((time.perf_counter() - t0) / steps * 1e3)
    gc.enable()
    ctx.close()
    m16, m8 = statistics.median(res["cs16"]), statistics.median(res["cu8"])
    return {"leg": "resident", "buffers": 512, "steps": steps, "rounds": rounds,
            "cs16_ms_per_step": round(m16, 4), "cu8_ms_per_step": round(m8, 4),
            "cs16_ms_range": [round(min(res["cs16"]), 4), round(max(res["cs16"]), 4)],
            "cu8_ms_range": [round(min(res["cu8"]), 4), round(max(res["cu8"]), 4)],
            "cs16_scan_ms": round(statistics.median(scans["cs16"]), 4), "cu8_scan_ms": round(statistics.median(scans["cu8"]), 4),
            "cu8_over_cs16": round(m8 / m16, 4), "cs16_Gsample_s": round(n / m16 / 1e6, 2), "cu8_Gsample_s": round(n / m8 / 1e6, 2),
            "parity_cs16": p16, "parity_cu8": p8}


def ring_leg(orc_mod, chunks: int, rounds: int, seconds: float) -> dict:
    from dump1090_rs_amd import Context, synth
    from dump1090_rs_amd._lib import AdsbMsg
    n = chunks * CHUNK
    cap = 1 << 18
    out = (AdsbMsg * cap)()
    ctxs, depth, parity = {}, {}, {}
    for fmt in ("cs16", "cu8"):
        ctx = Context(0, chunks)
        (ctx.ring_create_u8 if fmt == "cu8" else ctx.ring_create)(n)
        ctx.icao_flush()
        slots = ctx.max_in_flight()
        depth[fmt] = 3 if slots == 4 else slots
        orc = orc_mod.Oracle()
        ok = True
        for k in range(slots):   # fill every pinned slot once, each pass checked against the oracle (one stream)
            b = quantise(synth.make_iq(n, n_bursts=max(1, 64 * chunks // 512), seed=synth.SEED_DEFAULT + k))
            if fmt == "cu8":
                ctx.ring_acquire_u8()[:] = b
            else:
                ctx.ring_acquire()[:] = widen(b)
            ctx.ring_submit(n)
            ok = ok and same(ctx.collect(cap=cap), orc.demod_iq(widen(b), cap=cap)[0])
        parity[fmt] = ok
        ctx.set_profiling(0 if slots != 4 else 1)
        ctxs[fmt] = ctx

    def loop(fmt: str, secs: float):
        ctx, dp = ctxs[fmt], depth[fmt]
        acquire = ctx._L.adsb_ring_acquire_u8 if fmt == "cu8" else ctx._L.adsb_ring_acquire
        import ctypes as C
        ptr, capn = C.c_void_p(), C.c_size_t()
        i = done = 0
        t0 = time.perf_counter()
        while True:
            acquire(ctx._h, C.byref(ptr), C.byref(capn))
            ctx.ring_submit(n)
            i += 1
            if i - done >= dp:
                ctx.collect_raw(out, cap)
                done += 1
            if i >= 8 and time.perf_counter() - t0 >= secs:
                break
        while done < i:
            ctx.collect_raw(out, cap)
            done += 1
        return n * i / (time.perf_counter() - t0) / 1e9

    for fmt in ("cs16", "cu8"):
        loop(fmt, 0.3)   # warm-up
    rates = {"cs16": [], "cu8": []}
    gc.collect()
    gc.disable()
    for _ in range(rounds):
        for fmt in ("cs16", "cu8"):
            rates[fmt].append(loop(fmt, seconds))
    gc.enable()
    for c in ctxs.values():
        c.close()
    r16, r8 = statistics.median(rates["cs16"]), statistics.median(rates["cu8"])
    return {"leg": "ring", "buffers_per_slot": chunks, "depth": depth["cu8"], "rounds": rounds, "seconds": seconds,
            "cs16_Gsample_s": round(r16, 3), "cu8_Gsample_s": round(r8, 3),
            "cs16_range": [round(min(rates["cs16"]), 3), round(max(rates["cs16"]), 3)],
            "cu8_range": [round(min(rates["cu8"]), 3), round(max(rates["cu8"]), 3)],
            "cu8_over_cs16": round(r8 / r16, 4), "cs16_link_GBps": round(4 * r16, 2), "cu8_link_GBps": round(2 * r8, 2),
            "parity_cs16": parity["cs16"], "parity_cu8": parity["cu8"]}


def host_leg(orc_mod, rounds: int, calls: int) -> dict:
    from dump1090_rs_amd import Context, synth
    b = quantise(synth.make_iq(CHUNK, n_bursts=8, seed=synth.SEED_DEFAULT))
    w = widen(b)
    want, _ = orc_mod.Oracle().demod_iq(w)
    ctx = Context(0, 1)
    ctx.icao_flush()
    p16 = same(ctx.demod_iq(w), want)
    ctx.icao_flush()
    p8 = same(ctx.demod_iq_u8(b), want)
    fns = {"cs16": lambda: ctx.demod_iq(w), "cu8": lambda: ctx.demod_iq_u8(b)}
    for f in fns.values():
        for _ in range(200):
            f()
    res = {"cs16": [], "cu8": []}
    gc.collect()
    gc.disable()
    for _ in range(rounds):
        for fmt, f in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            res[fmt].append((time.perf_counter() - t0) / calls * 1e6)
    gc.enable()
    ctx.close()
    m16, m8 = statistics.median(res["cs16"]), statistics.median(res["cu8"])
    return {"leg": "host_buffer", "samples": CHUNK, "calls": calls, "rounds": rounds,
            "cs16_us_per_call": round(m16, 2), "cu8_us_per_call": round(m8, 2),
            "cs16_us_range": [round(min(res["cs16"]), 2), round(max(res["cs16"]), 2)],
            "cu8_us_range": [round(min(res["cu8"]), 2), round(max(res["cu8"]), 2)],
            "cu8_over_cs16": round(m8 / m16, 4), "parity_cs16": p16, "parity_cu8": p8}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="directory that u8_rate.jsonl is appended to (default: stdout only)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--legs", default="resident,ring,host")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("u8_rate: no GPU", file=sys.stderr)
        return 2
    from dump1090_rs_amd import _lib
    from oracle import binding
    binding.build()
    lines = []
    legs = args.legs.split(",")
    if "resident" in legs:
        lines.append(resident_leg(torch, binding, args.rounds, args.steps))
    if "ring" in legs:
        for chunks in (1, 4, 16, 64):
            lines.append(ring_leg(binding, chunks, args.rounds, args.seconds))
    if "host" in legs:
        lines.append(host_leg(binding, args.rounds, 500))
    ok = True
    text = []
    for ln in lines:
        ln["library"] = _lib.lib().adsb_version().decode()
        ln["device"] = torch.cuda.get_device_name(0)
        text.append(json.dumps(ln))
        print(text[-1], flush=True)
        ok = ok and ln["parity_cs16"] and ln["parity_cu8"]
    if args.out:
        out = Path(args.out)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "u8_rate.jsonl", "a") as f:
            f.write("".join(t + "\n" for t in text))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

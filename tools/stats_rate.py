"""What the signal statistics (adsb_set_signal_stats) cost: the mode on against off on the same samples, in one process,
the modes alternating round by round; every leg's records checked against the restatement over the CPU oracle's
magnitudes (tests/signal_support.py) and its frames against the CPU oracle's own demodulation of the same samples.

    python tools/stats_rate.py [--out DIR] [--rounds R] [--seconds S] [--label TEXT] [--only SHAPE] [--kernel-only FMT]

Shapes (R rounds, the median reported, the spread of the rounds kept beside it):
  resident   icao_flush + one blocking pass over 512 device-resident buffers, sparse sky (64 bursts); ms per step;
  pipelined  the same step in a steady pipeline, four passes in flight, blocks of 20 steps between fences, the modes
             alternating block by block; ms per step (median of the blocks, their spread);
  config1    adsb_demod_iq of the one 131072-sample capture of BASELINE config 1 from host memory; us per call;
  ring       the pinned ring at 1 and at 16 buffers per slot, CS16 and CU8, submitted and collected for S seconds;
             Gsample/s.  (The one-buffer ring is where the second read of the slot over the link shows.)
--kernel-only cs16|cu8 runs nothing but 30 blocking 512-buffer passes with the mode on: the run to put under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters) for k_signal_stats' own duration.
--parent-lib PATH is "off means off": the pipelined shape with the mode off on this build and on the library at PATH (the
parent commit's, built on the same box), both loaded into this one process, alternating in blocks of 20 steps; the
acceptance margin is the parent's own block-to-block spread, and this build's median has to lie inside it
(`inside_parent_spread`).  --off-only runs the pipelined shape with the mode off on this build alone.
One JSON line per shape and mode goes to stdout and, with --out, is appended to DIR/stats_rate.jsonl.
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
MODES = (False, True)
NAMES = {False: "off", True: "on"}


def keys(msgs):
    return [(m.buffer(), int(m.score), int(m.j), int(m.try_phase), int(m.chunk), float(m.signal_level)) for m in msgs]


def widen(raw):
    """CU8 bytes -> the CS16 they mean under a new context's table (include/adsb_hip.h: T_soapy); CS16 as it is."""
    import numpy as np
    if raw.dtype != np.uint8:
        return raw
    x = np.arange(256, dtype=np.float32)
    t = np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)
    return np.ascontiguousarray(t[raw.reshape(-1, 2)])


def quantise(iq):
    import numpy as np
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


def restated(raw):
    from oracle import binding
    from dump1090_rs_amd.context import SIGNAL_STATS_DTYPE
    from tests import signal_support as ss
    return ss.restated(binding.Oracle(), widen(raw), raw, SIGNAL_STATS_DTYPE)


def oracle_frames(raw):
    """What the CPU oracle makes of the call, as keys() lists it."""
    from oracle import binding
    want, _ = binding.Oracle().demod_iq(widen(raw), cap=1 << 20, threads=16)
    return [(w["buffer"], int(w["score"]), int(w["j"]), int(w["try_phase"]), int(w["chunk"]), float(w["signal_level"])) for w in want]


def same_records(got, want) -> bool:
    import numpy as np
    return len(got) == len(want) and all(np.array_equal(got[n], want[n]) for n in want.dtype.names)


def has_mode(c) -> bool:
    return hasattr(c._L, "adsb_set_signal_stats")


def resident(torch, rounds):
    from dump1090_rs_amd import Context, synth
    n = 512 * CHUNK
    d = synth.make_iq_torch(n, n_bursts=64, device="cuda")
    want, want_frames = restated(d.cpu().numpy()), oracle_frames(d.cpu().numpy())
    torch.cuda.synchronize()
    out = {}
    with Context(0, 512) as c:
        frames, ok = {}, {}
        for on in MODES:
            c.set_signal_stats(on)
            c.icao_flush()
            frames[on] = keys(c.demod_iq_device(d.data_ptr(), n, cap=1 << 20))
            ok[on] = same_records(c.signal_stats(), want if on else want[:0]) and frames[on] == want_frames
        t = {m: [] for m in MODES}
        for _ in range(rounds):
            for on in MODES:
                c.set_signal_stats(on)
                c.icao_flush()
                c.demod_iq_device(d.data_ptr(), n, cap=1 << 20)
                t0 = time.perf_counter()
                for _ in range(10):
                    c.icao_flush()
                    c.demod_iq_device(d.data_ptr(), n, cap=1 << 20)
                t[on].append((time.perf_counter() - t0) / 10 * 1e3)
        for on in MODES:
            out[on] = {"ms_per_step": statistics.median(t[on]), "spread": [min(t[on]), max(t[on])], "parity": ok[on]}
    return out


def pipelined(torch, modes=MODES, blocks=11, per_block=20):
    import ctypes as C
    from dump1090_rs_amd import Context, synth
    from dump1090_rs_amd._lib import AdsbMsg
    n = 512 * CHUNK
    d = synth.make_iq_torch(n, n_bursts=64, device="cuda")
    torch.cuda.synchronize()
    cap = 1 << 14
    outs = [(AdsbMsg * cap)() for _ in range(per_block)]
    counts = [C.c_size_t() for _ in range(per_block)]
    out = {}
    with Context(0, 512) as c:
        L, h, ptr = c._L, c._h, C.c_void_p(d.data_ptr())
        depth = c.max_in_flight()
        want_rec = restated(d.cpu().numpy()) if True in modes else None

        def block(check_records=False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            done, good = 0, True
            for k in range(per_block):
                if k >= depth:
                    assert L.adsb_collect(h, outs[done], cap, C.byref(counts[done])) == 0
                    done += 1
                assert L.adsb_icao_flush(h) == 0 and L.adsb_submit_iq_device(h, ptr, n) == 0
            while done < per_block:
                assert L.adsb_collect(h, outs[done], cap, C.byref(counts[done])) == 0
                done += 1
            dt = time.perf_counter() - t0
            if check_records:
                good = same_records(c.signal_stats(), want_rec)
            return dt, good

        t, ok, want = {m: [] for m in modes}, {m: True for m in modes}, None
        c.icao_flush()      # every step's list is the oracle's (each step starts from an empty filter)
        oracle_ok = keys(c.demod_iq_device(d.data_ptr(), n, cap=1 << 20)) == oracle_frames(d.cpu().numpy())
        want = C.string_at(c._out_buf, c.stats()["n_messages"] * C.sizeof(AdsbMsg))
        ok = {m: oracle_ok for m in modes}
        for b in range(blocks):
            for on in modes:
                if has_mode(c):
                    c.set_signal_stats(on)
                dt, good = block(check_records=on)
                ok[on] = ok[on] and good
                if b:
                    t[on].append(dt / per_block * 1e3)
                for k in range(per_block):
                    got = C.string_at(outs[k], counts[k].value * C.sizeof(AdsbMsg))
                    ok[on] = ok[on] and got == want
        for on in modes:
            out[on] = {"ms_per_step": statistics.median(t[on]), "spread": [min(t[on]), max(t[on])],
                       "blocks": [round(x, 4) for x in t[on]], "steps": per_block * len(t[on]), "in_flight": depth, "parity": ok[on]}
    return out


def two_builds(torch, parent_path, blocks=11, per_block=20):
    """The pipelined sparse step, mode off, on this build and on the library at parent_path in one process, alternating
    block by block.  Both through the bare C ABI; every collected list compared with the oracle's."""
    import ctypes as C
    from dump1090_rs_amd import synth, _lib
    from dump1090_rs_amd._lib import AdsbMsg
    n = 512 * CHUNK
    d = synth.make_iq_torch(n, n_bursts=64, device="cuda")
    want_frames = oracle_frames(d.cpu().numpy())
    torch.cuda.synchronize()
    cap = 1 << 14
    outs = [(AdsbMsg * cap)() for _ in range(per_block)]
    counts = [C.c_size_t() for _ in range(per_block)]
    libs = {"parent": C.CDLL(str(parent_path)), "this": _lib.lib()}
    ctx, ver = {}, {}
    for name, L in libs.items():
        L.adsb_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_size_t]
        L.adsb_submit_iq_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.adsb_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.adsb_icao_flush.argtypes = [C.c_void_p]
        L.adsb_destroy.argtypes = [C.c_void_p]
        L.adsb_destroy.restype = None
        L.adsb_version.restype = C.c_char_p
        h = C.c_void_p()
        assert L.adsb_create(C.byref(h), 0, 512) == 0
        ctx[name], ver[name] = h, L.adsb_version().decode()
    ptr, depth = C.c_void_p(d.data_ptr()), 4

    def block(name):
        L, h = libs[name], ctx[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = 0
        for k in range(per_block):
            if k >= depth:
                assert L.adsb_collect(h, outs[done], cap, C.byref(counts[done])) == 0
                done += 1
            assert L.adsb_icao_flush(h) == 0 and L.adsb_submit_iq_device(h, ptr, n) == 0
        while done < per_block:
            assert L.adsb_collect(h, outs[done], cap, C.byref(counts[done])) == 0
            done += 1
        dt = time.perf_counter() - t0
        good = True
        for k in range(per_block):
            m = outs[k]
            got = [(bytes(m[i].msg[: m[i].len]), int(m[i].score), int(m[i].j), int(m[i].try_phase), int(m[i].chunk),
                    float(m[i].signal_level)) for i in range(counts[k].value)]
            good = good and got == want_frames
        return dt, good

    t, ok = {k: [] for k in libs}, {k: True for k in libs}
    for b in range(blocks):
        for name in libs:
            dt, good = block(name)
            ok[name] = ok[name] and good
            if b:
                t[name].append(dt / per_block * 1e3)
    for name, L in libs.items():
        L.adsb_destroy(ctx[name])
    lo, hi = min(t["parent"]), max(t["parent"])
    out = []
    for name in libs:
        out.append({"shape": "pipelined_sparse_off", "library": name, "version": ver[name], "ms_per_step": statistics.median(t[name]),
                    "spread": [min(t[name]), max(t[name])], "blocks": [round(x, 4) for x in t[name]], "steps": per_block * len(t[name]),
                    "in_flight": depth, "parity": ok[name]})
    out[1]["inside_parent_spread"] = lo <= out[1]["ms_per_step"] <= hi
    return out


def config1(rounds):
    from dump1090_rs_amd import Context, utils
    fx = json.loads((ROOT / "tests/golden/reference_frames.json").read_text())["fixtures"][0]
    iq = utils.read_test_data(str(ROOT / "tests/golden" / fx["file"]))
    want, want_frames = restated(iq), oracle_frames(iq)
    out = {}
    with Context(0, 1) as c:
        frames, ok = {}, {}
        for on in MODES:
            c.set_signal_stats(on)
            c.icao_flush()
            frames[on] = keys(c.demod_iq(iq))
            ok[on] = same_records(c.signal_stats(), want if on else want[:0]) and frames[on] == want_frames
        t = {m: [] for m in MODES}
        for _ in range(rounds):
            for on in MODES:
                c.set_signal_stats(on)
                t0 = time.perf_counter()
                for _ in range(200):
                    c.icao_flush()
                    c.demod_iq(iq)
                t[on].append((time.perf_counter() - t0) / 200 * 1e6)
        for on in MODES:
            out[on] = {"us_per_call": statistics.median(t[on]), "spread": [min(t[on]), max(t[on])], "parity": ok[on]}
    return out


def ring(rounds, seconds, per, cu8):
    from dump1090_rs_amd import Context, synth
    iq = synth.make_iq(per * CHUNK, n_bursts=per * 4, seed=99)
    raw = quantise(iq) if cu8 else iq
    want, want_frames = restated(raw), oracle_frames(raw)
    out = {}
    with Context(0, per) as c:
        (c.ring_create_u8 if cu8 else c.ring_create)(per * CHUNK)
        acquire = c.ring_acquire_u8 if cu8 else c.ring_acquire
        depth = c.max_in_flight()
        frames, ok = {}, {}
        for on in MODES:   # (every slot gets the capture once: the timed loop below submits it as it stands)
            c.set_signal_stats(on)
            ok[on] = True
            for _ in range(depth):
                c.icao_flush()
                acquire()[:] = raw
                c.ring_submit(len(raw))
                frames[on] = keys(c.collect())
                ok[on] = ok[on] and same_records(c.signal_stats(), want if on else want[:0]) and frames[on] == want_frames
        rate = {m: [] for m in MODES}
        for _ in range(rounds):
            for on in MODES:
                c.set_signal_stats(on)
                c.icao_flush()
                done, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < seconds:
                    if c.pending() == depth:
                        c.collect()
                        done += 1
                    acquire()
                    c.ring_submit(len(raw))
                while c.pending():
                    c.collect()
                    done += 1
                rate[on].append(done * len(raw) / (time.perf_counter() - t0) / 1e9)
        for on in MODES:
            out[on] = {"gsample_per_s": statistics.median(rate[on]), "spread": [min(rate[on]), max(rate[on])], "parity": ok[on]}
    return out


def kernel_only(torch, fmt):
    from dump1090_rs_amd import Context, synth
    n = 512 * CHUNK
    iq = synth.make_iq_torch(n, n_bursts=64, device="cuda")
    d = torch.from_numpy(quantise(iq.cpu().numpy())).cuda() if fmt == "cu8" else iq
    torch.cuda.synchronize()
    with Context(0, 512) as c:
        c.set_signal_stats(True)
        run = c.demod_iq_device_u8 if fmt == "cu8" else c.demod_iq_device
        for _ in range(30):
            c.icao_flush()
            run(d.data_ptr(), n, cap=1 << 20)
        return len(c.signal_stats()) == 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    ap.add_argument("--only", default=None, help="one shape: resident, pipelined, config1, ring")
    ap.add_argument("--off-only", action="store_true", help="the pipelined shape with the mode off alone (any build)")
    ap.add_argument("--kernel-only", default=None, choices=("cs16", "cu8"))
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libadsb_hip.so: off means off, both builds in one run")
    a = ap.parse_args()
    import torch
    if a.kernel_only:
        return 0 if kernel_only(torch, a.kernel_only) else 1
    lines = []
    if a.parent_lib:
        lines += two_builds(torch, a.parent_lib)
    elif a.off_only:
        res = pipelined(torch, modes=(False,))
        lines.append({"shape": "pipelined_sparse", "stats": "off", **res[False]})
    else:
        shapes = [("resident_sparse", lambda: resident(torch, a.rounds)), ("pipelined_sparse", lambda: pipelined(torch)),
                  ("config1", lambda: config1(a.rounds))]
        shapes += [("ring%d_%s" % (per, "cu8" if cu8 else "cs16"), lambda per=per, cu8=cu8: ring(a.rounds, a.seconds, per, cu8))
                   for per in (1, 16) for cu8 in (False, True)]
        for shape, run in shapes:
            if a.only and not shape.startswith(a.only):
                continue
            res = run()
            for on in MODES:
                lines.append({"shape": shape, "stats": NAMES[on], **res[on]})
            figure = next(k for k in res[True] if k not in ("spread", "parity", "blocks", "steps", "in_flight"))
            ratio = res[True][figure] / res[False][figure]
            lines.append({"shape": shape, "stats": "on/off", "ratio": ratio if "per" in figure and "gsample" not in figure else 1.0 / ratio,
                          "of": "time", "off_spread": res[False]["spread"], "parity": True})
    if a.label:
        lines = [{**ln, "build": a.label} for ln in lines]
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "stats_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

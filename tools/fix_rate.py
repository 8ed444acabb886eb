"""Single-bit (ADSB_FIX_1BIT) and two-bit (ADSB_FIX_2BIT) repair against no repair on the same samples, each result
checked against the CPU restatement of its mode (tests/fix_restatement.c, tests/fix2_restatement.c over the oracle).

    python tools/fix_rate.py [--out DIR] [--rounds R] [--seconds S] [--noise-only] [--pipelined-only] [--label TEXT]

Shapes, each run with correction off, 1bit and 2bit in the same process, alternating round by round (R rounds, the
median reported, the spread kept):
  resident  BASELINE config 2's step: icao_flush + one blocking pass over 512 device-resident buffers, sparse (64
            bursts) and busy (5000 bursts); ms per step;
  config1   adsb_demod_iq of the one 131072-sample capture of config 1 from host memory, blocking; us per call;
  ring      a pinned CS16 ring of 16 buffers per slot, filled once, submitted and collected for S seconds; Gsample/s.
  noise     (2bit only) 64 buffers of noise: the trials the device turned into two-bit hits per buffer (records of
            mode 3 minus those of mode 1) next to the expectation, 5671 / 2^24 of the failed DF17/18 trials, and the
            exact count (the oracle's trials whose residual is a pair syndrome).
  pipelined BASELINE config 5's step in a steady pipeline: icao_flush + adsb_submit_iq_device of 512 resident buffers
            with 5000 bursts, four passes in flight, collected in order through the C ABI into preallocated arrays; blocks
            of 20 steps between fences, the three modes alternating block by block, at least 200 steps a mode; every
            collected list compared byte for byte (outside the timed region) with one that equals the restatement; ms per
            step (median of the blocks, their spread) and how many of the passes the host scored (adsb_host_replays).
            --label names the build (the commit) in the line, so that two builds run on one box can be told apart.
One JSON line per shape and mode goes to stdout and, with --out, is appended to DIR/fix_rate.jsonl.
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
MODES = (0, 1, 3)
NAMES = {0: "none", 1: "1bit", 3: "2bit"}


def keys(msgs):
    return [(m.buffer(), int(m.score), int(m.j), int(m.try_phase), int(m.chunk), float(m.signal_level)) for m in msgs]


def parity(iq, mode, got) -> bool:
    from tests import fix2_support as f2
    return keys(got) == f2.Restated(mode).demod_iq(iq)


def resident(torch, rounds, n_bursts):
    from dump1090_rs_amd import Context, synth
    n = 512 * CHUNK
    d = synth.make_iq_torch(n, n_bursts=n_bursts, device="cuda")
    iq = d.cpu().numpy()
    torch.cuda.synchronize()
    out = {}
    with Context(0, 512) as c:
        ok = {}
        for mode in MODES:
            c.set_error_correction(mode)
            c.icao_flush()
            ok[mode] = parity(iq, mode, c.demod_iq_device(d.data_ptr(), n, cap=1 << 20))
        t = {m: [] for m in MODES}
        for r in range(rounds):
            for mode in MODES:
                c.set_error_correction(mode)
                c.icao_flush()
                c.demod_iq_device(d.data_ptr(), n, cap=1 << 20)   # warm-up: the stream's density
                t0 = time.perf_counter()
                for _ in range(10):
                    c.icao_flush()
                    c.demod_iq_device(d.data_ptr(), n, cap=1 << 20)
                t[mode].append((time.perf_counter() - t0) / 10 * 1e3)
        for mode in MODES:
            out[mode] = {"ms_per_step": statistics.median(t[mode]), "spread": [min(t[mode]), max(t[mode])], "parity": ok[mode]}
    return out


def config1(rounds):
    from dump1090_rs_amd import Context, utils
    fx = json.loads((ROOT / "tests/golden/reference_frames.json").read_text())["fixtures"][0]
    iq = utils.read_test_data(str(ROOT / "tests/golden" / fx["file"]))
    out = {}
    with Context(0, 1) as c:
        ok = {}
        for mode in MODES:
            c.set_error_correction(mode)
            c.icao_flush()
            ok[mode] = parity(iq, mode, c.demod_iq(iq))
        t = {m: [] for m in MODES}
        for r in range(rounds):
            for mode in MODES:
                c.set_error_correction(mode)
                t0 = time.perf_counter()
                for _ in range(200):
                    c.icao_flush()
                    c.demod_iq(iq)
                t[mode].append((time.perf_counter() - t0) / 200 * 1e6)
        for mode in MODES:
            out[mode] = {"us_per_call": statistics.median(t[mode]), "spread": [min(t[mode]), max(t[mode])], "parity": ok[mode]}
    return out


def ring(rounds, seconds):
    from dump1090_rs_amd import Context, synth
    per = 16
    iq = synth.make_iq(per * CHUNK, n_bursts=per * 4, seed=99)
    out = {}
    with Context(0, per) as c:
        c.ring_create(per * CHUNK)
        depth = c.max_in_flight()
        ok = {}
        for mode in MODES:   # (every slot gets the capture once: the timed loop below submits it as it stands)
            c.set_error_correction(mode)
            for _ in range(depth):
                c.icao_flush()
                buf = c.ring_acquire()
                buf[:] = iq
                c.ring_submit(len(iq))
                ok[mode] = parity(iq, mode, c.collect()) and ok.get(mode, True)
        rate = {m: [] for m in MODES}
        for r in range(rounds):
            for mode in MODES:
                c.set_error_correction(mode)
                c.icao_flush()
                done, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < seconds:
                    if c.pending() == depth:
                        c.collect()
                        done += 1
                    c.ring_acquire()   # (the slot still holds the capture: the samples are the same every time)
                    c.ring_submit(len(iq))
                while c.pending():
                    c.collect()
                    done += 1
                rate[mode].append(done * len(iq) / (time.perf_counter() - t0) / 1e9)
        for mode in MODES:
            out[mode] = {"gsample_per_s": statistics.median(rate[mode]), "spread": [min(rate[mode]), max(rate[mode])],
                         "parity": ok[mode]}
    return out


def pipelined(torch, blocks=11, per_block=20, n_bursts=5000):
    import ctypes as C
    from dump1090_rs_amd import Context, synth
    from dump1090_rs_amd._lib import AdsbMsg
    from dump1090_rs_amd.context import ModeSMessage
    n = 512 * CHUNK
    d = synth.make_iq_torch(n, n_bursts=n_bursts, device="cuda")
    iq = d.cpu().numpy()
    torch.cuda.synchronize()
    cap = 1 << 14
    outs = [(AdsbMsg * cap)() for _ in range(per_block)]
    counts = [C.c_size_t() for _ in range(per_block)]
    out = {}
    with Context(0, 512) as c:
        L, h, ptr = c._L, c._h, C.c_void_p(d.data_ptr())
        depth = c.max_in_flight()

        def block():
            """per_block steps, `depth` in flight; seconds between the fences"""
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
            return time.perf_counter() - t0

        want, ok = {}, {}
        for mode in MODES:   # what every step of the mode must return: one list that equals the restatement
            c.set_error_correction(mode)
            c.icao_flush()
            got = c.demod_iq_device(d.data_ptr(), n, cap=1 << 20)
            ok[mode] = parity(iq, mode, got)
            block()      # (the first pass told the context how dense the stream is: from here on the steady pipeline)
            want[mode] = C.string_at(outs[per_block - 1], counts[per_block - 1].value * C.sizeof(AdsbMsg))
            m = outs[per_block - 1]
            last = [ModeSMessage(bytes(m[i].msg), int(m[i].len), float(m[i].signal_level), int(m[i].score), int(m[i].j),
                                 int(m[i].try_phase), int(m[i].chunk)) for i in range(counts[per_block - 1].value)]
            ok[mode] = ok[mode] and keys(last) == keys(got)
        t = {m: [] for m in MODES}
        replays = {m: 0 for m in MODES}
        for b in range(blocks):
            for mode in MODES:
                c.set_error_correction(mode)
                before = int(L.adsb_host_replays(h))
                dt = block()
                if b:    # (the first block of a mode: warm-up)
                    t[mode].append(dt / per_block * 1e3)
                    replays[mode] += int(L.adsb_host_replays(h)) - before
                for k in range(per_block):
                    ok[mode] = ok[mode] and C.string_at(outs[k], counts[k].value * C.sizeof(AdsbMsg)) == want[mode]
        for mode in MODES:
            out[mode] = {"ms_per_step": statistics.median(t[mode]), "spread": [min(t[mode]), max(t[mode])],
                         "blocks": [round(x, 4) for x in t[mode]], "steps": per_block * len(t[mode]), "in_flight": depth,
                         "host_scored_passes": replays[mode], "frames_per_step": len(want[mode]) // C.sizeof(AdsbMsg),
                         "parity": ok[mode]}
    return out


def noise(torch, n_buffers=64):
    import numpy as np
    from dump1090_rs_amd import Context, synth
    from oracle import binding
    from tests import fix2_support as f2
    iq = np.concatenate([synth.noise_numpy(CHUNK, 9000 + k) for k in range(n_buffers)])
    d = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    recs, ok = {}, True
    with Context(0, n_buffers) as c:
        for mode in (1, 3):
            c.set_error_correction(mode)
            c.icao_flush()
            got = c.demod_iq_device(d.data_ptr(), len(iq), cap=1 << 20)
            recs[mode] = c.stats()["n_records"]   # (adsb_stats: the counters of this call alone)
            ok = parity(iq, mode, got) and ok
    import ctypes as C
    pairs = (C.c_uint32 * 5671)()
    f2.restatement().fix2_pair_syndromes(pairs)
    pair_set = set(pairs)
    O = binding.lib()
    failed = exact = 0
    for k in range(n_buffers):
        _, tr = binding.all_trials(np.ascontiguousarray(iq[k * CHUNK:(k + 1) * CHUNK]), k)
        for m in tr["msg"]:
            if (m[0] >> 3) in (17, 18):
                r = O.orc_modes_checksum(bytes(m), 112)
                failed += r != 0
                exact += r in pair_set
    return {"two_bit_hits_per_buffer": (recs[3] - recs[1]) / n_buffers, "exact_per_buffer": exact / n_buffers,
            "two_bit_hits": recs[3] - recs[1], "exact": exact,
            "failed_df1718_per_buffer": failed / n_buffers, "expected_per_buffer": failed * 5671 / 2 ** 24 / n_buffers,
            "parity": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--noise-only", action="store_true", help="only the noise leg")
    ap.add_argument("--pipelined-only", action="store_true", help="only the pipelined dense leg")
    ap.add_argument("--label", default=None, help="what build this is (its commit), kept in every line")
    a = ap.parse_args()
    import torch
    lines = []
    shapes = () if a.noise_only else (("pipelined_5000", lambda: pipelined(torch)),) if a.pipelined_only else (("resident_sparse", lambda: resident(torch, a.rounds, 64)),
                                      ("resident_5000", lambda: resident(torch, a.rounds, 5000)),
                                      ("config1", lambda: config1(a.rounds)), ("ring16", lambda: ring(a.rounds, a.seconds)),
                                      ("pipelined_5000", lambda: pipelined(torch)))
    for shape, run in shapes:
        res = run()
        for mode in MODES:
            lines.append({"shape": shape, "fix": NAMES[mode], **res[mode]})
    if not a.pipelined_only:
        lines.append({"shape": "noise64", "fix": "2bit", **noise(torch)})
    if a.label:
        lines = [{**ln, "build": a.label} for ln in lines]
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        p = Path(a.out)
        p.mkdir(parents=True, exist_ok=True)
        with open(p / "fix_rate.jsonl", "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if all(ln["parity"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

"""What the tail of a sparse pass costs, from a `rocprofv3 --kernel-trace --output-format csv` run of `bench.py`
(pipelined or `--sync`; no counters in that run).

    python tools/tail_trace.py <..._kernel_trace.csv> [--csv OUT.csv] [--label TEXT]

From the dispatches' own begin / end stamps:
  - k_match and k_records, each beside a scan (its interval overlaps a k_scan_fast launch's) and alone: count, mean,
    median, min, max in us;
  - the steady pipeline: the median interval between consecutive scan launches' starts (the step), the tail kernels'
    busy time per step and its share of the step;
  - per timed block (a run of at least eight scans with no moment between them at which none is running): the time from
    the end of the block's last scan to the end of its last records kernel (the drain), from a scan's end to the start of
    the first match behind it (the hand-off over the `scanned` event, or the tail stream still busy with the pass before),
    and from a match's end to the records kernel behind it.
One line per figure: name, n, mean, median, min, max.  With --csv the same rows go to a file (profiles/tail_*.csv).
"""
from __future__ import annotations

import argparse
import bisect
import csv
import statistics
import sys


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    return rows


def kind(name):
    for k in ("k_scan_fast", "k_match_sparse", "k_match", "k_records", "k_order_prefix", "k_score", "k_emit"):
        if k in name:
            return k
    return None


def stat_row(name, xs):
    if not xs:
        return [name, 0, "", "", "", ""]
    return [name, len(xs), round(statistics.fmean(xs), 3), round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--csv", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    rows = load(a.trace)
    by = {}
    for s, e, n in rows:
        k = kind(n)
        if k:
            by.setdefault(k, []).append((s, e))
    scans = by.get("k_scan_fast", [])
    if not scans:
        print("no k_scan_fast launches in", a.trace, file=sys.stderr)
        return 1
    starts = [s for s, _ in scans]
    # a scan's launches overlap their neighbours by a tile round: the longest one still running decides "beside"
    max_len = max(e - s for s, e in scans)

    def beside(s, e):
        i = bisect.bisect_left(starts, s - max_len)
        while i < len(scans) and scans[i][0] < e:
            if scans[i][1] > s:
                return True
            i += 1
        return False

    out = []
    for k in ("k_match", "k_records"):
        d = {True: [], False: []}
        for s, e in by.get(k, []) + (by.get("k_match_sparse", []) if k == "k_match" else []):
            d[beside(s, e)].append((e - s) / 1e3)
        out.append(stat_row(k + "_beside_scan_us", d[True]))
        out.append(stat_row(k + "_alone_us", d[False]))
    out.append(stat_row("k_scan_fast_us", [(e - s) / 1e3 for s, e in scans]))
    gaps = [b - a0 for a0, b in zip(starts, starts[1:])]
    # blocks: runs of scans with no moment between them at which no scan is running (the fences between the timed blocks
    # drain the device); the short ones -- blocking calls, the ramp's single steps -- are left out
    blocks, cur, busy_until = [], [0], scans[0][1]
    for i in range(1, len(scans)):
        if scans[i][0] > busy_until:
            blocks.append(cur)
            cur = []
        cur.append(i)
        busy_until = max(busy_until, scans[i][1])
    blocks.append(cur)
    block_start = [scans[b[0]][0] for b in blocks] + [float("inf")]
    keep = [k for k, b in enumerate(blocks) if len(b) >= 8]
    inside = set(i for k in keep for i in blocks[k][1:])
    out.append(stat_row("scan_start_interval_us", [gaps[i - 1] / 1e3 for i in sorted(inside)]))
    match, recs = sorted(by.get("k_match", []) + by.get("k_match_sparse", [])), sorted(by.get("k_records", []))
    mstarts, rstarts = [s for s, _ in match], [s for s, _ in recs]
    busy, drain, handoff, m2r = [], [], [], []
    for k in keep:
        b = blocks[k]
        t0, t1 = scans[b[0]][0], max(scans[i][1] for i in b)
        tail = [(s, e) for s, e in match + recs if t0 <= s < block_start[k + 1]]
        if tail and t1 > t0:
            busy.append(sum(min(e, t1) - s for s, e in tail if s < t1) / (t1 - t0))
            drain.append((max(e for _, e in tail) - t1) / 1e3)
        for i in b:
            j = bisect.bisect_left(mstarts, scans[i][1])   # the first match not before this scan's end
            if j < len(match) and match[j][0] < block_start[k + 1]:
                handoff.append((match[j][0] - scans[i][1]) / 1e3)
                r = bisect.bisect_left(rstarts, match[j][1])
                if r < len(recs) and recs[r][0] < block_start[k + 1]:
                    m2r.append((recs[r][0] - match[j][1]) / 1e3)
    out.append(stat_row("tail_busy_share_of_block", busy))
    out.append(stat_row("drain_last_scan_end_to_last_records_end_us", drain))
    out.append(stat_row("scan_end_to_match_start_us", handoff))
    out.append(stat_row("match_end_to_records_start_us", m2r))
    head = ["figure", "n", "mean", "median", "min", "max"]
    for r in [head] + out:
        print(",".join(str(x) for x in r))
    if a.csv:
        with open(a.csv, "w", newline="") as f:
            w = csv.writer(f)
            if a.label:
                w.writerow(["# " + a.label])
            w.writerow(head)
            w.writerows(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

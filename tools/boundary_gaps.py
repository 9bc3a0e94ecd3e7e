#!/usr/bin/env python3
"""usage: tools/boundary_gaps.py <kernel_trace.csv> [--traffic profiles/traffic_c3_bf16.json] [--min-steps 20]

What the kernel boundaries of a training step cost, family by family, from ONE `rocprofv3 --kernel-trace` run of
`python bench.py --steps 50 --warmup 10` (a run of its own: no counters, no other tracing domain, the program behind `--`).

The trace is cut into steps at the optimizer launch (the last launch of a step).  Steps whose launch sequence is the commonest one are
kept (warm-up and capture steps launch the same kernels, the other legs of a run do not).  For every launch of a kept step:
    duration = its own end - begin
    gap      = the NEXT launch's begin - its end: the boundary BEHIND this kernel, the one its dirty bytes would lengthen
Per family the table gives launches per step, the per-launch duration and gap (mean over the family's launches of a step, then the median
over the steps), their per-step sums, and the bytes one launch of the family writes (WRITE_SIZE of tools/traffic.sh's pass, calibrated
there; "-" without a traffic file, "stale" marks one recorded for other kernel sources).  The gap behind the optimizer launch runs into
the next step's host work and is listed apart."""
import argparse
import collections
import csv
import json
import os
import re
import statistics
import sys


def family(name):
    """Kernel family of a (demangled) kernel name: ring GEMMs by tile, everything else by the kernel's bare name."""
    n = name.replace("void ", "").replace("(anonymous namespace)::", "")
    m = re.search(r"m2f_gemm16_ring_kernel<(\d+), (\d+), \d+, ([^,>]+)", n)
    if m:
        table = m.group(3).strip() in ("true", "(bool)1", "1")
        return f"ring {m.group(1)}x{m.group(2)}" + (" table (weight gradients)" if table else "")
    n = re.split(r"[<(]", n, maxsplit=1)[0]
    return n[4:] if n.startswith("m2f_") else n


def written_bytes(path):
    """family -> bytes written per launch, from tools/traffic.sh's JSON; (table, stale)"""
    if not path or not os.path.exists(path):
        return {}, False
    d = json.load(open(path))
    cal = (d.get("calibration_bytes_per_count") or {}).get("WRITE_SIZE") or 0.0
    agg = collections.defaultdict(lambda: [0.0, 0])
    for k, v in (d.get("by_kernel_raw") or {}).get("WRITE_SIZE", {}).items():
        f = family(k)
        agg[f][0] += v["sum"] * cal
        agg[f][1] += v["n"]
    stale = False
    try:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
        import bench
        stale = d.get("source_hash") != bench.source_hash()
    except Exception:
        stale = True
    return {f: s / n for f, (s, n) in agg.items() if n}, stale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--traffic", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "traffic_c3_bf16.json"))
    ap.add_argument("--min-steps", type=int, default=20)
    a = ap.parse_args()
    ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), family(r["Kernel_Name"])) for r in csv.DictReader(open(a.trace)))
    steps, cur = [], []
    for i, (b, e, f) in enumerate(ks):
        gap = ks[i + 1][0] - e if i + 1 < len(ks) else None
        cur.append((f, e - b, gap))
        if f.startswith("adam"):
            steps.append(cur)
            cur = []
    shape = collections.Counter(tuple(f for f, _, _ in s) for s in steps).most_common(1)
    if not shape or shape[0][1] < a.min_steps:
        sys.exit(f"boundary_gaps: fewer than {a.min_steps} steps with one launch sequence in {a.trace}")
    kept = [s for s in steps if tuple(f for f, _, _ in s) == shape[0][0]]
    wb, stale = written_bytes(a.traffic)
    fams = list(dict.fromkeys(shape[0][0]))
    med = statistics.median
    rows = []
    for f in fams:
        per_step = []
        for s in kept:
            x = [(d, g) for ff, d, g in s if ff == f and g is not None and not ff.startswith("adam")]
            if f.startswith("adam"):
                x = [(d, 0) for ff, d, g in s if ff == f]
            per_step.append((len(x), sum(d for d, _ in x), sum(g for _, g in x)))
        n = per_step[0][0]
        if not n:
            continue
        dur, gap = med(p[1] for p in per_step) / 1e3, med(p[2] for p in per_step) / 1e3
        rows.append((f, n, dur / n, gap / n, dur, gap, wb.get(f)))
    print(f"# {os.path.basename(a.trace)}: {len(kept)} steps of {len(shape[0][0])} launches (of {len(steps)} optimizer launches in the trace)")
    print(f"# written bytes: {'-' if not wb else os.path.basename(a.traffic) + (' (stale: recorded for other kernel sources)' if stale else '')}")
    print(f"{'family':44s} {'n/step':>6s} {'dur us':>8s} {'gap us':>8s} {'dur/step':>9s} {'gap/step':>9s} {'dur+gap':>9s} {'MB written':>10s}")
    for f, n, d1, g1, d, g, w in rows:
        print(f"{f[:44]:44s} {n:6d} {d1:8.2f} {g1:8.2f} {d:9.1f} {g:9.1f} {d + g:9.1f} {('%10.2f' % (w / 1e6)) if w is not None else '         -'}")
    td, tg = sum(r[4] for r in rows), sum(r[5] for r in rows)
    print(f"{'all (gap behind the optimizer launch left out)':44s} {sum(r[1] for r in rows):6d} {'':8s} {'':8s} {td:9.1f} {tg:9.1f} {td + tg:9.1f}")
    tail = med(s[-1][2] for s in kept if s[-1][2] is not None) / 1e3
    print(f"# behind the optimizer launch, to the next step's first kernel: {tail:.1f} us (host work between replays included)")


if __name__ == "__main__":
    main()

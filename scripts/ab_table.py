#!/usr/bin/env python3
"""Table of a scripts/lib_ab.sh output (or any file of bench.py JSON lines,
each preceded by a {"variant": ...} marker line): per variant the runs'
`value`, its median and spread (max - min), and the medians of the pack and
unpack times of --full runs.

    ab_table.py OUT [baseline variant]

With a baseline it also says, per variant, whether its median lies outside
three times the larger of the two spreads."""
import json
import statistics
import sys

runs = {}
variant = None
for ln in open(sys.argv[1]):
    ln = ln.strip()
    if not ln.startswith("{"):
        continue
    d = json.loads(ln)
    if "variant" in d and "value" not in d:
        variant = d["variant"]
        continue
    if "value" in d:
        runs.setdefault(variant, []).append(d)
base = sys.argv[2] if len(sys.argv) > 2 else None


def med(xs):
    return statistics.median(xs) if xs else float("nan")


stat = {}
for v, rs in runs.items():
    vals = [r["value"] for r in rs]
    stat[v] = (med(vals), max(vals) - min(vals))
for v, rs in runs.items():
    vals = [r["value"] for r in rs]
    k = [r["kernels"] for r in rs if "kernels" in r]
    m, sp = stat[v]
    row = f"{v:12s} n={len(vals)} median {m:8.1f} spread {sp:5.1f}  [{' '.join(f'{x:.1f}' for x in vals)}]"
    if k:
        row += (f"  pack {med([x['pack']['ms'] for x in k]) * 1e3:6.1f} us"
                f"  unpack {med([x['unpack']['ms'] for x in k]) * 1e3:6.1f} us")
        if all("pack_nosync" in x for x in k):
            row += f"  pack_nosync {med([x['pack_nosync']['ms'] for x in k]) * 1e3:6.1f} us"
    if base and v != base and base in stat:
        bm, bs = stat[base]
        bar = 3 * max(sp, bs)
        row += f"  vs {base}: {m - bm:+.1f} ({(m / bm - 1) * 100:+.2f} %), bar {bar:.1f}: " + (
            "outside" if abs(m - bm) > bar else "inside")
    print(row)

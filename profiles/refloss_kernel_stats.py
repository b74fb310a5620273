"""Row (d) of profiles/refloss_bench.txt: the kernels of the fused step on their own, from the database of

    rocprofv3 --kernel-trace --stats -d DIR -o refloss -- python profiles/refloss_bench.py --kernels

The --kernels run does only fused steps, three cases in turn (profiles/refloss_bench.py).  A case starts at its first
k_refloss_gated dispatch of a new batch size (that kernel's grid_y is the batch).  Per case and kernel: the median
duration of one dispatch and the dispatches per step (count / the case's k_refloss_gated count).

usage: refloss_kernel_stats.py DB [--out FILE]   (appends JSON lines to FILE)
"""
from __future__ import annotations

import argparse
import collections
import json
import re
import sqlite3
import statistics

CASES = {4: "4x3x256x256", 32: "32x3x224x224", 8: "8x3x2160x3840"}


def short(name: str) -> str:
    m = re.search(r"uwie::\(anonymous namespace\)::(\w+(<[^>]*>)?)", name)
    if m:
        return m.group(1)
    return name.split("(")[0][:60]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    con = sqlite3.connect(a.db)
    rows = con.execute("select name, grid_y, duration from kernels order by start").fetchall()
    case, per = None, collections.defaultdict(lambda: collections.defaultdict(list))
    for name, gy, dur in rows:
        s = short(name)
        if s == "k_refloss_gated" and CASES.get(gy) != case:
            case = CASES.get(gy)
        if case is not None:
            per[case][s].append(dur)
    lines = []
    for case, ks in per.items():
        steps = len(ks["k_refloss_gated"])
        total = 0.0
        for s, d in sorted(ks.items(), key=lambda kv: -statistics.median(kv[1]) * len(kv[1])):
            med = statistics.median(d) / 1e3
            calls = len(d) / steps
            total += med * calls
            lines.append({"case": case, "row": "(d) kernel " + s, "us": round(med, 2), "per step": round(calls, 2)})
        lines.append({"case": case, "row": "(d) all kernels of a fused step", "ms": round(total / 1e3, 4)})
    out = [json.dumps(r) for r in lines]
    print("\n".join(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

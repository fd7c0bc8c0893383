#!/usr/bin/env python
"""One line per group of bench.py result files <group>_<n>.json in a directory: ms_per_step of every run, mean, spread
(max - min), and the segments / rows / finish kernel times.  usage: tools/bench_summary.py <dir>"""
import glob, json, os, re, sys
out = sys.argv[1]
groups = {}
for f in sorted(glob.glob(os.path.join(out, "*.json"))):
    tag = os.path.basename(f)[:-5]
    try:
        d = json.loads(open(f).read().strip().splitlines()[-1])
    except Exception as e:
        print(tag, "unreadable", e); continue
    g = re.sub(r"_\d+$", "", tag)
    groups.setdefault(g, []).append((d["ms_per_step"], d["kernels_ms_per_step"]["segments"], d["kernels_ms_per_step"]["rows"], d["kernels_ms_per_step"]["finish"]))
for g, v in groups.items():
    ms = [x[0] for x in v]
    print("%-18s n=%d ms_per_step %s  mean %.3f spread %.3f | segments %s | rows %s | finish %s" % (
        g, len(v), " ".join("%.3f" % x for x in ms), sum(ms) / len(ms), max(ms) - min(ms),
        " ".join("%.3f" % x[1] for x in v), " ".join("%.2f" % x[2] for x in v), " ".join("%.3f" % x[3] for x in v)))

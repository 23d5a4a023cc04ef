"""bench.py's result lines of the parent commit and of this tree, taken alternately in one session on one MI355X: per quantity the
median of each side, the parent's own spread (max - min of its repeats), and whether this tree's median is worse than the parent's by
more than that spread.  Exit status 1 if it is, for any quantity.

usage: compare_bench.py DIR   (DIR holds bench_{parent,tree}_{f64,f32}_{1,2,3}.json)"""
import glob
import json
import os
import statistics
import sys

QUANTITIES = [  # name, how to read it, higher is better
    ("value, Gnode-updates/s", lambda j: j["value"], True),
    ("boundary launch to t+1, ms", lambda j: j["roofline"]["boundary"]["ms"][0], False),
    ("boundary launch to t+2, ms", lambda j: j["roofline"]["boundary"]["ms"][1], False),
    ("boundary launch to t+3, ms", lambda j: j["roofline"]["boundary"]["third_level_ms"]["boundary_nodes_to_t3"], False),
    ("third level's list, ms", lambda j: j["roofline"]["boundary"]["third_level_ms"]["fixup_list_of_the_shell_nodes"], False),
]
failed = False
for precision in ("f64", "f32"):
    runs = {side: [json.loads(open(f).read().strip().splitlines()[-1]) for f in sorted(glob.glob(os.path.join(sys.argv[1], "bench_%s_%s_*.json" % (side, precision))))]
            for side in ("parent", "tree")}
    print("%s: %d runs of the parent, %d of this tree (steps %d, warmup %d)" % (precision, len(runs["parent"]), len(runs["tree"]), runs["tree"][0]["steps"], runs["tree"][0]["warmup"]))
    for name, get, higher in QUANTITIES:
        try:
            p, t = [get(j) for j in runs["parent"]], [get(j) for j in runs["tree"]]
        except KeyError:
            continue  # (two-step passes, --tuning triple=0: no third level)
        pm, tm, spread = statistics.median(p), statistics.median(t), max(p) - min(p)
        worse_by = (pm - tm) if higher else (tm - pm)
        ok = worse_by <= spread
        failed = failed or not ok
        print("  %-30s parent %s median %.4f spread %.4f | tree %s median %.4f | worse by %+.4f: %s" % (name, p, pm, spread, t, tm, worse_by, "ok" if ok else "WORSE THAN THE SPREAD"))
sys.exit(1 if failed else 0)

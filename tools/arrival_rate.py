#!/usr/bin/env python3
"""What an arrival map costs: seconds of a box room with an impulse source over a run with no plan, with a plain decay plan
(wv_set_decay: the yardstick, one global clock) and with an arrival plan (wv_set_arrival: onset, peak and bins counted from every
node's own arrival) of the same box and cadence.  One invocation, the three alternating, `--repeats` repeats each; every repeat
starts from the same checkpoint.  Per plan and period: seconds (min / median / max), the cost per capture over the run without a
plan, the fold kernel's mean time from a further repeat with kernel timing on, and the traffic model of a full fold beside it.  At the
last period the arrival plan's six outputs are compared byte for byte with arrival.arrival_fold over a snapshot plan's captures.

    python tools/arrival_rate.py [--dims 1024,1024,64] [--steps 240] [--periods 1,8] [--precision f64] [--repeats 5] [--json FILE]

The box is the full z-plane in the middle of the mesh.  No bar: figures (DESIGN.md 4.13 has the model they are held against)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import arrival as A, engine as E, mesh as M  # noqa: E402

EDGES = (0, 10, 16)        # bins of 10 and 6 captures and the open-ended rest: an edge inside a fold and one on a fold's end
DECAY = (3, 80)            # the yardstick: three bins of 80 captures
THRESHOLD = 1e-6


def rows_for(eng, dims, steps, period, repeats):
    eng.rollback()                                          # (every period starts where the checkpoint stands)
    start = eng.step_count()
    plan = dict(box=((0, 0, dims[2] // 2), (None, None, 1)), first_step=start + period, period=period)
    captures = steps // period
    nodes = dims[0] * dims[1]
    setters = {"none": lambda: None, "decay": lambda: eng.set_decay(DECAY[0], DECAY[1], **plan), "arrival": lambda: eng.set_arrival(EDGES, THRESHOLD, **plan)}
    seconds, folds, out = {k: [] for k in setters}, {}, None
    for repeat in range(repeats + 1):                      # the last repeat runs with kernel timing on and is not timed
        timing = repeat == repeats
        for name, set_plan in setters.items():             # the three alternate within every round
            eng.rollback()
            assert eng.step_count() == start
            set_plan()                                      # (a plan's memory is allocated outside the timed region, as the engine's is)
            eng.enable_kernel_timing(timing)
            eng.synchronize()
            t0 = time.perf_counter()
            assert eng.run_steps(steps) == (steps, 0)
            if name == "decay":
                got, count = eng.fetch_decay()
            elif name == "arrival":
                got, count = eng.fetch_arrival()
            eng.synchronize()
            if not timing:
                seconds[name].append(time.perf_counter() - t0)
            if name != "none":
                assert count == captures
                if timing:
                    n = eng.query(E.Engine.QUERY_DECAY_FOLDS if name == "decay" else E.Engine.QUERY_ARRIVAL_FOLDS)
                    ns = eng.query(E.Engine.QUERY_DECAY_NS if name == "decay" else E.Engine.QUERY_ARRIVAL_NS)
                    # a full fold of 16 captures: decay 4 t + 16 r bytes per node, arrival 4 t + 28 + 16 r (r = 1 late in a run)
                    model = nodes * (64 + 16) if name == "decay" else nodes * (64 + 28 + 16)
                    folds[name] = dict(folds=n, mean_fold_ms=ns / 1e6 / n if n else 0.0, model_bytes_full_fold=model)
                if name == "arrival":
                    out = got
            eng.enable_kernel_timing(False)
            eng.set_decay(None)
            eng.set_arrival(None)
    return seconds, folds, out, plan, captures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="1024,1024,64")
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--periods", default="1,8")
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    dims = tuple(int(v) for v in args.dims.split(","))
    periods = [int(v) for v in args.periods.split(",")]
    steps = args.steps
    assert len(dims) == 3 and all(steps % p == 0 for p in periods) and args.repeats >= 1
    report = {"dims": dims, "steps": steps, "repeats": args.repeats, "edges": EDGES, "decay": DECAY, "threshold": THRESHOLD}
    ok = True
    for precision in args.precision.split(","):
        mesh = M.box_mesh(*dims, coefficients=M.bench_materials(), surface_of_face=[0, 1, 2, 3, 2, 3])
        eng = E.Engine(mesh, precision=precision)
        mesh.nodes = None
        try:
            sig = np.zeros(64 + steps)
            sig[0] = 1.0
            eng.set_source(E.SOURCE_HARD, mesh.compute_index(dims[0] // 2, dims[1] // 2, dims[2] // 2), sig)
            eng.set_receivers([mesh.compute_index(dims[0] // 2 + 3, dims[1] // 2, dims[2] // 2)])
            assert eng.run_steps(48) == (48, 0)     # warm-up: passes set up, the wave front well inside the box
            eng.checkpoint()
            print("%dx%dx%d %s, plane z=%d (%d nodes), %d steps per repeat, %d repeats; seconds (min / median / max)"
                  % (dims + (precision, dims[2] // 2, dims[0] * dims[1], steps, args.repeats)), flush=True)
            report[precision] = {}
            for period in periods:
                seconds, folds, out, plan, captures = rows_for(eng, dims, steps, period, args.repeats)
                base = float(np.median(seconds["none"]))
                rows = {}
                for name, s in seconds.items():
                    s = sorted(s)
                    rows[name] = dict(seconds_min=s[0], seconds_median=float(np.median(s)), seconds_max=s[-1], **folds.get(name, {}))
                    if name != "none":
                        rows[name]["us_per_capture"] = (rows[name]["seconds_median"] - base) / captures * 1e6
                    f = folds.get(name)
                    print("  every %d  %-8s %8.4f / %8.4f / %8.4f s%s%s" % (period, name, s[0], rows[name]["seconds_median"], s[-1],
                          "" if name == "none" else "; %8.2f us per capture over no plan" % rows[name]["us_per_capture"],
                          "" if not f else "; %d folds, mean %.4f ms, model %d bytes per full fold" % (f["folds"], f["mean_fold_ms"], f["model_bytes_full_fold"])),
                          flush=True)
                spread = max(rows[n]["seconds_max"] - rows[n]["seconds_min"] for n in rows)
                ratio = rows["arrival"]["us_per_capture"] / rows["decay"]["us_per_capture"] if rows["decay"]["us_per_capture"] > 0 else float("nan")
                print("  every %d  arrival / decay per capture: %.3f (largest spread of a row: %.4f s = %.2f us per capture)"
                      % (period, ratio, spread, spread / captures * 1e6), flush=True)
                report[precision]["every %d" % period] = dict(rows=rows, captures=captures, arrival_over_decay_per_capture=ratio,
                                                               largest_spread_s=spread)
            # the outputs of the last period's arrival plan against the definition over a snapshot plan's captures
            eng.rollback()
            eng.set_snapshots(**plan)
            assert eng.run_steps(steps) == (steps, 0)
            snaps, _ = eng.fetch_snapshots()
            eng.set_snapshots(None)
            want = A.arrival_fold(snaps, np.float32(THRESHOLD), EDGES)
            same = all(out[k].tobytes() == want[k].tobytes() for k in A.KEYS)
            heard = want["onset"] != A.NONE
            print("  every %d  against arrival.arrival_fold over the snapshots: %s; %d of %d nodes have an onset, in %d distinct captures"
                  % (periods[-1], "bytewise equal" if same else "DIFFER", heard.sum(), heard.size, len(set(want["onset"][heard].tolist()))), flush=True)
            report[precision]["bytewise_equal"] = bool(same)
            ok = ok and same
        finally:
            eng.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    print("ARRIVAL RATE %s" % ("OK" if ok else "OUTPUTS DIFFER"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

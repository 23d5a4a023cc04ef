#!/usr/bin/env python3
"""What a lateral map costs: seconds of a box room with an impulse source over a run with no plan, with an intensity plan
(wv_set_intensity: the yardstick, the same capture, one global clock, p v only) and with a lateral plan (wv_set_lateral: p^2, p v
and v v^T in bins counted from every node's own arrival) of the same box and cadence.  One invocation, the ways alternating,
`--repeats` repeats each; every repeat starts from the same checkpoint.  The lateral plan runs twice: with a threshold the wavefront
reaches while it crosses the plane (most nodes are ahead of their onset and touch no bin), and with a threshold of 0 (every node is
behind its onset: the steady state the model B (16 t + 52 + 160 r) describes).  Per plan and period: seconds of the run (min / median
/ max) and the cost per capture over the run without a plan, seconds of the fetch on its own, the fold kernel's and the capture
kernel's mean times from a further repeat with kernel timing on, and beside the fold the bytes the model gives for THIS run's folds
(lateral.fold_traffic over the final onsets).  At the last period the lateral plan's outputs are compared byte for byte
with lateral.lateral_fold over a snapshot plan's captures of the box's hull.

    python tools/lateral_rate.py [--dims 1024,1024,64] [--steps 240] [--periods 1,8] [--precision f64] [--repeats 5] [--json FILE]

The box is the z-plane in the middle of the mesh less its rim.  No bar: figures (DESIGN.md 4.14 has the model they are held against)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import engine as E, lateral as L, mesh as M  # noqa: E402

EDGES = (0, 10, 16)        # bins of 10 and 6 captures and the open-ended rest: an edge inside a fold and one on a fold's end
INTENSITY = (3, 80)        # the yardstick: three bins of 80 captures
THRESHOLD = 1e-6
SPACING, RATE, DENSITY = 0.05, 12000.0, 1.2


def fold_sizes(captures):
    """The engine folds when its stage of 16 is full, and what is left on the fetch."""
    return [16] * (captures // 16) + ([captures % 16] if captures % 16 else [])


def intensity_model(nodes, captures):
    """Bytes per fold of the intensity plan: 16 t + 48 + 64 r per node, r the distinct bins among the fold's captures (at EVERY node)."""
    out, c0 = [], 0
    for t in fold_sizes(captures):
        bins = {min(c // INTENSITY[1], INTENSITY[0] - 1) for c in range(c0, c0 + t)}
        out.append(nodes * (16 * t + 48 + 64 * len(bins)))
        c0 += t
    return out


def rows_for(eng, dims, steps, period, repeats):
    eng.rollback()                                          # (every period starts where the checkpoint stands)
    start = eng.step_count()
    box = ((1, 1, dims[2] // 2), (dims[0] - 2, dims[1] - 2, 1))
    plan = dict(box=box, first_step=start + period, period=period)
    constants = dict(spacing=SPACING, sample_rate=RATE / period, ambient_density=DENSITY)
    captures = steps // period
    nodes = (dims[0] - 2) * (dims[1] - 2)
    # "lateral": the front is still crossing the plane, most nodes are ahead of their onset and touch no bin; "lateral steady": a
    # threshold of 0 puts every node behind its onset from capture 0 on -- the state the model B (16 t + 52 + 160 r) describes
    setters = {"none": lambda: None, "intensity": lambda: eng.set_intensity(INTENSITY[0], INTENSITY[1], **plan, **constants),
               "lateral": lambda: eng.set_lateral(EDGES, THRESHOLD, **plan, **constants),
               "lateral steady": lambda: eng.set_lateral(EDGES, 0.0, **plan, **constants)}
    intensity_queries = (E.Engine.QUERY_INTENSITY_FOLDS, E.Engine.QUERY_INTENSITY_NS, E.Engine.QUERY_INTENSITY_GATHERS, E.Engine.QUERY_INTENSITY_GATHER_NS)
    lateral_queries = (E.Engine.QUERY_LATERAL_FOLDS, E.Engine.QUERY_LATERAL_NS, E.Engine.QUERY_LATERAL_GATHERS, E.Engine.QUERY_LATERAL_GATHER_NS)
    seconds, fetches, kernels, out = {k: [] for k in setters}, {k: [] for k in setters if k != "none"}, {}, None
    for repeat in range(repeats + 1):                      # the last repeat runs with kernel timing on and is not timed
        timing = repeat == repeats
        for name, set_plan in setters.items():             # the four alternate within every round
            eng.rollback()
            assert eng.step_count() == start
            set_plan()                                      # (a plan's memory is allocated outside the timed region, as the engine's is)
            eng.enable_kernel_timing(timing)
            eng.synchronize()
            t0 = time.perf_counter()
            assert eng.run_steps(steps) == (steps, 0)
            eng.synchronize()
            t1 = time.perf_counter()                        # the run; the fetch (with the fold of what is staged) is timed on its own
            if name == "intensity":
                got, count = eng.fetch_intensity()
            elif name != "none":
                got, count = eng.fetch_lateral()
            eng.synchronize()
            t2 = time.perf_counter()
            if not timing:
                seconds[name].append(t1 - t0)
                if name != "none":
                    fetches[name].append(t2 - t1)
            if name != "none":
                assert count == captures
                if timing:
                    folds, fold_ns, gathers, gather_ns = (eng.query(q) for q in (intensity_queries if name == "intensity" else lateral_queries))
                    model = intensity_model(nodes, captures) if name == "intensity" else L.fold_traffic(got["onset"], EDGES, fold_sizes(captures))
                    if folds != len(model):                 # (the model's bytes are then spread over the folds there were)
                        print("  every %d  %s: %d folds where the stage alone would make %d" % (period, name, folds, len(model)), flush=True)
                    mean_ms = fold_ns / 1e6 / folds
                    kernels[name] = dict(folds=folds, mean_fold_ms=mean_ms, model_bytes_mean_fold=sum(model) / folds,
                                         model_tb_per_s=sum(model) / folds / (mean_ms * 1e-3) / 1e12, gathers=gathers,
                                         mean_gather_ms=gather_ns / 1e6 / gathers if gathers else 0.0,
                                         fetch_bytes=int(got.nbytes if name == "intensity" else sum(v.nbytes for v in got.values())))
                    if name != "intensity":
                        kernels[name]["nodes_with_an_onset_at_the_end"] = int((got["onset"] != L.NONE).sum())
                if name == "lateral":
                    out = got
            eng.enable_kernel_timing(False)
            eng.set_intensity(None)
            eng.set_lateral(None)
    return seconds, fetches, kernels, out, plan, constants, captures


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
    report = {"dims": dims, "steps": steps, "repeats": args.repeats, "edges": EDGES, "intensity": INTENSITY, "threshold": THRESHOLD}
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
            print("%dx%dx%d %s, plane z=%d less its rim (%d nodes), %d steps per repeat, %d repeats; seconds (min / median / max)"
                  % (dims + (precision, dims[2] // 2, (dims[0] - 2) * (dims[1] - 2), steps, args.repeats)), flush=True)
            report[precision] = {}
            for period in periods:
                seconds, fetches, kernels, out, plan, constants, captures = rows_for(eng, dims, steps, period, args.repeats)
                base = float(np.median(seconds["none"]))
                rows = {}
                for name, sec in seconds.items():
                    sec = sorted(sec)
                    rows[name] = dict(seconds_min=sec[0], seconds_median=float(np.median(sec)), seconds_max=sec[-1], **kernels.get(name, {}))
                    line = "  every %d  %-14s run %8.4f / %8.4f / %8.4f s" % (period, name, sec[0], rows[name]["seconds_median"], sec[-1])
                    if name != "none":
                        f, k = sorted(fetches[name]), kernels[name]
                        rows[name].update(us_per_capture=(rows[name]["seconds_median"] - base) / captures * 1e6, fetch_seconds_min=f[0],
                                          fetch_seconds_median=float(np.median(f)), fetch_seconds_max=f[-1])
                        line += "; %8.2f us per capture over no plan; fetch %7.4f / %7.4f / %7.4f s for %d bytes" \
                            % (rows[name]["us_per_capture"], f[0], rows[name]["fetch_seconds_median"], f[-1], k["fetch_bytes"])
                        line += "; %d folds, mean %.4f ms for %.0f model bytes = %.2f TB/s; %d captures timed, mean %.4f ms" \
                            % (k["folds"], k["mean_fold_ms"], k["model_bytes_mean_fold"], k["model_tb_per_s"], k["gathers"], k["mean_gather_ms"])
                        if "nodes_with_an_onset_at_the_end" in k:
                            line += "; %d nodes behind their onset at the end" % k["nodes_with_an_onset_at_the_end"]
                    print(line, flush=True)
                spread = max(rows[n]["seconds_max"] - rows[n]["seconds_min"] for n in rows)
                ratios = {}
                for name in ("lateral", "lateral steady"):
                    ratios[name] = dict(per_capture=rows[name]["us_per_capture"] / rows["intensity"]["us_per_capture"] if rows["intensity"]["us_per_capture"] > 0 else float("nan"),
                                        per_fold_measured=kernels[name]["mean_fold_ms"] / kernels["intensity"]["mean_fold_ms"],
                                        per_fold_model=kernels[name]["model_bytes_mean_fold"] / kernels["intensity"]["model_bytes_mean_fold"])
                    print("  every %d  %s / intensity per capture of the run: %.3f; per fold: %.3f measured, %.3f by the model of this run"
                          % (period, name, ratios[name]["per_capture"], ratios[name]["per_fold_measured"], ratios[name]["per_fold_model"]), flush=True)
                print("  every %d  largest spread of a row: %.4f s = %.2f us per capture" % (period, spread, spread / captures * 1e6), flush=True)
                report[precision]["every %d" % period] = dict(rows=rows, captures=captures, over_intensity=ratios, largest_spread_s=spread)
            # the outputs of the last period's lateral plan against the definition over a snapshot plan's captures of the hull
            eng.rollback()
            (origin, extent), box_in_hull = L.hull_box(plan["box"])
            eng.set_snapshots(box=(origin, extent), first_step=plan["first_step"], period=plan["period"])
            assert eng.run_steps(steps) == (steps, 0)
            snaps, _ = eng.fetch_snapshots()
            eng.set_snapshots(None)
            want = L.lateral_fold(snaps, box_in_hull, np.float32(THRESHOLD), EDGES, constants["spacing"], constants["sample_rate"],
                                  constants["ambient_density"])
            same = all(out[k].tobytes() == want[k].tobytes() for k in L.KEYS)
            heard = want["onset"] != L.NONE
            print("  every %d  against lateral.lateral_fold over the hull snapshots: %s; %d of %d nodes have an onset, in %d distinct captures"
                  % (periods[-1], "bytewise equal" if same else "DIFFER", heard.sum(), heard.size, len(set(want["onset"][heard].tolist()))), flush=True)
            report[precision]["bytewise_equal"] = bool(same)
            ok = ok and same
        finally:
            eng.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    print("LATERAL RATE %s" % ("OK" if ok else "OUTPUTS DIFFER"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

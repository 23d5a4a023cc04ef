#!/usr/bin/env python3
"""What a band-limited arrival map costs: seconds of a box room with an impulse source over a run with no plan, with an arrival plan
(wv_set_arrival), with a banded decay plan (wv_set_decay_bands: the yardstick, the same capture and cascades on one global clock) and
with a banded arrival plan (wv_set_arrival_bands) of the same box and cadence, for every band count of `--bands`, four sections per
band.  One invocation, the four alternating, `--repeats` repeats each; every repeat starts from the same checkpoint.  Per plan: seconds
(min / median / max), the cost per capture over the run without a plan, the fold kernel's mean time from a further repeat with kernel
timing on -- also as ns per node and capture -- and the traffic model of a full fold beside it.  At every band count the banded arrival
plan's outputs on a strip of the plane are compared byte for byte with arrival.banded_arrival_fold over a snapshot plan's captures.

    python tools/arrival_bands_rate.py [--dims 1024,1024,64] [--steps 240] [--bands 1,4,8] [--period 1] [--precision f64] [--repeats 5] [--json FILE]

The box is the full z-plane in the middle of the mesh.  No bar: figures (DESIGN.md 4.17 has the model they are held against)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import arrival as A, decay as D, engine as E, mesh as M  # noqa: E402

EDGES = (0, 10, 16)        # bins of 10 and 6 captures, then ...
TAIL = (21, 26, 10)        # ... one of 10 that ends at 26, and 21 bins of 10 captures from there, the last open-ended: 24 bins
DECAY = (24, 10)           # the yardstick: 24 bins of 10 captures
SECTIONS = 4
THRESHOLD = 1e-6
CENTRES = (250.0, 500.0, 1000.0, 125.0, 2000.0, 63.0, 31.5, 16.0)   # octave bands at a nominal 8 kHz, the first K of them
RATE = 8000.0
STRIP = 64                 # rows of the plane compared with the definition: the ones around the source, which the wave front has crossed
FOLD_BINS = 2              # bins a full fold of 16 captures touches where bins are 10 captures long


def strip_rows(dims):
    y0 = max(0, dims[1] // 2 - STRIP // 2)
    return y0, min(STRIP, dims[1] - y0)


def rows_for(eng, dims, steps, period, repeats, sections, lags):
    eng.rollback()
    start = eng.step_count()
    plan = dict(box=((0, 0, dims[2] // 2), (None, None, 1)), first_step=start + period, period=period)
    captures = steps // period
    nodes, K = dims[0] * dims[1], sections.shape[0]
    setters = {"none": lambda: None, "arrival": lambda: eng.set_arrival(EDGES, THRESHOLD, **plan),
               "decay_bands": lambda: eng.set_decay(DECAY[0], DECAY[1], bands=sections, **plan),
               "arrival_bands": lambda: eng.set_arrival_bands(EDGES, sections, THRESHOLD, tail=TAIL, lag=lags, **plan)}
    fetch = {"arrival": eng.fetch_arrival, "decay_bands": eng.fetch_decay, "arrival_bands": eng.fetch_arrival_bands}
    queries = {"arrival": (E.Engine.QUERY_ARRIVAL_FOLDS, E.Engine.QUERY_ARRIVAL_NS), "decay_bands": (E.Engine.QUERY_DECAY_FOLDS, E.Engine.QUERY_DECAY_NS),
               "arrival_bands": (E.Engine.QUERY_ARRIVAL_BANDS_FOLDS, E.Engine.QUERY_ARRIVAL_BANDS_NS)}
    # a full fold of 16 captures, bytes per node
    model = {"arrival": 64 + 28 + 16 * FOLD_BINS, "decay_bands": K * (64 + 32 * SECTIONS + 16 * FOLD_BINS),
             "arrival_bands": K * (64 + 32 * SECTIONS + 20 + 16 * FOLD_BINS) + 8}
    seconds, folds, out = {k: [] for k in setters}, {}, None
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
            if name != "none":
                got, count = fetch[name]()
            eng.synchronize()
            if not timing:
                seconds[name].append(time.perf_counter() - t0)
            if name != "none":
                assert count == captures
                if timing:
                    n, ns = eng.query(queries[name][0]), eng.query(queries[name][1])
                    folds[name] = dict(folds=n, mean_fold_ms=ns / 1e6 / n if n else 0.0, model_bytes_full_fold=nodes * model[name],
                                       fold_ns_per_node_and_capture=ns / (nodes * captures))
                if name == "arrival_bands":
                    y0, n_rows = strip_rows(dims)
                    out = {k: np.ascontiguousarray(v[..., y0:y0 + n_rows, :]) for k, v in got.items()}
                del got
            eng.enable_kernel_timing(False)
            eng.set_decay(None)
            eng.set_arrival(None)
            eng.set_arrival_bands(None, None)
    return seconds, folds, out, plan, captures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="1024,1024,64")
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--bands", default="1,4,8")
    ap.add_argument("--period", type=int, default=1)
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    dims = tuple(int(v) for v in args.dims.split(","))
    counts = [int(v) for v in args.bands.split(",")]
    steps, period = args.steps, args.period
    assert len(dims) == 3 and steps % period == 0 and args.repeats >= 1 and all(1 <= k <= 8 for k in counts)
    report = {"dims": dims, "steps": steps, "period": period, "repeats": args.repeats, "edges": EDGES, "tail": TAIL, "decay": DECAY,
              "sections": SECTIONS, "threshold": THRESHOLD}
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
            print("%dx%dx%d %s, plane z=%d (%d nodes), %d steps per repeat at period %d, %d repeats; seconds (min / median / max)"
                  % (dims + (precision, dims[2] // 2, dims[0] * dims[1], steps, period, args.repeats)), flush=True)
            report[precision] = {}
            for K in counts:
                bands = D.octave_band_edges(CENTRES[:K])
                sections = np.stack([D.butterworth_bandpass(lo, hi, RATE / period) for lo, hi in bands])
                lags = [min(A.lag_captures(sections[k], c, RATE / period), 40) for k, c in enumerate(CENTRES[:K])]
                seconds, folds, out, plan, captures = rows_for(eng, dims, steps, period, args.repeats, sections, lags)
                base = float(np.median(seconds["none"]))
                rows = {}
                for name, s in seconds.items():
                    s = sorted(s)
                    rows[name] = dict(seconds_min=s[0], seconds_median=float(np.median(s)), seconds_max=s[-1], **folds.get(name, {}))
                    if name != "none":
                        rows[name]["us_per_capture"] = (rows[name]["seconds_median"] - base) / captures * 1e6
                    f = folds.get(name)
                    print("  %d bands  %-13s %8.4f / %8.4f / %8.4f s%s%s" % (K, name, s[0], rows[name]["seconds_median"], s[-1],
                          "" if name == "none" else "; %8.2f us per capture over no plan" % rows[name]["us_per_capture"],
                          "" if not f else "; %d folds, mean %.4f ms = %.4f ns per node and capture, model %d bytes per full fold"
                          % (f["folds"], f["mean_fold_ms"], f["fold_ns_per_node_and_capture"], f["model_bytes_full_fold"])), flush=True)
                both = rows["decay_bands"]["mean_fold_ms"] + rows["arrival"]["mean_fold_ms"]
                ratio = rows["arrival_bands"]["mean_fold_ms"] / both if both > 0 else float("nan")
                print("  %d bands  fold: arrival_bands / (decay_bands + arrival) = %.3f; lags %r" % (K, ratio, lags), flush=True)
                # the plan's outputs on a strip of the plane against the definition over a snapshot plan's captures
                eng.rollback()
                y0, n_rows = strip_rows(dims)
                strip = dict(plan, box=((0, y0, dims[2] // 2), (None, n_rows, 1)))
                eng.set_snapshots(**strip)
                assert eng.run_steps(steps) == (steps, 0)
                snaps, _ = eng.fetch_snapshots()
                eng.set_snapshots(None)
                want = A.banded_arrival_fold(snaps, np.float32(THRESHOLD), EDGES, sections, tail=TAIL, lag=lags)
                same = all(out[k].tobytes() == want[k].tobytes() for k in A.KEYS)
                heard = want["onset"] != A.NONE
                print("  %d bands  against arrival.banded_arrival_fold over the snapshots of %d rows: %s; %d of %d nodes have an onset, in %d distinct "
                      "captures; %d of %d bins hold energy" % (K, snaps.shape[2], "bytewise equal" if same else "DIFFER", heard.sum(), heard.size,
                                                                len(set(want["onset"][heard].tolist())), (want["bins"].reshape(K, want["bins"].shape[1], -1).max(axis=2) > 0).sum(),
                                                                K * want["bins"].shape[1]), flush=True)
                report[precision]["%d bands" % K] = dict(rows=rows, captures=captures, lags=lags, bytewise_equal=bool(same),
                                                           fold_over_decay_bands_plus_arrival=ratio)
                ok = ok and same
        finally:
            eng.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    print("ARRIVAL BANDS RATE %s" % ("OK" if ok else "OUTPUTS DIFFER"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

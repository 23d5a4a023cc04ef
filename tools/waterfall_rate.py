#!/usr/bin/env python3
"""What a waterfall of the field costs: steps per second of a box room with a source while a box of the field is Fourier-transformed
at K frequencies per time bin over a run, the way it had to be done before wv_set_waterfall (a snapshot plan, fetch_snapshots, the
binned Fourier sums in NumPy on the host -- timed to the finished bins) against a waterfall plan (the engine folds on the device;
fetch_waterfall brings n_bins * K complex fields).  One invocation, the ways alternating, every repeat from the same checkpoint, so
both ways capture the same steps and their bins are compared bytewise.

    python tools/waterfall_rate.py [--side 512] [--steps 480] [--repeats 3] [--precision f64] [--json FILE]

cases (both at period 3, so that every pass stays a three-step pass):
       plane   one full z-plane, K = 16, 32 bins
       field   the whole field decimated by 4 on every axis, K = 8, 16 bins
ways:  no plan
       snapshots + numpy    snapshot plan + fetch_snapshots + the NumPy fold (on up to 16 threads, split along the nodes)
       waterfall plan       wv_set_waterfall + fetch_waterfall
Then, with kernel timing on, per case: the fold kernel's mean time at n_bins = 1 beside the spectrum fold's for the same box and K
(the two launches move the same bytes by the model, so a difference is the held-bin branch's cost), and the fold's time per bin
edge crossed (the binned plan's fold time less the one-bin plan's, over the edges its folds crossed)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import engine as E, mesh as M  # noqa: E402

PERIOD = 3
STAGE = 16
THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))
WAYS = ("no plan", "snapshots + numpy", "waterfall plan")


def host_fold(snaps, steps, freqs, n_bins, bin_captures, pool):
    """The definition (include/wayverb_amd.h), in capture order: re[b][k] = re[b][k] + p * c, im[b][k] = im[b][k] - p * s on float64 arrays."""
    n, K = snaps.shape[0], len(freqs)
    tw = np.array([[E.spectrum_twiddle(f, int(s)) for f in freqs] for s in steps])      # [n][K][2]
    flat = snaps.reshape(n, -1)
    out = np.empty((n_bins, K, flat.shape[1]), dtype=np.complex128)
    bounds = np.linspace(0, flat.shape[1], THREADS + 1).astype(np.int64)

    def part(i):
        lo, hi = int(bounds[i]), int(bounds[i + 1])
        re, im = np.zeros((n_bins, K, hi - lo)), np.zeros((n_bins, K, hi - lo))
        for j in range(n):
            p = flat[j, lo:hi].astype(np.float64)
            b = min(j // bin_captures, n_bins - 1)
            for k in range(K):
                re[b, k] = re[b, k] + p * tw[j, k, 0]
                im[b, k] = im[b, k] - p * tw[j, k, 1]
        out.real[:, :, lo:hi], out.imag[:, :, lo:hi] = re, im

    list(pool.map(part, range(THREADS)))
    return out.reshape((n_bins, K) + snaps.shape[1:])


def edges_crossed(captures, bin_captures, n_bins):
    """Bin edges inside the folds of `captures` captures from capture 0: folds of 16, then what a fetch finds staged."""
    bin_of = lambda j: min(j // bin_captures, n_bins - 1)       # noqa: E731
    return sum(bin_of(min(first + STAGE, captures) - 1) - bin_of(first) for first in range(0, captures, STAGE))


def measure(eng, side, steps, repeats, pool):
    start = eng.step_count()
    captures = steps // PERIOD
    cases = {"plane": (dict(box=((0, 0, side // 2), (None, None, 1))), 16, 32), "field": (dict(box="mesh", stride=4), 8, 16)}
    out = {}

    def repeat(body, before=None):
        eng.rollback()
        assert eng.step_count() == start
        if before:
            before()    # (a plan is set once per run: its memory is allocated outside the timed region, as the engine itself is)
        eng.synchronize()
        t0 = time.perf_counter()
        got = body()
        seconds = time.perf_counter() - t0
        assert eng.step_count() == start + steps
        return seconds, got

    def plain():
        assert eng.run_steps(steps) == (steps, 0)

    for name, (box, K, n_bins) in cases.items():
        freqs = list(np.linspace(0.0, 0.5 / PERIOD, K))
        bin_captures = max(1, captures // n_bins)
        cadence = dict(first_step=start + PERIOD, period=PERIOD, **box)

        def old():
            assert eng.run_steps(steps) == (steps, 0)
            snaps, at = eng.fetch_snapshots()
            assert list(at) == list(range(start + PERIOD, start + steps + 1, PERIOD))
            return host_fold(snaps, at, freqs, n_bins, bin_captures, pool)

        def new():
            assert eng.run_steps(steps) == (steps, 0)
            got, count = eng.fetch_waterfall()
            assert count == captures
            return got

        seconds = {way: [] for way in WAYS}
        bins = {}
        for _ in range(repeats):   # the ways alternate within every round
            seconds["no plan"].append(repeat(plain)[0])
            s, bins["old"] = repeat(old, lambda: eng.set_snapshots(**cadence))
            seconds["snapshots + numpy"].append(s)
            eng.set_snapshots(None)
            s, bins["new"] = repeat(new, lambda: eng.set_waterfall(freqs, n_bins, bin_captures, **cadence))
            seconds["waterfall plan"].append(s)
            eng.set_waterfall(None, None, None)
        same = bins["old"].tobytes() == bins["new"].tobytes()
        # the fold kernels' own times, from the engine's events
        eng.enable_kernel_timing(True)
        fold = {}
        for label, setter, stop, folds, ns in (
                ("spectrum", lambda: eng.set_spectrum(freqs, **cadence), lambda: eng.set_spectrum(None), E.Engine.QUERY_SPECTRUM_FOLDS, E.Engine.QUERY_SPECTRUM_NS),
                ("waterfall one bin", lambda: eng.set_waterfall(freqs, 1, 1, **cadence), lambda: eng.set_waterfall(None, None, None),
                 E.Engine.QUERY_WATERFALL_FOLDS, E.Engine.QUERY_WATERFALL_NS),
                ("waterfall binned", lambda: eng.set_waterfall(freqs, n_bins, bin_captures, **cadence), lambda: eng.set_waterfall(None, None, None),
                 E.Engine.QUERY_WATERFALL_FOLDS, E.Engine.QUERY_WATERFALL_NS)):
            eng.rollback()
            setter()
            assert eng.run_steps(steps) == (steps, 0)
            eng.fetch_spectrum() if label == "spectrum" else eng.fetch_waterfall()
            n, total = eng.query(folds), eng.query(ns)
            fold[label] = dict(folds=n, total_ms=total * 1e-6, mean_ms=total * 1e-6 / max(n, 1))
            stop()
        eng.enable_kernel_timing(False)
        crossed = edges_crossed(captures, bin_captures, n_bins)
        fold["bin_edges_crossed"] = crossed
        fold["ms_per_bin_edge_crossed"] = (fold["waterfall binned"]["total_ms"] - fold["waterfall one bin"]["total_ms"]) / crossed if crossed else None
        fold["one_bin_over_spectrum"] = fold["waterfall one bin"]["mean_ms"] / fold["spectrum"]["mean_ms"] if fold["spectrum"]["mean_ms"] else None
        out[name] = dict(K=K, n_bins=n_bins, bin_captures=bin_captures, captures=captures, nodes=int(np.prod(bins["new"].shape[2:])),
                         seconds={way: sorted(s) for way, s in seconds.items()},
                         steps_per_second={way: steps / sorted(s)[len(s) // 2] for way, s in seconds.items()},
                         bytewise_equal=bool(same), not_zeros=bool(np.abs(bins["new"]).max() > 0), fold=fold)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--steps", type=int, default=480, help="steps per repeat, a multiple of 3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    if args.steps % PERIOD or args.steps < PERIOD:
        ap.error("--steps must be a multiple of %d" % PERIOD)
    side, steps = args.side, args.steps
    mesh = M.box_mesh(side, side, side, coefficients=M.bench_materials(), surface_of_face=[0, 1, 2, 3, 2, 3])
    eng = E.Engine(mesh, precision=args.precision)
    mesh.nodes = None
    with ThreadPoolExecutor(THREADS) as pool:
        try:
            sig = np.zeros(64 + steps)
            sig[0] = 1.0
            eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2, side // 2, side // 2), sig)
            eng.set_receivers([mesh.compute_index(side // 2 + 3, side // 2, side // 2)])
            assert eng.run_steps(48) == (48, 0)     # warm-up: passes set up, the wave front well inside the box
            eng.checkpoint()
            cases = measure(eng, side, steps, args.repeats, pool)
        finally:
            eng.close()
    print("%d^3 %s, %d steps per repeat, a capture every %d steps, %d repeats (median)" % (side, args.precision, steps, PERIOD, args.repeats))
    for name, c in cases.items():
        print("  %s: %d nodes, K = %d, %d bins of %d captures" % (name, c["nodes"], c["K"], c["n_bins"], c["bin_captures"]))
        for way in WAYS:
            print("    %-18s %9.1f steps/s" % (way, c["steps_per_second"][way]))
        print("    bins of the two ways: %s" % ("bytewise equal" if c["bytewise_equal"] and c["not_zeros"] else "DIFFER"))
        f = c["fold"]
        print("    fold kernels, mean ms: spectrum %.4f (%d folds), waterfall at one bin %.4f (%d), waterfall binned %.4f (%d); "
              "%s ms per bin edge crossed (%d crossed)" % (f["spectrum"]["mean_ms"], f["spectrum"]["folds"], f["waterfall one bin"]["mean_ms"],
                                                          f["waterfall one bin"]["folds"], f["waterfall binned"]["mean_ms"], f["waterfall binned"]["folds"],
                                                          "%.4f" % f["ms_per_bin_edge_crossed"] if f["ms_per_bin_edge_crossed"] is not None else "-",
                                                          f["bin_edges_crossed"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(side=side, steps=steps, period=PERIOD, repeats=args.repeats, precision=args.precision, host_threads=THREADS, cases=cases),
                      f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if all(c["bytewise_equal"] and c["not_zeros"] for c in cases.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

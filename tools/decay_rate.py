#!/usr/bin/env python3
"""What a decay map costs: seconds of a box room with a source while the squared field of a box is summed into time bins over a run,
the way it had to be done before wv_set_decay (a snapshot plan, fetch_snapshots, `E[b] = E[b] + p * p` in NumPy on the host -- timed
to the finished bins) against a decay plan (the engine folds on the device; fetch_decay brings n_bins doubles per node).  One
invocation, the ways alternating, three repeats each; every repeat starts from the same checkpoint, so old and new capture the same
steps and their bins are compared byte for byte.

    python tools/decay_rate.py [--side 512] [--steps 240] [--precision f64] [--bin-captures 16] [--json FILE]

boxes:   plane   one full z-plane
         field   the whole field decimated by 4 on every axis
each at  period 3 (every pass stays a three-step pass) and period 1 (every step ends a pass)
ways:    a       snapshot plan + fetch_snapshots + the NumPy accumulation (on up to 16 threads, split along the nodes: the sums are
                 elementwise)
         b       decay plan + fetch_decay
The bar, in every row: b takes fewer seconds than a by more than the spread of a's three repeats.

    python tools/decay_rate.py --bands 1,4,8 [--side 256] [--steps 240] [--json FILE]

What the band filters of a banded decay plan (wv_set_decay_bands) cost instead: steps per second of the same room over one full
z-plane with no plan, a plain decay plan and a banded plan of K octave bands (four sections each) for every K given, at period 1 and
period 3, the plans alternating, three repeats each; the fold kernel's mean time from a further repeat with kernel timing on; and per
K and period the bins against decay.banded_bins over the snapshots of the same plan, byte for byte.  No bar: figures."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import decay as D, engine as E, mesh as M  # noqa: E402

PERIODS = (3, 1)
THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))


def host_bins(snaps, n_bins, bin_captures, pool):
    """The definition (include/wayverb_amd.h), in capture order: E[min(j // W, n_bins - 1)] += p_j * p_j on float64 arrays."""
    n = snaps.shape[0]
    flat = snaps.reshape(n, -1)
    out = np.zeros((n_bins, flat.shape[1]))
    bounds = np.linspace(0, flat.shape[1], THREADS + 1).astype(np.int64)

    def part(i):
        lo, hi = int(bounds[i]), int(bounds[i + 1])
        for j in range(n):
            b = min(j // bin_captures, n_bins - 1)
            p = flat[j, lo:hi].astype(np.float64)
            out[b, lo:hi] = out[b, lo:hi] + p * p

    list(pool.map(part, range(THREADS)))
    return out.reshape((n_bins,) + snaps.shape[1:])


def timed_rows(eng, side, steps, bin_captures, pool):
    """{row: [seconds per repeat]}, {row: bins of the last repeat}, {row: fold launches of the last repeat}"""
    start = eng.step_count()
    boxes = {"plane": dict(box=((0, 0, side // 2), (None, None, 1))), "field": dict(box="mesh", stride=4)}
    seconds, bins, folds = {}, {}, {}

    def repeat(row, body, before):
        eng.rollback()
        assert eng.step_count() == start
        before()    # (a plan is set once per run: its memory is allocated outside the timed region, as the engine itself is)
        eng.synchronize()
        t0 = time.perf_counter()
        out = body()
        seconds.setdefault(row, []).append(time.perf_counter() - t0)
        assert eng.step_count() == start + steps
        bins[row] = out

    for _ in range(3):   # old and new alternate within every round
        for name, box in boxes.items():
            for period in PERIODS:
                captures = steps // period
                n_bins = -(-captures // bin_captures)
                row = "%s every %d" % (name, period)

                def old():
                    assert eng.run_steps(steps) == (steps, 0)
                    snaps, at = eng.fetch_snapshots()
                    assert list(at) == list(range(start + period, start + steps + 1, period))
                    return host_bins(snaps, n_bins, bin_captures, pool)

                def new():
                    assert eng.run_steps(steps) == (steps, 0)
                    out, count = eng.fetch_decay()
                    assert count == captures
                    folds[row] = eng.query(E.Engine.QUERY_DECAY_FOLDS)
                    return out

                repeat("a " + row, old, lambda: eng.set_snapshots(first_step=start + period, period=period, **box))
                eng.set_snapshots(None)
                repeat("b " + row, new, lambda: eng.set_decay(n_bins, bin_captures, first_step=start + period, period=period, **box))
                eng.set_decay(None)
    return seconds, bins, folds


def band_sections(k_bands, period):
    """K octave bands, 4th-order Butterworth band-passes, below 0.2 of the rate of the captured series (1 / period per step)."""
    return np.stack([D.butterworth_bandpass(lo, hi, 1.0 / period) for lo, hi in D.octave_band_edges([0.2 / period / 2 ** k for k in range(k_bands)])])


def band_rows(eng, side, steps, bin_captures, band_counts):
    """{row: [seconds per repeat]}, {row: (fold launches, mean fold ms, model bytes per fold)}, {row: bins equal the NumPy definition's}"""
    start = eng.step_count()
    box = dict(box=((0, 0, side // 2), (None, None, 1)))
    nodes = side * side
    seconds, folds, equal = {}, {}, {}

    def run(row, set_plan, timing=False):
        eng.rollback()
        set_plan()
        eng.enable_kernel_timing(timing)
        eng.synchronize()
        t0 = time.perf_counter()
        assert eng.run_steps(steps) == (steps, 0)
        out = eng.fetch_decay()[0] if eng.decay_shape is not None else None
        eng.synchronize()
        if not timing:
            seconds.setdefault(row, []).append(time.perf_counter() - t0)
        return out

    for period in PERIODS:
        captures = steps // period
        n_bins = -(-captures // bin_captures)
        plan = dict(first_step=start + period, period=period, **box)
        plans = [("none", None)] + [("plain", 0)] + [("bands %d" % k, k) for k in band_counts]
        for repeat in range(4):   # three timed rounds, the plans alternating within each; a fourth with kernel timing on
            for name, k in plans:
                row = "%s every %d" % (name, period)
                sections = band_sections(k, period) if k else None
                got = run(row, (lambda: None) if k is None else (lambda: eng.set_decay(n_bins, bin_captures, bands=sections, **plan)), timing=repeat == 3)
                if repeat == 3 and k is not None:
                    n, ns = eng.query(E.Engine.QUERY_DECAY_FOLDS), eng.query(E.Engine.QUERY_DECAY_NS)
                    r = -(-16 // bin_captures) + (1 if 16 % bin_captures else 0)   # bins a full stage of 16 captures touches at the most
                    model = nodes * k * (4 * 16 + 32 * 4 + 16 * r) if k else nodes * (4 * 16 + 16 * r)
                    folds[row] = dict(folds=n, mean_fold_ms=ns / 1e6 / n if n else 0.0, model_bytes_full_fold=model)
                eng.enable_kernel_timing(False)
                eng.set_decay(None)
                if repeat == 3 and k:
                    eng.rollback()
                    eng.set_snapshots(**plan)
                    assert eng.run_steps(steps) == (steps, 0)
                    snaps, _ = eng.fetch_snapshots()
                    eng.set_snapshots(None)
                    want = D.banded_bins(snaps, sections, n_bins, bin_captures)
                    equal[row] = bool(got.tobytes() == want.tobytes() and (want.reshape(k, -1).max(axis=1) > 0).all())
    return seconds, folds, equal


def bands_main(args):
    side, steps = args.side, args.steps
    band_counts = [int(k) for k in args.bands.split(",")]
    assert all(1 <= k <= 8 for k in band_counts)
    report = {"side": side, "steps": steps, "bin_captures": args.bin_captures, "bands": band_counts}
    for precision in args.precision.split(","):
        mesh = M.box_mesh(side, side, side, coefficients=M.bench_materials(), surface_of_face=[0, 1, 2, 3, 2, 3])
        eng = E.Engine(mesh, precision=precision)
        mesh.nodes = None
        try:
            sig = np.zeros(64 + steps)
            sig[0] = 1.0
            eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2, side // 2, side // 2), sig)
            eng.set_receivers([mesh.compute_index(side // 2 + 3, side // 2, side // 2)])
            assert eng.run_steps(48) == (48, 0)
            eng.checkpoint()
            seconds, folds, equal = band_rows(eng, side, steps, args.bin_captures, band_counts)
        finally:
            eng.close()
        print("%d^3 %s, plane z=%d (%d nodes), %d steps per repeat, %d captures per bin; steps per second (three repeats: min / median / max)"
              % (side, precision, side // 2, side * side, steps, args.bin_captures))
        rows = {}
        for row in seconds:
            s = sorted(steps / v for v in seconds[row])
            rows[row] = dict(steps_per_s_min=s[0], steps_per_s_median=s[1], steps_per_s_max=s[2], **folds.get(row, {}))
            f = folds.get(row)
            print("  %-18s %9.1f / %9.1f / %9.1f steps/s%s" % (row, s[0], s[1], s[2], "" if not f else
                  "; %d folds, mean %.4f ms, model %d bytes per full fold" % (f["folds"], f["mean_fold_ms"], f["model_bytes_full_fold"])), flush=True)
        for row in equal:
            print("  %s against decay.banded_bins over the snapshots: bins %s" % (row, "bytewise equal" if equal[row] else "DIFFER"), flush=True)
        report[precision] = dict(rows=rows, bytewise_equal=equal)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    ok = all(v for p in args.precision.split(",") for v in report[p]["bytewise_equal"].values())
    print("DECAY BANDS RATE %s" % ("OK" if ok else "BINS DIFFER"))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--steps", type=int, default=240, help="steps per repeat, a multiple of 3")
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--bin-captures", type=int, default=16)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--bands", metavar="K[,K...]", help="measure banded decay plans of K octave bands each (1 .. 8) against no plan and "
                                                       "a plain one, on one plane, instead of the comparison above")
    args = ap.parse_args()
    assert args.steps % 3 == 0 and args.bin_captures >= 1
    if args.bands:
        return bands_main(args)
    side, steps = args.side, args.steps
    report = {"side": side, "steps": steps, "bin_captures": args.bin_captures, "host_threads": THREADS}
    precisions = args.precision.split(",")
    with ThreadPoolExecutor(THREADS) as pool:
        for precision in precisions:
            mesh = M.box_mesh(side, side, side, coefficients=M.bench_materials(), surface_of_face=[0, 1, 2, 3, 2, 3])
            eng = E.Engine(mesh, precision=precision)
            mesh.nodes = None
            try:
                sig = np.zeros(64 + steps)
                sig[0] = 1.0
                eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2, side // 2, side // 2), sig)
                eng.set_receivers([mesh.compute_index(side // 2 + 3, side // 2, side // 2)])
                assert eng.run_steps(48) == (48, 0)     # warm-up: passes set up, the wave front well inside the box
                eng.checkpoint()
                seconds, bins, folds = timed_rows(eng, side, steps, args.bin_captures, pool)
            finally:
                eng.close()
            print("%d^3 %s, %d steps per repeat, %d captures per bin; seconds (three repeats: min / median / max)"
                  % (side, precision, steps, args.bin_captures))
            rows, verdicts = {}, {}
            for row in sorted(seconds):
                s = sorted(seconds[row])
                rows[row] = dict(seconds_min=s[0], seconds_median=s[1], seconds_max=s[2])
                print("  %-18s %8.4f / %8.4f / %8.4f s" % (row, s[0], s[1], s[2]), flush=True)
            for row in sorted(r[2:] for r in seconds if r.startswith("a ")):
                old, new = rows["a " + row], rows["b " + row]
                same = bins["a " + row].tobytes() == bins["b " + row].tobytes() and np.abs(bins["b " + row]).max() > 0
                spread = old["seconds_max"] - old["seconds_min"]
                gain = old["seconds_median"] - new["seconds_median"]
                verdicts[row] = dict(bytewise_equal_to_old=bool(same), seconds_saved=gain, spread_of_old=spread,
                                     beats_old_by_more_than_its_spread=bool(gain > spread), folds=folds[row])
                print("  b %s against a: bins %s, %.4f s fewer at a spread of %.4f s (%s); %d fold launches"
                      % (row, "bytewise equal" if same else "DIFFER", gain, spread, "beats it" if gain > spread else "DOES NOT beat it", folds[row]),
                      flush=True)
            report[precision] = dict(rows=rows, verdicts=verdicts)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    ok = all(v["bytewise_equal_to_old"] and v["beats_old_by_more_than_its_spread"] for p in precisions for v in report[p]["verdicts"].values())
    print("DECAY RATE %s" % ("OK" if ok else "BAR MISSED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

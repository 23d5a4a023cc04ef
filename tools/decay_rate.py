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
The bar, in every row: b takes fewer seconds than a by more than the spread of a's three repeats."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import engine as E, mesh as M  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--steps", type=int, default=240, help="steps per repeat, a multiple of 3")
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--bin-captures", type=int, default=16)
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    assert args.steps % 3 == 0 and args.bin_captures >= 1
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

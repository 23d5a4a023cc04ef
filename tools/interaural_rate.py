#!/usr/bin/env python3
"""What interaural maps cost: steps per second of a box room with a source while, for every seat of a box, the field at two nodes an
ear-distance apart is correlated at lags of up to +-L captures per time bin over a run, the way it had to be done before
wv_set_interaural (a snapshot plan of the hull of both ear planes, fetch_snapshots, the NumPy twin interaural.interaural_fold on the
host -- timed to the finished bins) against an interaural plan (the engine folds on the device; fetch_interaural brings 20 + 8 n_bins
(2 L + 3) bytes per seat).  One invocation, the ways alternating, every repeat from the same checkpoint, so both ways capture the same
steps and their onsets, energies and bins are compared bytewise.

    python tools/interaural_rate.py [--side 512] [--steps 480] [--repeats 3] [--precision f64] [--json FILE]

cases (both at period 3, so that every pass stays a three-step pass; two bins, the edge at 40 captures):
       plane   one z-plane less two rows on either side in y, the ears two nodes either side of the seat along y
       field   the field decimated by 4 on every axis, the ears one stride (four nodes) either side along y
each at L = 8 and L = 16, without a filter and with a band-pass of two sections.
ways:  no plan
       snapshots + numpy    snapshot plan + fetch_snapshots + the NumPy twin (on up to 16 threads, split along the seats)
       interaural plan      wv_set_interaural + fetch_interaural
Then, with kernel timing on: the fold kernel's time per capture and seat."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import engine as E, interaural as IA, mesh as M  # noqa: E402

PERIOD = 3
EDGES = [0, 40]
THRESHOLD = 1e-7
THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))
WAYS = ("no plan", "snapshots + numpy", "interaural plan")
SECTIONS = np.array([[0.2, 0.0, -0.2, -1.5, 0.6], [0.3, 0.0, -0.3, -1.1, 0.5]])      # two band-pass sections, stable


def host_fold(a, b, L, sections, pool):
    """The definition (wayverb_amd/interaural.py), the seats split among the threads."""
    n = a.shape[0]
    fa, fb = a.reshape(n, -1), b.reshape(n, -1)
    bounds = np.linspace(0, fa.shape[1], THREADS + 1).astype(np.int64)
    parts = list(pool.map(lambda i: IA.interaural_fold(np.ascontiguousarray(fa[:, bounds[i]:bounds[i + 1]]), np.ascontiguousarray(fb[:, bounds[i]:bounds[i + 1]]),
                                                       THRESHOLD, EDGES, L, sections), range(THREADS)))
    return {k: np.concatenate([p[k] for p in parts], axis=-1) for k in ("onset", "pre", "bins")}


def measure(eng, side, steps, repeats, pool):
    start = eng.step_count()
    captures = steps // PERIOD
    # (the seats' box, its stride, the ears, the snapshot plan's hull box, and where the two ear planes lie in the hull's snapshots)
    cases = {
        "plane": (dict(box=((0, 2, side // 2), (None, side - 4, 1))), (0, -2, 0), (0, 2, 0), dict(box=((0, 0, side // 2), (None, None, 1))),
                  (slice(0, side - 4), slice(4, side))),
        "field": (dict(box=((0, 4, 0), (None, side - 8, None)), stride=4), (0, -4, 0), (0, 4, 0), dict(box="mesh", stride=4),
                  (slice(0, side // 4 - 2), slice(2, side // 4))),
    }
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

    for name, (box, ear_a, ear_b, hull, (ya, yb)) in cases.items():
        cadence = dict(first_step=start + PERIOD, period=PERIOD)
        for L in (8, 16):
            for sections in (None, SECTIONS):
                def old():
                    assert eng.run_steps(steps) == (steps, 0)
                    snaps, at = eng.fetch_snapshots()
                    assert list(at) == list(range(start + PERIOD, start + steps + 1, PERIOD))
                    return host_fold(snaps[:, :, ya], snaps[:, :, yb], L, sections, pool)

                def new():
                    assert eng.run_steps(steps) == (steps, 0)
                    got, count = eng.fetch_interaural()
                    assert count == captures
                    return got

                def set_plan():
                    eng.set_interaural(EDGES, ear_a, ear_b, L, THRESHOLD, sections, **cadence, **box)

                seconds = {way: [] for way in WAYS}
                maps = {}
                for _ in range(repeats):   # the ways alternate within every round
                    seconds["no plan"].append(repeat(plain)[0])
                    s, maps["old"] = repeat(old, lambda: eng.set_snapshots(**cadence, **hull))
                    seconds["snapshots + numpy"].append(s)
                    eng.set_snapshots(None)
                    s, maps["new"] = repeat(new, set_plan)
                    seconds["interaural plan"].append(s)
                    eng.set_interaural(None)
                shape = maps["new"]["onset"].shape
                # (the host's parts lie seat after seat along one last axis, in the box's own order)
                same = all(maps["new"][k].tobytes() == np.ascontiguousarray(maps["old"][k]).tobytes() for k in ("onset", "pre", "bins"))
                # the fold kernel's own time, from the engine's events
                eng.enable_kernel_timing(True)
                eng.rollback()
                set_plan()
                assert eng.run_steps(steps) == (steps, 0)
                eng.fetch_interaural()
                folds, ns = eng.query(E.Engine.QUERY_INTERAURAL_FOLDS), eng.query(E.Engine.QUERY_INTERAURAL_NS)
                eng.set_interaural(None)
                eng.enable_kernel_timing(False)
                nodes = int(np.prod(shape))
                out["%s L=%d %s" % (name, L, "two sections" if sections is not None else "no filter")] = dict(
                    case=name, L=L, n_sections=0 if sections is None else 2, captures=captures, nodes=nodes,
                    seconds={way: sorted(s) for way, s in seconds.items()},
                    steps_per_second={way: steps / sorted(s)[len(s) // 2] for way, s in seconds.items()},
                    bytewise_equal=bool(same), not_zeros=bool(np.abs(maps["new"]["bins"]).max() > 0),
                    fold=dict(folds=folds, total_ms=ns * 1e-6, ms_per_capture=ns * 1e-6 / captures, ps_per_capture_and_seat=ns * 1e3 / captures / nodes))
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
    if args.side % 4 or args.side < 32:
        ap.error("--side must be a multiple of 4, 32 at the least")
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
        print("  %s: %d seats, %d captures" % (name, c["nodes"], c["captures"]))
        for way in WAYS:
            print("    %-18s %9.1f steps/s" % (way, c["steps_per_second"][way]))
        print("    maps of the two ways: %s" % ("bytewise equal" if c["bytewise_equal"] and c["not_zeros"] else "DIFFER"))
        print("    fold kernel: %.4f ms per capture (%d folds), %.2f ps per capture and seat" % (c["fold"]["ms_per_capture"], c["fold"]["folds"],
                                                                                                 c["fold"]["ps_per_capture_and_seat"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(side=side, steps=steps, period=PERIOD, repeats=args.repeats, precision=args.precision, host_threads=THREADS, cases=cases),
                      f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if all(c["bytewise_equal"] and c["not_zeros"] for c in cases.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

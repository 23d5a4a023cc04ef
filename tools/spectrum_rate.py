#!/usr/bin/env python3
"""What a spectrum of the field costs: steps per second of a box room with a source while a box of the field is Fourier-transformed at
K frequencies over a run, the way it had to be done before wv_set_spectrum (a snapshot plan, fetch_snapshots, the Fourier sums in
NumPy on the host -- timed to the finished spectrum) against a spectrum plan (the engine folds on the device; fetch_spectrum brings
K complex fields).  fp64 and fp32, one invocation, the ways alternating, three repeats each; every repeat starts from the same
checkpoint, so old and new capture the same steps and their spectra are compared bit for bit.

    python tools/spectrum_rate.py [--side 512] [--steps 480] [--precision f64,f32] [--json FILE]

cases (both at period 3, so that every pass stays a three-step pass):
       plane   one full z-plane, K = 64
       field   the whole field decimated by 4 on every axis, K = 16
ways:  a       no plan
       b       snapshot plan + fetch_snapshots + the NumPy fold (on up to 16 threads, split along the nodes: the sums are elementwise)
       c       spectrum plan + fetch_spectrum"""
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
THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))


def host_fold(snaps, steps, freqs, pool):
    """The definition (include/wayverb_amd.h), in capture order: re[k] = re[k] + p * c, im[k] = im[k] - p * s on float64 arrays."""
    n, K = snaps.shape[0], len(freqs)
    tw = np.array([[E.spectrum_twiddle(f, int(s)) for f in freqs] for s in steps])      # [n][K][2]
    flat = snaps.reshape(n, -1)
    out = np.empty((K, flat.shape[1]), dtype=np.complex128)
    bounds = np.linspace(0, flat.shape[1], THREADS + 1).astype(np.int64)

    def part(i):
        lo, hi = int(bounds[i]), int(bounds[i + 1])
        re, im = np.zeros((K, hi - lo)), np.zeros((K, hi - lo))
        for j in range(n):
            p = flat[j, lo:hi].astype(np.float64)
            for k in range(K):
                re[k] = re[k] + p * tw[j, k, 0]
                im[k] = im[k] - p * tw[j, k, 1]
        out.real[:, lo:hi], out.imag[:, lo:hi] = re, im

    list(pool.map(part, range(THREADS)))
    return out.reshape((K,) + snaps.shape[1:])


def timed_rows(eng, side, steps, pool):
    """{row: [seconds per repeat]}, {row: spectrum of the last repeat}"""
    start = eng.step_count()
    cases = {"plane": (dict(box=((0, 0, side // 2), (None, None, 1))), list(np.linspace(0.0, 0.5 / PERIOD, 64))),
             "field": (dict(box="mesh", stride=4), list(np.linspace(0.0, 0.5 / PERIOD, 16)))}
    seconds, spectra = {}, {}

    def repeat(row, body, before=None):
        eng.rollback()
        assert eng.step_count() == start
        if before:
            before()    # (a plan is set once per run: its memory is allocated outside the timed region, as the engine itself is)
        eng.synchronize()
        t0 = time.perf_counter()
        out = body()
        seconds.setdefault(row, []).append(time.perf_counter() - t0)
        assert eng.step_count() == start + steps
        spectra[row] = out

    def plain():
        assert eng.run_steps(steps) == (steps, 0)

    for _ in range(3):   # the ways alternate within every round
        repeat("a", plain)
        for name, (box, freqs) in cases.items():
            def old():
                assert eng.run_steps(steps) == (steps, 0)
                snaps, at = eng.fetch_snapshots()
                assert list(at) == list(range(start + PERIOD, start + steps + 1, PERIOD))
                return host_fold(snaps, at, freqs, pool)

            def new():
                assert eng.run_steps(steps) == (steps, 0)
                out, captures = eng.fetch_spectrum()
                assert captures == steps // PERIOD
                return out

            repeat("b " + name, old, lambda: eng.set_snapshots(first_step=start + PERIOD, period=PERIOD, **box))
            eng.set_snapshots(None)
            repeat("c " + name, new, lambda: eng.set_spectrum(freqs, first_step=start + PERIOD, period=PERIOD, **box))
            eng.set_spectrum(None)
    return seconds, spectra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--steps", type=int, default=480, help="steps per repeat, a multiple of 3")
    ap.add_argument("--precision", default="f64,f32")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    assert args.steps % PERIOD == 0
    side, steps = args.side, args.steps
    report = {"side": side, "steps": steps, "period": PERIOD, "host_threads": THREADS}
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
                seconds, spectra = timed_rows(eng, side, steps, pool)
                triples = eng.query(E.Engine.QUERY_TRIPLE_PASSES)
            finally:
                eng.close()
            print("%d^3 %s, %d steps per repeat, a capture every %d steps; seconds and steps/s (three repeats: min / median / max); "
                  "%d three-step passes in all" % (side, precision, steps, PERIOD, triples))
            rows = {}
            for row in sorted(seconds):
                s = sorted(seconds[row])
                rows[row] = dict(seconds_min=s[0], seconds_median=s[1], seconds_max=s[2], steps_per_s_median=steps / s[1])
                print("  %-8s %8.4f / %8.4f / %8.4f s   %9.1f / %9.1f / %9.1f steps/s"
                      % (row, s[0], s[1], s[2], steps / s[2], steps / s[1], steps / s[0]), flush=True)
            verdicts = {}
            for name in ("plane", "field"):
                old, new = rows["b " + name], rows["c " + name]
                same = spectra["b " + name].tobytes() == spectra["c " + name].tobytes() and np.abs(spectra["c " + name]).max() > 0
                spread = old["seconds_max"] - old["seconds_min"]
                gain = old["seconds_median"] - new["seconds_median"]
                verdicts[name] = dict(bitwise_equal_to_old=bool(same), seconds_saved=gain, spread_of_old=spread,
                                      beats_old_by_more_than_its_spread=bool(gain > spread),
                                      c_over_a=rows["a"]["seconds_median"] / new["seconds_median"])
                print("  c %s against b %s: spectrum %s, %.4f s fewer at a spread of %.4f s (%s); c runs at %.3f of row a's steps/s"
                      % (name, name, "bitwise equal" if same else "DIFFERS", gain, spread, "beats it" if gain > spread else "DOES NOT beat it",
                         verdicts[name]["c_over_a"]), flush=True)
            report[precision] = dict(rows=rows, verdicts=verdicts)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    ok = all(v["bitwise_equal_to_old"] and v["beats_old_by_more_than_its_spread"] for p in precisions for v in report[p]["verdicts"].values())
    print("SPECTRUM RATE %s" % ("OK" if ok else "BAR MISSED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What an intensity map costs: steps per second of a box room with a source while the sound intensity over one z-plane (less its
rim) is summed into time bins, three ways, alternating, three repeats each, every repeat from the same state:

    no plan              the run alone
    plan every 1 / 3     wv_set_intensity (the engine gathers and folds on the device; fetch_intensity brings 4 n_bins doubles per node)
    receivers every 1    the way it had to be done before: a directional receiver at every node of the plane
                         (wv_set_directional_receivers, a 16-byte record per node and step over the link), summed per bin on the host

    python tools/intensity_rate.py [--side 256] [--steps 240] [--precision f64] [--bin-captures 16] [--json FILE]

A further repeat per plan with kernel timing on gives the fold's and the gather's mean kernel time beside the traffic model
B (16 t + 48 + 64 r) of a full fold; and, untimed, the ways are held to equal bytes where they are defined to agree: the plan's bins
and velocities against intensity.intensity_bins over snapshots of the plane's hull, its E planes against a plain decay plan's bins,
its velocities against the velocities the receiver path carries.  (The receiver path's sums are sums of products rounded to float:
close to the plan's bins, not equal; the largest relative difference is reported.)

The bar: the plan at period 1 takes fewer seconds than the receivers by more than the spread of the latter's three repeats.  Also
reported: whether the plan at period 3 costs less than at period 1."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import engine as E, intensity as I, mesh as M  # noqa: E402

SPACING, DENSITY, SPEED = 0.05, 1.225, 340.0
RATE = SPEED * np.sqrt(3.0) / SPACING


def measure(eng, mesh, side, steps, bin_captures):
    start = eng.step_count()
    z = side // 4                                               # (clear of the source node at side / 2: the receiver path reads that node with its sample in)
    box = ((1, 1, z), (side - 2, side - 2, 1))
    nodes = (side - 2) * (side - 2)
    centres = [mesh.compute_index(x, y, z) for y in range(1, side - 1) for x in range(1, side - 1)]
    plain_recv = [mesh.compute_index(side // 2 + 3, side // 2, side // 2)]
    seconds, kernels, bytewise, figures = {}, {}, {}, {}

    def const(period):
        return dict(spacing=SPACING, sample_rate=RATE / period, ambient_density=DENSITY)

    def fresh(receivers=None):
        """Back to the state after the warm-up; the receivers changed where asked (a checkpoint is taken with the set it will see)."""
        eng.rollback()
        if receivers is not None:
            if receivers == "directional":
                eng.set_directional_receivers(centres, SPACING, RATE, DENSITY)
            else:
                eng.set_receivers(plain_recv)
            eng.checkpoint()
        assert eng.step_count() == start

    def plan_run(period, n_steps, timing=False, first_step=None):
        captures = n_steps // period + (1 if first_step == start else 0)
        n_bins = max(1, -(-captures // bin_captures))
        eng.set_intensity(n_bins, bin_captures, box=box, period=period, first_step=start + period if first_step is None else first_step, **const(period))
        eng.enable_kernel_timing(timing)
        eng.synchronize()
        t0 = time.perf_counter()
        assert eng.run_steps(n_steps) == (n_steps, 0)
        bins, count = eng.fetch_intensity()
        took = time.perf_counter() - t0
        assert count == captures
        return bins, took

    for repeat in range(3):
        fresh()
        eng.synchronize()
        t0 = time.perf_counter()
        assert eng.run_steps(steps) == (steps, 0)
        eng.synchronize()
        seconds.setdefault("no plan", []).append(time.perf_counter() - t0)
        for period in (1, 3):
            fresh()
            seconds.setdefault("plan every %d" % period, []).append(plan_run(period, steps)[1])
            eng.set_intensity(None)
        fresh("directional")
        n_bins = -(-steps // bin_captures)
        eng.synchronize()
        t0 = time.perf_counter()
        assert eng.run_steps(steps) == (steps, 0)
        records = eng.fetch_directional(start, steps)
        sums = np.zeros((4, n_bins, nodes))
        for j in range(steps):
            b = min(j // bin_captures, n_bins - 1)
            p = records["pressure"][j].astype(np.float64)
            sums[:3, b] = sums[:3, b] + records["intensity"][j].astype(np.float64).T
            sums[3, b] = sums[3, b] + p * p
        seconds.setdefault("receivers every 1", []).append(time.perf_counter() - t0)
        receiver_velocity = eng.fetch_directional_velocity(len(centres))
        fresh("plain")
    # kernel timing, a repeat of its own per period
    for period in (1, 3):
        fresh()
        plan_run(period, steps, timing=True)
        folds, fold_ns = eng.query(E.Engine.QUERY_INTENSITY_FOLDS), eng.query(E.Engine.QUERY_INTENSITY_NS)
        gathers, gather_ns = eng.query(E.Engine.QUERY_INTENSITY_GATHERS), eng.query(E.Engine.QUERY_INTENSITY_GATHER_NS)
        r = -(-16 // bin_captures) + (1 if 16 % bin_captures else 0)   # bins a full stage of 16 captures touches at the most
        kernels[period] = dict(fold=dict(launches=folds, mean_ms=fold_ns / 1e6 / folds if folds else 0.0, model_bytes=nodes * (16 * 16 + 48 + 64 * r)),
                               gather=dict(launches=gathers, mean_ms=gather_ns / 1e6 / gathers if gathers else 0.0,
                                           model_bytes=nodes * 16 + 3 * side * side * np.dtype(eng.dtype).itemsize))
        eng.enable_kernel_timing(False)
        eng.set_intensity(None)
    # the ways against each other, untimed: the captures of steps start .. start + steps - 1 (the steps the receivers record)
    fresh()
    bins, _ = plan_run(1, steps - 1, first_step=start)
    velocity = eng.fetch_intensity_velocity()
    eng.set_intensity(None)
    n_bins = bins.shape[1]
    fresh()
    eng.set_decay(n_bins, bin_captures, box=box, period=1, first_step=start)
    assert eng.run_steps(steps - 1) == (steps - 1, 0)
    decay = eng.fetch_decay()[0]
    eng.set_decay(None)
    fresh()
    hull, box_in_hull = I.hull_box((box[0], (side - 2, side - 2, 1)))
    eng.set_snapshots(box=hull, period=1, first_step=start)
    assert eng.run_steps(steps - 1) == (steps - 1, 0)
    snaps, _ = eng.fetch_snapshots()
    eng.set_snapshots(None)
    want, want_v = I.intensity_bins(snaps, box_in_hull, SPACING, RATE, DENSITY, n_bins, bin_captures, return_velocity=True)
    live = all(np.abs(bins[a]).max() > 0 for a in range(4))
    bytewise["plan against intensity_bins over hull snapshots (bins and velocities)"] = bool(
        live and bins.tobytes() == want.tobytes() and velocity.tobytes() == want_v.tobytes())
    bytewise["plan's E planes against a decay plan's bins"] = bool(live and bins[3].tobytes() == decay.tobytes())
    bytewise["plan's velocities against the receiver path's"] = bool(
        np.abs(receiver_velocity).max() > 0 and velocity.reshape(3, -1).T.tobytes() == receiver_velocity.tobytes())
    scale = np.abs(bins[:3]).max()
    figures["receiver sums against plan bins, largest difference over largest bin"] = float(np.abs(sums[:3].reshape(bins[:3].shape) - bins[:3]).max() / scale)
    return seconds, kernels, bytewise, figures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--steps", type=int, default=240, help="steps per repeat, a multiple of 3")
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--bin-captures", type=int, default=16)
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    assert args.steps % 3 == 0 and args.bin_captures >= 1 and args.side >= 16
    side, steps = args.side, args.steps
    report = {"side": side, "steps": steps, "bin_captures": args.bin_captures}
    precisions = args.precision.split(",")
    ok = True
    for precision in precisions:
        mesh = M.box_mesh(side, side, side, coefficients=M.bench_materials(), surface_of_face=[0, 1, 2, 3, 2, 3])
        eng = E.Engine(mesh, precision=precision)
        try:
            sig = np.zeros(64 + steps)
            sig[0] = 1.0
            eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2, side // 2, side // 2), sig)
            eng.set_receivers([mesh.compute_index(side // 2 + 3, side // 2, side // 2)])
            assert eng.run_steps(48) == (48, 0)     # warm-up: passes set up, the wave front well inside the box
            eng.checkpoint()
            seconds, kernels, bytewise, figures = measure(eng, mesh, side, steps, args.bin_captures)
        finally:
            eng.close()
        print("%d^3 %s, plane z=%d (%d nodes), %d steps per repeat, %d captures per bin; seconds (three repeats: min / median / max)"
              % (side, precision, side // 4, (side - 2) ** 2, steps, args.bin_captures))
        rows = {}
        for row in seconds:
            s = sorted(seconds[row])
            rows[row] = dict(seconds_min=s[0], seconds_median=s[1], seconds_max=s[2], steps_per_s_median=steps / s[1])
            print("  %-18s %8.4f / %8.4f / %8.4f s  (%9.1f steps/s)" % (row, s[0], s[1], s[2], steps / s[1]), flush=True)
        for period, k in kernels.items():
            for name in ("fold", "gather"):
                print("  plan every %d: %d %s launches, mean %.4f ms, model %d bytes" % (period, k[name]["launches"], name, k[name]["mean_ms"], k[name]["model_bytes"]))
        for what, same in bytewise.items():
            print("  %s: %s" % (what, "bytewise equal" if same else "DIFFER"), flush=True)
        for what, value in figures.items():
            print("  %s: %.3g" % (what, value))
        old, new = rows["receivers every 1"], rows["plan every 1"]
        spread, gain = old["seconds_max"] - old["seconds_min"], old["seconds_median"] - new["seconds_median"]
        verdict = dict(seconds_saved=gain, spread_of_receivers=spread, beats_receivers_by_more_than_their_spread=bool(gain > spread),
                       period_3_costs_less_than_period_1=bool(rows["plan every 3"]["seconds_median"] < new["seconds_median"]))
        print("  plan every 1 against receivers every 1: %.4f s fewer at a spread of %.4f s (%s); plan every 3 %s than plan every 1"
              % (gain, spread, "beats it" if gain > spread else "DOES NOT beat it", "costs less" if verdict["period_3_costs_less_than_period_1"] else "costs NO less"))
        report[precision] = dict(rows=rows, fold=kernels[1]["fold"], gather=kernels[1]["gather"], kernels_every_3=kernels[3], bytewise=bytewise,
                                 figures=figures, verdict=verdict)
        ok = ok and all(bytewise.values()) and verdict["beats_receivers_by_more_than_their_spread"]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    print("INTENSITY RATE %s" % ("OK" if ok else "BAR MISSED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

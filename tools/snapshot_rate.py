#!/usr/bin/env python3
"""What watching a run costs: steps per second of a box room with a source while part of the field is recorded every k steps, the way
it had to be done before wv_set_snapshots (wv_run k steps, wv_read_planes, repeat) against a snapshot plan (the engine captures on the
device behind the pass and copies on a stream of its own).  fp64 and fp32, one invocation, old and new alternating, three repeats each;
every repeat starts from the same checkpoint, so old and new record the same steps and their output is compared bit for bit.

    python tools/snapshot_rate.py [--side 512] [--steps 480] [--json FILE]

rows:  a          no snapshots
       b k=K      wv_run K steps + wv_read_planes of one z-plane as floats        (K = 1, 4, 16)
       c k=K      a plan for the same plane and the same K
       d old/new  the whole field decimated by 4 on every axis, every 16 steps"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import engine as E, mesh as M  # noqa: E402


def timed_rows(eng, side, steps):
    """{row: [steps/s per repeat]}, {row: recorded output of the last repeat}"""
    z = side // 2
    start = eng.step_count()
    rates, recorded = {}, {}

    def repeat(row, body, before=None):
        eng.rollback()
        assert eng.step_count() == start
        if before:
            before()    # (a plan is set once per run: its ring is allocated outside the timed region, as the engine itself is)
        eng.synchronize()
        t0 = time.perf_counter()
        out = body()
        dt = time.perf_counter() - t0
        assert eng.step_count() == start + steps
        rates.setdefault(row, []).append(steps / dt)
        recorded[row] = out

    def plain():
        assert eng.run_steps(steps) == (steps, 0)

    def stop_and_read(k, whole):
        def body():
            out = []
            for _ in range(steps // k):
                assert eng.run_steps(k) == (k, 0)
                if whole:
                    out.append(np.ascontiguousarray(eng.read_planes(0, side, dtype=np.float32)[::4, ::4, ::4]))
                else:
                    out.append(eng.read_planes(z, 1, dtype=np.float32))
            return np.stack(out)
        return body

    def plan(k, whole):
        def before():
            if whole:
                eng.set_snapshots(box="mesh", stride=4, first_step=start + k, period=k)
            else:
                eng.set_snapshots(box=((0, 0, z), (None, None, 1)), first_step=start + k, period=k)
        return before

    def planned(k):
        def body():
            assert eng.run_steps(steps) == (steps, 0)
            out, at = eng.fetch_snapshots()
            assert list(at) == list(range(start + k, start + steps + 1, k))
            return out
        return body

    for _ in range(3):   # old and new alternate within every round
        repeat("a", plain)
        for k in (1, 4, 16):
            repeat("b k=%d" % k, stop_and_read(k, False))
            repeat("c k=%d" % k, planned(k), plan(k, False))
            eng.set_snapshots(None)
        repeat("d old", stop_and_read(16, True))
        repeat("d new", planned(16), plan(16, True))
        eng.set_snapshots(None)
    return rates, recorded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--steps", type=int, default=480, help="steps per repeat, a multiple of 16 (480: windows of 0.1 - 0.2 s, long against the host's jitter)")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    assert args.steps % 16 == 0
    side, steps = args.side, args.steps
    report = {"side": side, "steps": steps}
    for precision in ("f64", "f32"):
        mesh = M.box_mesh(side, side, side, coefficients=M.bench_materials(), surface_of_face=[0, 1, 2, 3, 2, 3])
        eng = E.Engine(mesh, precision=precision)
        mesh.nodes = None
        try:
            sig = np.zeros(64 + steps)
            sig[0] = 1.0
            eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2, side // 2, side // 2), sig)
            eng.set_receivers([mesh.compute_index(side // 2 + 3, side // 2, side // 2)])
            assert eng.run_steps(48) == (48, 0)     # warm-up: passes set up, the wave front well inside the recorded plane
            eng.checkpoint()
            rates, recorded = timed_rows(eng, side, steps)
        finally:
            eng.close()
        print("%d^3 %s, %d steps per repeat, steps/s (three repeats: min / median / max)" % (side, precision, steps))
        rows = {}
        for row in sorted(rates):
            r = sorted(rates[row])
            rows[row] = dict(min=r[0], median=r[1], max=r[2])
            print("  %-8s %9.1f / %9.1f / %9.1f" % (row, r[0], r[1], r[2]), flush=True)
        verdicts = {}
        for old, new in [("b k=%d" % k, "c k=%d" % k) for k in (1, 4, 16)] + [("d old", "d new")]:
            same = recorded[old].tobytes() == recorded[new].tobytes() and np.abs(recorded[new]).max() > 0
            spread = rows[old]["max"] - rows[old]["min"]
            gain = rows[new]["median"] - rows[old]["median"]
            verdicts[new] = dict(bitwise_equal_to_old=bool(same), gain_steps_per_s=gain, spread_of_old=spread,
                                 beats_old_by_more_than_its_spread=bool(gain > spread), share_of_a=rows[new]["median"] / rows["a"]["median"])
            print("  %s against %s: output %s, %+.1f steps/s at a spread of %.1f (%s), %.3f of row a"
                  % (new, old, "bitwise equal" if same else "DIFFERS", gain, spread, "beats it" if gain > spread else "DOES NOT beat it",
                     verdicts[new]["share_of_a"]), flush=True)
        report[precision] = dict(rows=rows, verdicts=verdicts)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    ok = all(v["bitwise_equal_to_old"] and v["beats_old_by_more_than_its_spread"] for p in ("f64", "f32") for v in report[p]["verdicts"].values())
    print("SNAPSHOT RATE %s" % ("OK" if ok else "BAR MISSED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

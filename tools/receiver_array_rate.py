#!/usr/bin/env python3
"""What a room full of listeners costs: steps per second of a 256^3 fp64 box (the bench's walls, a hard source) with R = 1, 10, 100, 1000
directional receivers at seeded inside nodes, the way it had to be done before receiver arrays -- the 7 R columns through
wv_set_receivers (above 64 of them one wave gathers them all), the raw columns to the host, postprocess.directional_receiver per
receiver in Python -- against wv_set_directional_receivers (the gather spread over the chip, the integrator on the device).

    python tools/receiver_array_rate.py --old-lib <libwayverb_amd.so of the commit before receiver arrays> [--side 256] [--steps 480]

Old and new alternate, three repeats each.  Two libraries with the same symbols do not share a process, so every repeat of either is
a child process of its own (this script with --worker): engine, 48 warm-up steps, then R = 1, 10, 100, 1000 in turn, 480 timed steps
each -- the same steps of the same run in old and new, so every old / new pair of records is compared bit for bit (by SHA-256).
rows:  old run    wv_run alone, columns recorded
       old all    ... plus wv_fetch_receivers and the host integration of every receiver
       new        wv_run + wv_fetch_directional"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNTS = (1, 10, 100, 1000)


def worker(args):
    from wayverb_amd import engine as E
    if args.lib:
        # the library of an earlier commit lacks the entry points load_library() declares: let those names resolve to nothing
        class Tolerant(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if not name.startswith("wv_"):
                        raise
                    return type("Missing", (), {})()
        E.C.CDLL = Tolerant
        E._LIB_PATH = args.lib
    from wayverb_amd import mesh as M, postprocess as P
    side, steps = args.side, args.steps
    mesh = M.box_mesh(side, side, side, coefficients=M.bench_materials(), surface_of_face=[0, 1, 2, 3, 2, 3])
    eng = E.Engine(mesh, precision="f64")
    spacing, sample_rate, density = float(np.float32(0.0442)), 13333.0, 400.0 / 340.0
    rng = np.random.default_rng(11)
    xyz = rng.integers(2, side - 2, (max(COUNTS), 3))
    centres = [mesh.compute_index(int(x), int(y), int(z)) for x, y, z in xyz]
    out = {}
    try:
        sig = np.zeros(48 + steps * len(COUNTS))
        sig[0] = 1.0
        eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2, side // 2, side // 2), sig)
        eng.set_receivers(centres[:1])
        assert eng.run_steps(48) == (48, 0)      # warm-up: passes set up, the wave front on its way
        for n in COUNTS:
            first = eng.step_count()
            if args.mode == "old":
                cols = []
                for c in centres[:n]:
                    cols += [c] + list(mesh.compute_neighbors(c))
                eng.set_receivers(cols)
                eng.synchronize()
                t0 = time.perf_counter()
                assert eng.run_steps(steps) == (steps, 0)
                t1 = time.perf_counter()
                traces = eng.fetch_receivers(first, steps)
                records = np.stack([P.directional_receiver(traces[:, 7 * i:7 * i + 7], spacing, sample_rate, density) for i in range(n)], axis=1)
                t2 = time.perf_counter()
                out[str(n)] = dict(run=steps / (t1 - t0), all=steps / (t2 - t0))
            else:
                eng.set_directional_receivers(centres[:n], spacing, sample_rate, density)
                eng.synchronize()
                t0 = time.perf_counter()
                assert eng.run_steps(steps) == (steps, 0)
                records = eng.fetch_directional(first, steps)
                t1 = time.perf_counter()
                out[str(n)] = dict(all=steps / (t1 - t0), wide_gathers=eng.query(E.Engine.QUERY_WIDE_GATHERS),
                                   directional_launches=eng.query(E.Engine.QUERY_DIRECTIONAL_LAUNCHES))
            assert records.shape == (steps, n) and np.abs(records["pressure"]).max() > 0
            out[str(n)]["sha256"] = hashlib.sha256(np.ascontiguousarray(records).tobytes()).hexdigest()
    finally:
        eng.close()
    print("WORKER " + json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-lib", help="libwayverb_amd.so built from the commit before receiver arrays")
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--steps", type=int, default=480)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--mode", choices=["old", "new"], help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.old_lib or not os.path.exists(args.old_lib):
        ap.error("--old-lib: the library of the commit before receiver arrays is what `old` runs on")

    def child(mode):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--mode", mode, "--side", str(args.side), "--steps", str(args.steps)]
        if mode == "old":
            cmd += ["--lib", os.path.abspath(args.old_lib)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith("WORKER ")]
        if p.returncode != 0 or len(lines) != 1:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("the %s worker failed (exit status %d): nothing more is started" % (mode, p.returncode))
        return json.loads(lines[0][len("WORKER "):])

    runs = {"old": [], "new": []}
    for _ in range(3):       # old and new alternate
        for mode in ("old", "new"):
            runs[mode].append(child(mode))
    print("%d^3 f64, %d steps per repeat, steps/s (three repeats: min / median / max)" % (args.side, args.steps))
    report = {"side": args.side, "steps": args.steps, "rows": {}, "verdicts": {}}
    ok = True
    for n in COUNTS:
        rows = {"old run": sorted(r[str(n)]["run"] for r in runs["old"]), "old all": sorted(r[str(n)]["all"] for r in runs["old"]),
                "new": sorted(r[str(n)]["all"] for r in runs["new"])}
        for name, r in rows.items():
            print("  R = %4d  %-8s %9.1f / %9.1f / %9.1f" % (n, name, r[0], r[1], r[2]))
        hashes = {r[str(n)]["sha256"] for mode in runs for r in runs[mode]}
        same = len(hashes) == 1
        spread = rows["old run"][2] - rows["old run"][0]
        v = dict(records_bitwise_equal=same, spread_of_old=spread, new_minus_old_run=rows["new"][1] - rows["old run"][1],
                 new_minus_old_all=rows["new"][1] - rows["old all"][1], new_over_old_run=rows["new"][1] / rows["old run"][1],
                 new_over_old_all=rows["new"][1] / rows["old all"][1], wide_gathers=runs["new"][0][str(n)]["wide_gathers"],
                 directional_launches=runs["new"][0][str(n)]["directional_launches"])
        print("  R = %4d  records %s; new against old run %+.1f steps/s (x %.3f), against old all %+.1f (x %.3f), spread of old %.1f"
              % (n, "bitwise equal in all six runs" if same else "DIFFER", v["new_minus_old_run"], v["new_over_old_run"], v["new_minus_old_all"],
                 v["new_over_old_all"], spread), flush=True)
        report["rows"][str(n)] = {k: dict(min=r[0], median=r[1], max=r[2]) for k, r in rows.items()}
        report["verdicts"][str(n)] = v
        ok = ok and same
    # what must hold: the untouched path is untouched (R = 1: within old's own spread), and the array pays (R = 1000: beyond it)
    one, thousand = report["verdicts"]["1"], report["verdicts"]["1000"]
    held_1 = abs(one["new_minus_old_run"]) <= one["spread_of_old"]
    held_1000 = thousand["new_minus_old_run"] > thousand["spread_of_old"]
    print("  R = 1: new %s old's spread; R = 1000: new %s old (run alone) by more than its spread"
          % ("within" if held_1 else "OUTSIDE", "beats" if held_1000 else "DOES NOT beat"))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    ok = ok and held_1 and held_1000
    print("RECEIVER ARRAY RATE %s" % ("OK" if ok else "BAR MISSED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

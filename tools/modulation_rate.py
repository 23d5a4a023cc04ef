#!/usr/bin/env python3
"""What a modulation map costs: seconds of a box room with an impulse source over a run with no plan, with a banded decay plan
(wv_set_decay_bands: the yardstick -- the same capture, the same cascades, one bin accumulator in place of the Fourier sums) and with
a modulation plan (wv_set_modulation) of the same plane, bands and cadence.  One invocation, the ways alternating, `--repeats` repeats
each; every repeat starts from the same checkpoint.  Per plan, band count and period: seconds of the run (min / median / max) and the
cost per capture over the run without a plan, seconds of the fetch on its own, and from a further repeat with kernel timing on the
fold kernel's mean time beside the bytes the model gives for this run's folds (B n_bands (4 t + 32 S + 16 + 32 M) for
the modulation fold, B n_bands (4 t + 32 S + 16 r) for the banded decay fold).  For every band count and period the modulation plan's
energies and sums are compared byte for byte with modulation.modulation_fold over a snapshot plan's captures, on a strip of the plane
(--check-nodes nodes at the most: the NumPy definition is a Python loop).

    python tools/modulation_rate.py [--dims 1024,1024,64] [--steps 240] [--periods 1,3] [--bands 3,7] [--freqs 14] [--precision f64]
                                    [--repeats 5] [--check-nodes 65536] [--json FILE]

The box is the z-plane in the middle of the mesh.  No bar: figures."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import decay as D, engine as E, mesh as M, modulation as MOD  # noqa: E402

RATE = 12000.0             # the mesh's nominal rate, which turns the standard's modulation frequencies into cycles per step
DECAY = (3, 80)            # the yardstick: three bins of 80 captures
SECTIONS = 4


def fold_sizes(captures):
    """The engine folds when its stage of 16 is full, and what is left on the fetch."""
    return [16] * (captures // 16) + ([captures % 16] if captures % 16 else [])


def decay_model(nodes, n_bands, captures):
    out, c0 = [], 0
    for t in fold_sizes(captures):
        bins = {min(c // DECAY[1], DECAY[0] - 1) for c in range(c0, c0 + t)}
        out.append(nodes * n_bands * (4 * t + 32 * SECTIONS + 16 * len(bins)))
        c0 += t
    return out


def modulation_model(nodes, n_bands, n_freqs, captures):
    return [nodes * n_bands * (4 * t + 32 * SECTIONS + 16 + 32 * n_freqs) for t in fold_sizes(captures)]


def band_sections(n_bands):
    """Octave bands from 0.1 cycles per capture downwards (upper edge 0.141), four Butterworth sections each."""
    return np.stack([D.butterworth_bandpass(lo, hi, 1.0) for lo, hi in D.octave_band_edges([0.1 / 2 ** k for k in range(n_bands)])])


def rows_for(eng, dims, steps, period, n_bands, freqs, repeats):
    eng.rollback()                                          # (every case starts where the checkpoint stands)
    start = eng.step_count()
    plan = dict(box=((0, 0, dims[2] // 2), (None, None, 1)), first_step=start + period, period=period)
    captures, nodes, bands = steps // period, dims[0] * dims[1], band_sections(n_bands)
    setters = {"none": lambda: None, "decay bands": lambda: eng.set_decay(DECAY[0], DECAY[1], bands=bands, **plan),
               "modulation": lambda: eng.set_modulation(freqs, bands, **plan)}
    seconds, fetches, kernels, out = {k: [] for k in setters}, {k: [] for k in setters if k != "none"}, {}, None
    for repeat in range(repeats + 1):                      # the last repeat runs with kernel timing on and is not timed
        timing = repeat == repeats
        for name, set_plan in setters.items():             # the three alternate within every round
            eng.rollback()
            assert eng.step_count() == start
            set_plan()                                      # (a plan's memory is allocated outside the timed region, as the engine's is)
            eng.enable_kernel_timing(timing)
            eng.synchronize()
            t0 = time.perf_counter()
            assert eng.run_steps(steps) == (steps, 0)
            eng.synchronize()
            t1 = time.perf_counter()                        # the run; the fetch (with the fold of what is staged) is timed on its own
            if name == "decay bands":
                got, count = eng.fetch_decay()
            elif name == "modulation":
                got = eng.fetch_modulation()
                count = eng.modulation_count()[0]
            eng.synchronize()
            t2 = time.perf_counter()
            if not timing:
                seconds[name].append(t1 - t0)
                if name != "none":
                    fetches[name].append(t2 - t1)
            if name != "none":
                assert count == captures
                if timing:
                    decay = name == "decay bands"
                    folds = eng.query(E.Engine.QUERY_DECAY_FOLDS if decay else E.Engine.QUERY_MODULATION_FOLDS)
                    fold_ns = eng.query(E.Engine.QUERY_DECAY_NS if decay else E.Engine.QUERY_MODULATION_NS)
                    model = decay_model(nodes, n_bands, captures) if decay else modulation_model(nodes, n_bands, len(freqs), captures)
                    if folds != len(model):                 # (the model's bytes are then spread over the folds there were)
                        print("  every %d  %s: %d folds where the stage alone would make %d" % (period, name, folds, len(model)), flush=True)
                    mean_ms = fold_ns / 1e6 / folds
                    kernels[name] = dict(folds=folds, mean_fold_ms=mean_ms, fold_us_per_capture=fold_ns / 1e3 / captures,
                                         model_bytes_mean_fold=sum(model) / folds, model_tb_per_s=sum(model) / folds / (mean_ms * 1e-3) / 1e12,
                                         fetch_bytes=int(got.nbytes if decay else got[0].nbytes + got[1].nbytes))
                if name == "modulation":
                    out = got
            eng.enable_kernel_timing(False)
            eng.set_decay(None)
            eng.set_modulation(None, None)
    return seconds, fetches, kernels, out, plan, bands, captures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="1024,1024,64")
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--periods", default="1,3")
    ap.add_argument("--bands", default="3,7")
    ap.add_argument("--freqs", type=int, default=14)
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-nodes", type=int, default=65536)
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    dims = tuple(int(v) for v in args.dims.split(","))
    periods = [int(v) for v in args.periods.split(",")]
    band_counts = [int(v) for v in args.bands.split(",")]
    steps = args.steps
    assert len(dims) == 3 and all(steps % p == 0 for p in periods) and args.repeats >= 1 and 1 <= args.freqs <= 16
    assert all(1 <= k <= 8 for k in band_counts)
    hz = (MOD.STI_MODULATION_HZ + (16.0, 20.0))[:args.freqs]
    freqs = MOD.cycles_per_step(hz, RATE)
    report = {"dims": dims, "steps": steps, "repeats": args.repeats, "decay": DECAY, "sections": SECTIONS, "modulation_hz": hz}
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
            print("%dx%dx%d %s, plane z=%d (%d nodes), %d modulation frequencies, %d steps per repeat, %d repeats; seconds (min / median / max)"
                  % (dims + (precision, dims[2] // 2, dims[0] * dims[1], len(freqs), steps, args.repeats)), flush=True)
            report[precision] = {"rows": {}, "bytewise_equal": {}, "modulation_over_decay_bands": {}}
            for n_bands in band_counts:
                for period in periods:
                    seconds, fetches, kernels, out, plan, bands, captures = rows_for(eng, dims, steps, period, n_bands, freqs, args.repeats)
                    base = float(np.median(seconds["none"]))
                    rows = {}
                    for name, sec in seconds.items():
                        sec = sorted(sec)
                        key = "%s, %d bands every %d" % (name, n_bands, period)
                        rows[name] = dict(seconds_min=sec[0], seconds_median=float(np.median(sec)), seconds_max=sec[-1], captures=captures, **kernels.get(name, {}))
                        line = "  %-34s run %8.4f / %8.4f / %8.4f s" % (key, sec[0], rows[name]["seconds_median"], sec[-1])
                        if name != "none":
                            f, k = sorted(fetches[name]), kernels[name]
                            rows[name].update(us_per_capture=(rows[name]["seconds_median"] - base) / captures * 1e6, fetch_seconds_min=f[0],
                                              fetch_seconds_median=float(np.median(f)), fetch_seconds_max=f[-1])
                            line += "; %8.2f us per capture over no plan; fetch %7.4f / %7.4f / %7.4f s for %d bytes" \
                                % (rows[name]["us_per_capture"], f[0], rows[name]["fetch_seconds_median"], f[-1], k["fetch_bytes"])
                            line += "; %d folds, mean %.4f ms = %.2f us per capture, for %.0f model bytes = %.2f TB/s" \
                                % (k["folds"], k["mean_fold_ms"], k["fold_us_per_capture"], k["model_bytes_mean_fold"], k["model_tb_per_s"])
                        print(line, flush=True)
                        report[precision]["rows"][key] = rows[name]
                    ratio = dict(per_fold_measured=kernels["modulation"]["mean_fold_ms"] / kernels["decay bands"]["mean_fold_ms"],
                                 per_fold_model=kernels["modulation"]["model_bytes_mean_fold"] / kernels["decay bands"]["model_bytes_mean_fold"])
                    print("  %d bands every %d  modulation / decay bands per fold: %.3f measured, %.3f by the model of this run"
                          % (n_bands, period, ratio["per_fold_measured"], ratio["per_fold_model"]), flush=True)
                    report[precision]["modulation_over_decay_bands"]["%d bands every %d" % (n_bands, period)] = ratio
                    # the modulation plan's outputs against the definition over a snapshot plan's captures, on a strip of the plane
                    eng.rollback()
                    eng.set_snapshots(**plan)
                    assert eng.run_steps(steps) == (steps, 0)
                    snaps, snap_steps = eng.fetch_snapshots()
                    eng.set_snapshots(None)
                    n_rows = max(1, min(dims[1], args.check_nodes // dims[0]))
                    y0 = (dims[1] - n_rows) // 2
                    want_e, want_s = MOD.modulation_fold(snaps[:, :, y0:y0 + n_rows], snap_steps, freqs, bands)
                    got_e, got_s = np.ascontiguousarray(out[0][:, :, y0:y0 + n_rows]), np.ascontiguousarray(out[1][:, :, :, y0:y0 + n_rows])
                    same = got_e.tobytes() == want_e.tobytes() and got_s.tobytes() == want_s.tobytes() and bool((want_e.reshape(n_bands, -1).max(axis=1) > 0).all())
                    print("  %d bands every %d  against modulation.modulation_fold over the snapshots of %d rows (%d nodes): %s"
                          % (n_bands, period, n_rows, n_rows * dims[0], "bytewise equal" if same else "DIFFER"), flush=True)
                    report[precision]["bytewise_equal"]["%d bands every %d" % (n_bands, period)] = bool(same)
                    ok = ok and same
        finally:
            eng.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    print("MODULATION RATE %s" % ("OK" if ok else "OUTPUTS DIFFER"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Waterfall of one horizontal plane of a room, on one GPU: the field of a single-band waveguide run Fourier-transformed at a few
frequencies per time bin ON THE DEVICE (wv_set_waterfall), then the cumulative spectral decay and the decay time of whatever rings at
each frequency, per node of the plane -- how long each mode of the room rings, and where.

    python tools/waterfall_map.py --freqs 31.5,40,50,63 --plane z=1.2 --out waterfall.npz           # the built-in hall
    python tools/waterfall_map.py --obj room.obj --source 1 1 1 --receiver 2 3 1.2 --cutoff 150 --freqs 40,80 --bin-ms 20
    python tools/waterfall_map.py --room 48 --freqs 40,80,120 --seconds 0.2                        # a box of 48^3 nodes

The room (--obj with --material, or the built-in hall), --source, --receiver (the mesh is anchored there), --cutoff, --usable-portion,
--seconds and --precision are tools/impulse_response.py's; --room N takes a box of N^3 nodes at the cutoff's spacing instead of a scene.
The npz holds bins complex128[n_bins, K, ny, nx], csd_db (the cumulative spectral decay in dB below its first edge), decay_s (seconds
per 60 dB, NaN where fewer than three edges lie between -5 and -25 dB), times_s (the bin edges), freqs_hz, bin_captures, captures,
period, sample_rate, plane, origin, spacing."""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--obj")
    ap.add_argument("--room", type=int, default=None, metavar="N", help="a box of N^3 nodes in place of a scene")
    ap.add_argument("--material", action="append", default=[], help="name=a  or  name=a1,...,a8 (band absorptions)")
    ap.add_argument("--source", type=float, nargs=3, default=None)
    ap.add_argument("--receiver", type=float, nargs=3, default=None)
    ap.add_argument("--cutoff", type=float, default=200.0)
    ap.add_argument("--usable-portion", type=float, default=0.6)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--precision", default="f64", choices=["f32", "f64"])
    ap.add_argument("--freqs", required=True, metavar="HZ,...", help="1 .. 64 frequencies in Hz")
    ap.add_argument("--plane", default=None, metavar="z=METRES", help="the height of the plane (default: the receiver's)")
    ap.add_argument("--every", type=int, default=3, help="capture every k-th step (3 keeps every pass a three-step pass; the frequencies "
                                                         "must lie below sample rate / (2 k))")
    ap.add_argument("--bin-ms", type=float, default=10.0, help="the length of a time bin in milliseconds")
    ap.add_argument("--out", default="waterfall.npz")
    args = ap.parse_args()

    try:
        freqs_hz = [float(x) for x in args.freqs.split(",")]
    except ValueError:
        freqs_hz = []
    if not 1 <= len(freqs_hz) <= 64 or any(not (f >= 0.0 and math.isfinite(f)) for f in freqs_hz):
        ap.error("--freqs takes 1 .. 64 frequencies in Hz, e.g. 31.5,40,50")
    z = None
    if args.plane is not None:
        if not args.plane.startswith("z="):
            ap.error("--plane takes z=<metres>")
        try:
            z = float(args.plane[2:])
        except ValueError:
            ap.error("--plane takes z=<metres>")
    if args.every < 1 or not (args.bin_ms > 0 and math.isfinite(args.bin_ms)):
        ap.error("--every must be >= 1 and --bin-ms positive")
    if args.room is not None and (args.obj or args.room < 8):
        ap.error("--room takes 8 or more nodes per axis, and no --obj beside it")

    from wayverb_amd import mesh as M
    from wayverb_amd import scene as S
    from wayverb_amd import simulation as W
    from wayverb_amd import waterfall as WF
    env = W.Environment()
    rate = W.compute_sampling_frequency(args.cutoff, args.usable_portion)
    t0 = time.perf_counter()
    if args.room is not None:
        n = args.room
        spacing = float(np.float32(W.grid_spacing(env.speed_of_sound, 1.0 / rate)))
        mesh = M.box_mesh(n, n, n, coefficients=np.array([M.flat_coefficients(0.05)], dtype=M.coefficients_dtype), spacing=spacing)
        vm = W.VoxelsAndMesh(None, None, 0, None, None, mesh, (0.0, 0.0, 0.0))
        source = args.source or [spacing * (n // 3)] * 3
        receiver = args.receiver or [spacing * (n // 2), spacing * (n // 2), spacing * (n // 2)]
    else:
        if args.obj:
            v, t, names = S.read_obj(args.obj)
        else:
            (v, t), names = S.hall_scene(), ["plaster", "wood"]
        table = {"plaster": [0.05] * 8, "wood": [0.30, 0.30, 0.45, 0.65, 0.56, 0.59, 0.71, 0.71]}
        for m in args.material:
            name, val = m.split("=")
            vals = [float(x) for x in val.split(",")]
            table[name] = vals * 8 if len(vals) == 1 else vals
        source, receiver = args.source or [9.0, 3.0, 1.5], args.receiver or [8.0, 20.0, 1.2]
        vm = W.compute_voxels_and_mesh(v, t, [table.get(name, [0.05] * 8) for name in names], receiver, rate, env.speed_of_sound)
    mesh = vm.mesh
    sample_rate = W.compute_sample_rate(mesh.spacing, env.speed_of_sound)
    # as many bins as the run fills (the last is open-ended), 4096 sums per node at the most
    captures = int(math.ceil(sample_rate * args.seconds)) // args.every + 1
    bin_captures = max(1, int(round(args.bin_ms * 1e-3 * sample_rate / args.every)))
    n_bins = max(1, min(-(-captures // bin_captures), 4096 // len(freqs_hz)))
    asked = dict(freqs_hz=freqs_hz, plane=receiver[2] if z is None else z, every=args.every, n_bins=n_bins, bin_captures=bin_captures)
    try:
        plan = W.waterfall_plan_arguments(asked, mesh, sample_rate)
    except ValueError as e:
        ap.error(str(e))
    got = W.canonical(vm, source, receiver, env, args.cutoff, args.usable_portion, args.seconds, precision=args.precision, waterfall=asked)
    if got is None:
        sys.exit("the waveguide run was stopped early")
    _, (bins, taken) = got
    bins = bins[:, :, 0]      # [n_bins, K, 1, ny, nx], what a plan of one plane fetches -> [n_bins, K, ny, nx]
    maps = WF.waterfall_maps(bins, bin_captures, args.every, sample_rate)
    np.savez(args.out, bins=bins, csd_db=maps["csd_db"], decay_s=maps["decay_s"], times_s=maps["times_s"], freqs_hz=np.array(freqs_hz),
             bin_captures=bin_captures, captures=taken, period=args.every, sample_rate=sample_rate, plane=plan["box"][0][2], spacing=mesh.spacing,
             origin=np.asarray(mesh.min_corner, dtype=np.float64) + mesh.spacing * np.array(plan["box"][0], dtype=np.float64))
    print("mesh %dx%dx%d (spacing %.4f m), %d steps at %.1f Hz, %.2f s wall" % (mesh.dims + (mesh.spacing, int(math.ceil(sample_rate * args.seconds)),
                                                                                   sample_rate, time.perf_counter() - t0)))
    for k, f in enumerate(freqs_hz):
        t = maps["decay_s"][k][np.isfinite(maps["decay_s"][k])]
        print("  %8.2f Hz: decay time %s (%d of %d nodes)" % (f, "median %.3f s" % np.median(t) if t.size else "not defined", t.size, maps["decay_s"][k].size))
    print("wrote the waterfall of plane z=%d (%d bins of %d captures, %d captures, %d frequencies) to %s"
          % (plan["box"][0][2], bins.shape[0], bin_captures, taken, len(freqs_hz), args.out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""IACC maps of one horizontal plane of a room, on one GPU: for every seat of the plane the field of a single-band waveguide run at two
nodes an ear-distance apart, correlated at lags of up to +-1 ms per time bin ON THE DEVICE (wv_set_interaural), then ISO 3382-1 Annex
B's IACC_E (0 .. 80 ms behind each seat's own arrival), IACC_L (from 80 ms on), IACC_A (all of it) and the lag of each maximum.  The
waveguide carries the band below the crossover, where two points in space an ear-distance apart are the head-less ("spaced omni") form
of the measurement: this is not a dummy head.

    python tools/interaural_map.py --plane z=1.2 --out interaural.npz                                # the built-in hall
    python tools/interaural_map.py --obj room.obj --source 1 1 1 --receiver 2 3 1.2 --cutoff 150 --ear-axis 1 0 0
    python tools/interaural_map.py --room 48 --seconds 0.2 --band 60,180                            # a box of 48^3 nodes

The room (--obj with --material, or the built-in hall), --source, --receiver (the mesh is anchored there), --cutoff, --usable-portion,
--seconds and --precision are tools/impulse_response.py's; --room N takes a box of N^3 nodes at the cutoff's spacing instead of a scene.
The seats are the plane less a rim as wide as the ears reach, so that every ear lies on the mesh.  The npz holds iacc_e, iacc_l, iacc_a,
lag_e_ms, lag_l_ms, lag_a_ms [ny, nx] (NaN where a seat heard nothing in the window), onset [ny, nx], bins float64[n_bins, 2 L + 3, ny,
nx], edges, max_lag, ear_a, ear_b, ear_distance_m, captures, period, sample_rate, plane, origin, spacing."""
import argparse
import math
import os
import sys
import time
import warnings

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
    ap.add_argument("--plane", default=None, metavar="z=METRES", help="the height of the plane (default: the receiver's)")
    ap.add_argument("--every", type=int, default=1, help="capture every k-th step (the lags are counted in captures: 16 of them at the most)")
    ap.add_argument("--ear-axis", type=float, nargs=3, default=[0.0, 1.0, 0.0], help="the direction from one ear to the other")
    ap.add_argument("--ear-distance", type=float, default=0.17, help="metres between the ears, rounded to mesh nodes")
    ap.add_argument("--max-lag-ms", type=float, default=1.0)
    ap.add_argument("--early-ms", type=float, default=80.0, help="where IACC_E ends and IACC_L begins, behind each seat's arrival")
    ap.add_argument("--threshold", type=float, default=1e-6, help="the pressure magnitude at either ear that counts as the arrival")
    ap.add_argument("--band", default=None, metavar="LO,HI", help="a band-pass in Hz ahead of the correlation (4th-order Butterworth)")
    ap.add_argument("--out", default="interaural.npz")
    args = ap.parse_args()

    z = None
    if args.plane is not None:
        if not args.plane.startswith("z="):
            ap.error("--plane takes z=<metres>")
        try:
            z = float(args.plane[2:])
        except ValueError:
            ap.error("--plane takes z=<metres>")
    if args.every < 1 or not (args.early_ms > 0 and math.isfinite(args.early_ms)) or not (args.threshold >= 0 and math.isfinite(args.threshold)):
        ap.error("--every must be >= 1, --early-ms positive and --threshold >= 0")
    band = None
    if args.band is not None:
        try:
            band = tuple(float(x) for x in args.band.split(","))
        except ValueError:
            band = ()
        if len(band) != 2 or not 0 < band[0] < band[1]:
            ap.error("--band takes LO,HI in Hz with 0 < LO < HI")
    if args.room is not None and (args.obj or args.room < 8):
        ap.error("--room takes 8 or more nodes per axis, and no --obj beside it")

    from wayverb_amd import interaural as IA
    from wayverb_amd import mesh as M
    from wayverb_amd import scene as S
    from wayverb_amd import simulation as W
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
    asked = dict(threshold=args.threshold, plane=receiver[2] if z is None else z, every=args.every, edges_ms=(0.0, args.early_ms), ear_axis=tuple(args.ear_axis),
                 ear_distance=args.ear_distance, max_lag_ms=args.max_lag_ms, band_hz=band)
    try:
        with warnings.catch_warnings(record=True) as said:
            warnings.simplefilter("always")
            plan = W.interaural_plan_arguments(asked, mesh, sample_rate)
    except ValueError as e:
        ap.error(str(e))
    for w in said:
        print("warning:", w.message, file=sys.stderr)
    # the seats: the plane less the rim the ears reach into (their z must stay on the mesh as it is)
    plane = plan["box"][0][2]
    lo = [max(0, -plan["ear_a"][k], -plan["ear_b"][k]) for k in range(3)]
    hi = [max(0, plan["ear_a"][k], plan["ear_b"][k]) for k in range(3)]
    if plane - lo[2] < 0 or plane + hi[2] > mesh.dims[2] - 1:
        ap.error("the ears of plane z=%d leave the mesh" % plane)
    asked = dict(asked, box=((lo[0], lo[1], plane), (mesh.dims[0] - lo[0] - hi[0], mesh.dims[1] - lo[1] - hi[1], 1)))
    del asked["plane"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (said above)
        got = W.canonical(vm, source, receiver, env, args.cutoff, args.usable_portion, args.seconds, precision=args.precision, interaural=asked)
    if got is None:
        sys.exit("the waveguide run was stopped early")
    _, (out, taken) = got
    bins, onset = out["bins"][:, :, 0], out["onset"][0]      # [n_bins, 2 L + 3, 1, ny, nx], what a plan of one plane fetches -> [n_bins, 2 L + 3, ny, nx]
    windows = dict(e=0, l=1, a=None) if bins.shape[0] == 2 else dict(a=None)
    maps = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (an all-NaN seat)
        for name, window in windows.items():
            maps["iacc_" + name] = IA.iacc(bins, window)
            maps["lag_%s_ms" % name] = IA.iacc_lag(bins, window, True, args.every, sample_rate)
    distance = mesh.spacing * math.sqrt(sum((b - a) ** 2 for a, b in zip(plan["ear_a"], plan["ear_b"])))
    np.savez(args.out, bins=bins, onset=onset, edges=np.array(plan["edges"]), max_lag=plan["max_lag"], ear_a=np.array(plan["ear_a"]), ear_b=np.array(plan["ear_b"]),
             ear_distance_m=distance, captures=taken, period=args.every, sample_rate=sample_rate, plane=plane, spacing=mesh.spacing,
             origin=np.asarray(mesh.min_corner, dtype=np.float64) + mesh.spacing * np.array(asked["box"][0], dtype=np.float64), **maps)
    print("mesh %dx%dx%d (spacing %.4f m), %d steps at %.1f Hz, %.2f s wall" % (mesh.dims + (mesh.spacing, int(math.ceil(sample_rate * args.seconds)),
                                                                                   sample_rate, time.perf_counter() - t0)))
    for name in windows:
        v = maps["iacc_" + name][np.isfinite(maps["iacc_" + name])]
        print("  IACC_%s: %s (%d of %d seats)" % (name.upper(), "median %.3f" % np.median(v) if v.size else "not defined", v.size, maps["iacc_" + name].size))
    print("wrote the interaural maps of plane z=%d (ears %r and %r, %.3f m apart, lags of +-%d captures, %d captures) to %s"
          % (plane, tuple(plan["ear_a"]), tuple(plan["ear_b"]), distance, plan["max_lag"], taken, args.out))


if __name__ == "__main__":
    main()

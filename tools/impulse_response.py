#!/usr/bin/env python3
"""Scene -> waveguide impulse response, end to end on one GPU (the waveguide leg of
BASELINE configs[4]): OBJ (v / f / usemtl) or the built-in hall, per-material 8-band absorptions,
single-band waveguide at `--cutoff`, microphone or omni capsule, WAV out.

    python tools/impulse_response.py --out ir.wav                       # built-in hall
    python tools/impulse_response.py --way demo/evaluation/receivers/concert.way   # a wayverb project bundle
    python tools/impulse_response.py --receiver 8 20 1.2 --receiver 4 12 1.2 --receiver 14 25 1.2 --out ir.wav
                                                                        # three listeners, ONE run of the mesh: ir_0.wav ir_1.wav ir_2.wav
    python tools/impulse_response.py --obj concert.obj --source 0 0 0 --receiver 0 1.47 -20.06 \
        --material DefaultMaterial=0.05 --material FrontColor=0.30,0.30,0.45,0.65,0.56,0.59,0.71,0.71
"""
import argparse
import os
import sys
import time
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import postprocess as P  # noqa: E402
from wayverb_amd import scene as S  # noqa: E402
from wayverb_amd import simulation as W  # noqa: E402


def write_wav(path, audio, rate):
    peak = float(np.abs(audio).max()) or 1.0
    pcm = np.clip(audio / peak * 32767.0, -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(pcm.tobytes())
    return peak


# the flags that set a capture plan, in the order main() looks at them: each excludes the ones ahead of it
PLAN_FLAGS = ("--snapshots", "--spectrum", "--decay-map", "--intensity-map", "--clarity-map", "--lateral-map", "--modulation-map")


def listed(flags):
    """--a, --b or --c"""
    return " or ".join(filter(None, [", ".join(flags[:-1]), flags[-1]]))


def one_plane(maps):
    """[..., 1, ny, nx], what a plan of one horizontal plane fetches -> [..., ny, nx]"""
    return maps[..., 0, :, :]


def npz_keys(plan, mesh, rate, captures):
    """What every plan's npz says of the run: the captures taken, the cadence, the plane and where its first node lies."""
    return dict(captures=captures, period=plan["period"], sample_rate=rate, plane=plan["box"][0][2], spacing=mesh.spacing,
                origin=np.asarray(mesh.min_corner, dtype=np.float64) + mesh.spacing * np.array(plan["box"][0], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj")
    ap.add_argument("--way", help="a .way project directory (config.json + model.model): scene, materials, first "
                                    "source / receiver / capsule and the waveguide parameters come from it")
    ap.add_argument("--material", action="append", default=[], help="name=a  or  name=a1,...,a8 (band absorptions)")
    ap.add_argument("--source", type=float, nargs=3, default=[9.0, 3.0, 1.5])
    ap.add_argument("--receiver", type=float, nargs=3, action="append", default=None,
                    help="may be given several times: every receiver listens to the same run of the mesh (the mesh is anchored at "
                         "the first, the others snap to their nearest node), and --out gets _<i> suffixes (default: 8 20 1.2)")
    ap.add_argument("--cutoff", type=float, default=200.0)
    ap.add_argument("--usable-portion", type=float, default=0.6)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rate", type=float, default=44100.0)
    ap.add_argument("--mic-shape", type=float, default=None, help="0 omni .. 1 figure-eight; omit for raw pressure")
    ap.add_argument("--pointing", type=float, nargs=3, default=[0.0, 0.0, 1.0])
    ap.add_argument("--precision", default="f64", choices=["f32", "f64"])
    ap.add_argument("--out", default="ir.wav")
    ap.add_argument("--snapshots", help="z=<plane>,every=<k>: record plane z of the field every k steps while the run goes on "
                                        "(Engine.set_snapshots; single-band runs)")
    ap.add_argument("--snapshot-out", default="snapshots", help="directory the snapshots go to, one step_<n>.npy (float32[ny, nx]) each")
    ap.add_argument("--spectrum", help="HZ[,HZ...]: Fourier-transform one horizontal plane of the field at these frequencies on the "
                                       "device while the run goes on (Engine.set_spectrum; single-band runs)")
    ap.add_argument("--spectrum-plane", default=None, help="z=<metres>: the height of that plane (default: the receiver's)")
    ap.add_argument("--spectrum-out", default="spectrum.npz", help="the complex maps go here: spectrum complex128[K, ny, nx], freqs_hz, "
                                                                   "captures, plane (node index), z (metres of that plane)")
    ap.add_argument("--decay-map", nargs="?", const="", default=None, metavar="z=METRES",
                    help="sum the squared field of one horizontal plane into time bins on the device while the run goes on "
                         "(Engine.set_decay; single-band runs) and write EDT / T20 / T30 and level maps of it; z=<metres>: the height "
                         "of that plane (default: the receiver's)")
    ap.add_argument("--decay-bin-ms", type=float, default=10.0, help="the length of a time bin in milliseconds")
    ap.add_argument("--decay-every", type=int, default=3, help="capture every k-th step (3 keeps every pass a three-step pass; the "
                                                               "levels then lie 10 log10(k) dB low, the decay times do not change)")
    ap.add_argument("--decay-bands", default=None, metavar="HZ,HZ,...",
                    help="with --decay-map: octave-band centres in Hz (8 at the most), e.g. 125,250,500 -- every node's captures go "
                         "through a 4th-order Butterworth band-pass per band on the device before they are squared, and the maps are "
                         "written per band (a leading band axis).  The filters run at sample rate / --decay-every: an impulse needs "
                         "--decay-every 1")
    ap.add_argument("--decay-out", default="decay.npz", help="the maps go here: bins float64[n_bins, ny, nx], edt_s / t20_s / t30_s and "
                                                             "their _r, level_db, edc_db, sample_rate, bin_captures, period, captures, "
                                                             "plane, origin (metres of the plane's first node), spacing")
    ap.add_argument("--intensity-map", action="store_true",
                    help="sum the sound intensity vector and the squared pressure of one horizontal plane (less its rim) into time "
                         "bins on the device while the run goes on (Engine.set_intensity; single-band runs, no other plan)")
    ap.add_argument("--intensity-plane", default=None, metavar="z=METRES", help="the height of that plane (default: the receiver's)")
    ap.add_argument("--intensity-every", type=int, default=1, help="capture every N-th step (the integrator then runs at sample rate / N: "
                                                                   "an impulse needs 1; 3 keeps every pass a three-step pass)")
    ap.add_argument("--intensity-bin-ms", type=float, default=10.0, help="the length of a time bin in milliseconds")
    ap.add_argument("--intensity-out", default="intensity.npz",
                    help="the maps go here: bins float64[4, n_bins, ny, nx] (Ix, Iy, Iz, E), times (seconds at which each bin begins), "
                         "net_direction [3, ny, nx], net_magnitude, diffuseness [ny, nx], captures, period, sample_rate, spacing")
    ap.add_argument("--clarity-map", action="store_true",
                    help="keep, per node of one horizontal plane and on the device, when the direct sound arrives, the peak, and the "
                         "squared pressure in bins of 0-50, 50-80 and 80+ ms counted from the node's OWN arrival (Engine.set_arrival; "
                         "single-band runs, no other plan): arrival time, direct level, C50, C80, D50 and centre time maps")
    ap.add_argument("--arrival-plane", default=None, metavar="z=METRES", help="the height of that plane (default: the receiver's)")
    ap.add_argument("--arrival-threshold", type=float, default=1e-4,
                    help="the pressure magnitude that counts as the arrival of the direct sound (default 1e-4; the source's impulse is 1)")
    ap.add_argument("--arrival-every", type=int, default=1, help="capture every N-th step (arrival times are then known to N steps)")
    ap.add_argument("--clarity-bands", default=None, metavar="HZ,HZ,...",
                    help="with --clarity-map: octave-band centres (8 at the most); the maps are then per band -- every capture goes through "
                         "a 4th-order Butterworth band-pass ahead of the square (Engine.set_arrival_bands), every band's clock starting "
                         "late by its filter's group delay -- and --arrival-out holds pre, moment [K, ny, nx], bins [K, n_bins, ny, nx], "
                         "bands_hz, lag, tail and c50_db, c80_db, d50, ts_s, edt_s, t20_s, t30_s [K, ny, nx]")
    ap.add_argument("--clarity-tail-ms", type=float, default=None,
                    help="with --clarity-bands: uniform bins behind the 80 ms edge out to this many milliseconds behind each node's arrival, "
                         "from which the per-band EDT, T20 and T30 are read (default: none, and those maps are NaN)")
    ap.add_argument("--clarity-tail-bin-ms", type=float, default=10.0, help="the length of a tail bin (default 10 ms)")
    ap.add_argument("--arrival-out", default="arrival.npz",
                    help="the maps go here: onset, peak, peak_capture, pre, moment [ny, nx], bins [3, ny, nx], edges, arrival_s, direct_db, "
                         "c50_db, c80_db, d50, d80, ts_s, pre_fraction, captures, period, sample_rate, plane, origin, spacing")
    ap.add_argument("--lateral-map", action="store_true",
                    help="keep, per node of one horizontal plane (less its rim) and on the device, the squared pressure, the sound "
                         "intensity and the second moments of the particle velocity in bins of 0-5, 5-80 and 80+ ms counted from the "
                         "node's OWN arrival (Engine.set_lateral; single-band runs, no other plan): the early lateral energy fraction "
                         "LF along each node's own lateral axis, the direction the direct sound came from and the diffuseness")
    ap.add_argument("--lateral-plane", default=None, metavar="z=METRES", help="the height of that plane (default: the receiver's)")
    ap.add_argument("--lateral-threshold", type=float, default=1e-4,
                    help="the pressure magnitude that counts as the arrival of the direct sound (default 1e-4; the source's impulse is 1)")
    ap.add_argument("--lateral-every", type=int, default=1, help="capture every N-th step (the integrator then runs at sample rate / N)")
    ap.add_argument("--lateral-out", default="lateral.npz",
                    help="the maps go here: lf, diffuseness [ny, nx], direct_direction, lateral_axis [3, ny, nx], onset, pre [ny, nx], "
                         "velocity [3, ny, nx], bins [10, 3, ny, nx], edges, captures, period, sample_rate, plane, origin, spacing")
    ap.add_argument("--modulation-map", nargs="?", const="", default=None, metavar="z=METRES",
                    help="keep, per node of one horizontal plane (default: the receiver's height) and on the device, the energy of "
                         "octave bands and the Fourier sums of their squared signal at the 14 modulation frequencies of IEC 60268-16 "
                         "(Engine.set_modulation; single-band runs, no other plan): the modulation transfer function and the "
                         "modulation transfer index per band, and with --sti-rest the speech transmission index")
    ap.add_argument("--modulation-bands", default="125,250,500", metavar="HZ,HZ,...",
                    help="octave centres the mesh carries (default 125,250,500; up to 8); their upper edges belong below a quarter of the sample rate")
    ap.add_argument("--modulation-every", type=int, default=1, help="capture every N-th step (the band filters then run at sample rate / N)")
    ap.add_argument("--sti-rest", default=None, metavar="HZ:MTI,...",
                    help="the modulation transfer index of the octave bands the mesh does not carry, from a geometric method or a "
                         "measurement, e.g. 1000:0.55,2000:0.5,4000:0.5,8000:0.45; with all seven bands known the file holds sti")
    ap.add_argument("--modulation-out", default="modulation.npz",
                    help="the maps go here: mtf [K, 14, ny, nx], mti [K, ny, nx], sti [ny, nx] (with --sti-rest), energy, bands_hz, "
                         "freqs_hz, captures, period, sample_rate, plane, origin, spacing")
    args = ap.parse_args()

    bands = None
    if args.way:
        from wayverb_amd import wayfile
        cfg, v, t, way_absorptions = wayfile.read_way(args.way)
        names = None
        args.source = cfg["sources"][0]["position"]
        args.receiver = [cfg["receivers"][0]["position"]]
        wg = cfg["waveguide"]
        params = wg["single"] if wg["mode"] == "single" else wg["multiple"]
        args.cutoff, args.usable_portion = params["cutoff"], params["usable_portion"]
        bands = wg["multiple"]["bands"] if wg["mode"] == "multiple" else None
        capsule = cfg["receivers"][0]["capsules"][0]
        if capsule["mode"] == "microphone":
            args.mic_shape = capsule["microphone"]["shape"]
            args.pointing = capsule["microphone"]["pointing"]
        else:
            print("capsule %r is an HRTF capsule: not supported by this engine, recording omni pressure" % capsule["name"])
    elif args.obj:
        v, t, names = S.read_obj(args.obj)
    else:
        v, t = S.hall_scene()
        names = ["plaster", "wood"]
    table = {"plaster": [0.05] * 8, "wood": [0.30, 0.30, 0.45, 0.65, 0.56, 0.59, 0.71, 0.71]}
    for m in args.material:
        name, val = m.split("=")
        vals = [float(x) for x in val.split(",")]
        table[name] = vals * 8 if len(vals) == 1 else vals
    absorptions = way_absorptions if args.way else [table.get(n, [0.05] * 8) for n in names]

    receivers = args.receiver or [[8.0, 20.0, 1.2]]
    args.receiver = receivers[0]
    plans = {}   # impulse_response's keyword -> the plan; the flags exclude each other, so it never holds two

    def alone(flag):
        """The refusal of `flag` beside multi-band runs and the plan flags ahead of it, one of which `plans` then holds already."""
        if bands or plans:
            ap.error("%s: single-band runs without %s" % (flag, listed(PLAN_FLAGS[:PLAN_FLAGS.index(flag)])))

    def z_of(value, option):
        """z=<metres> -> the number's text, which metres() converts once the flag's other checks have passed; not given: None."""
        if value and not value.startswith("z="):
            ap.error("%s takes z=<metres>" % option)
        return value[2:] if value else None

    def metres(z):
        """The height z_of() found; not given: the receiver's."""
        return float(z) if z else args.receiver[2]

    if args.snapshots:
        if bands:
            ap.error("--snapshots: single-band runs only")
        want = dict(item.split("=") for item in args.snapshots.split(","))
        if sorted(want) != ["every", "z"]:
            ap.error("--snapshots takes z=<plane>,every=<k>")
        plane, every = int(want["z"]), int(want["every"])
        plans["snapshots"] = lambda mesh: dict(box=((0, 0, plane), (None, None, 1)), period=every)
    if args.spectrum:
        alone("--spectrum")
        freqs_hz = [float(x) for x in args.spectrum.split(",")]
        height = metres(z_of(args.spectrum_plane, "--spectrum-plane"))
        spectrum_plane = {}

        def spectrum(mesh):
            plane = int(round((height - mesh.min_corner[2]) / mesh.spacing))
            if not 0 <= plane < mesh.dims[2]:
                ap.error("--spectrum-plane: z=%g m is outside the mesh" % height)
            spectrum_plane.update(plane=plane, z=mesh.min_corner[2] + plane * mesh.spacing)
            return dict(freqs_hz=freqs_hz, box=((0, 0, plane), (None, None, 1)))
        plans["spectrum"] = spectrum
    if args.decay_map is not None:
        alone("--decay-map")
        z = z_of(args.decay_map, "--decay-map")
        if args.decay_every < 1 or not args.decay_bin_ms > 0:
            ap.error("--decay-every must be >= 1 and --decay-bin-ms positive")
        decay_height = metres(z)
        decay_plan = {}
        try:
            decay_centres = [float(c) for c in args.decay_bands.split(",")] if args.decay_bands else []
        except ValueError:
            ap.error("--decay-bands takes octave centres in Hz, e.g. 125,250,500")
        if len(decay_centres) > 8 or any(not c > 0 for c in decay_centres):
            ap.error("--decay-bands: 1 .. 8 positive centre frequencies")

        def decay(mesh, rate):
            plane = int(round((decay_height - mesh.min_corner[2]) / mesh.spacing))
            if not 0 <= plane < mesh.dims[2]:
                ap.error("--decay-map: z=%g m is outside the mesh" % decay_height)
            captures = int(np.ceil(rate * args.seconds)) // args.decay_every + 1
            per_bin = max(1, int(round(args.decay_bin_ms * 1e-3 * rate / args.decay_every)))
            n_bins = max(1, min(4096, -(-captures // per_bin)))
            decay_plan.update(n_bins=n_bins, bin_captures=per_bin, box=((0, 0, plane), (None, None, 1)), period=args.decay_every)
            if decay_centres:
                from wayverb_amd import decay as D
                decay_plan["bands"] = D.octave_band_edges(decay_centres)
                for sentence in W.octave_band_warnings(decay_centres, decay_plan["bands"], rate, args.decay_every, "", "--decay-every %d"):
                    print("warning: " + sentence, file=sys.stderr)
            return decay_plan
        plans["decay"] = decay
    if args.intensity_map:
        alone("--intensity-map")
        z = z_of(args.intensity_plane, "--intensity-plane")
        if args.intensity_every < 1 or not args.intensity_bin_ms > 0:
            ap.error("--intensity-every must be >= 1 and --intensity-bin-ms positive")
        plans["intensity"] = dict(plane=metres(z), every=args.intensity_every, bin_seconds=args.intensity_bin_ms * 1e-3)
    if args.clarity_map:
        alone("--clarity-map")
        z = z_of(args.arrival_plane, "--arrival-plane")
        if args.arrival_every < 1 or not (args.arrival_threshold >= 0 and np.isfinite(args.arrival_threshold)):
            ap.error("--arrival-every must be >= 1 and --arrival-threshold >= 0 and finite")
        plans["arrival"] = dict(plane=metres(z), every=args.arrival_every, threshold=args.arrival_threshold, early_ms=(50.0, 80.0))
        if args.clarity_bands:
            from wayverb_amd import decay as D
            centres = [float(v) for v in args.clarity_bands.split(",")]
            if not 1 <= len(centres) <= 8 or any(not c > 0 for c in centres):
                ap.error("--clarity-bands takes 1 .. 8 positive octave centres")
            plans["arrival"].update(bands=D.octave_band_edges(centres), tail_ms=args.clarity_tail_ms, tail_bin_ms=args.clarity_tail_bin_ms,
                                    lag="group-delay")
    elif args.clarity_bands:
        ap.error("--clarity-bands goes with --clarity-map")
    if args.lateral_map:
        alone("--lateral-map")
        z = z_of(args.lateral_plane, "--lateral-plane")
        if args.lateral_every < 1 or not (args.lateral_threshold >= 0 and np.isfinite(args.lateral_threshold)):
            ap.error("--lateral-every must be >= 1 and --lateral-threshold >= 0 and finite")
        plans["lateral"] = dict(plane=metres(z), every=args.lateral_every, threshold=args.lateral_threshold, edges_ms=(0.0, 5.0, 80.0))
    if args.modulation_map is not None:
        alone("--modulation-map")
        z = z_of(args.modulation_map, "--modulation-map")
        try:
            modulation_centres = [float(c) for c in args.modulation_bands.split(",")]
            sti_rest = {float(item.split(":")[0]): float(item.split(":")[1]) for item in args.sti_rest.split(",")} if args.sti_rest else None
        except (ValueError, IndexError):
            ap.error("--modulation-bands takes octave centres in Hz, e.g. 125,250,500, and --sti-rest HZ:MTI pairs, e.g. 1000:0.55,2000:0.5")
        if not 1 <= len(modulation_centres) <= 8 or any(not c > 0 for c in modulation_centres) or args.modulation_every < 1:
            ap.error("--modulation-bands: 1 .. 8 positive centre frequencies; --modulation-every must be >= 1")
        plans["modulation"] = dict(plane=metres(z), every=args.modulation_every, bands_hz=modulation_centres)
    t0 = time.perf_counter()
    method = P.ATTENUATOR_NULL if args.mic_shape is None else P.ATTENUATOR_MICROPHONE
    if len(receivers) > 1:
        if bands or plans:
            ap.error("several --receiver: single-band runs without %s" % listed(PLAN_FLAGS))
        audios, per, positions, vm = W.impulse_responses(v, t, absorptions, args.source, receivers, args.cutoff, args.usable_portion,
                                                         args.seconds, args.rate, method=method, pointing=args.pointing,
                                                         shape=args.mic_shape or 0.0, precision=args.precision)
        dt = time.perf_counter() - t0
        mesh = vm.mesh
        print("mesh %dx%dx%d (%d nodes, spacing %.4f m), %d steps at %.1f Hz for %d receivers in one run, %.2f s wall"
              % (mesh.dims + (mesh.num_nodes, mesh.spacing, per[0][0][0].shape[0], per[0][0][1], len(receivers), dt)))
        stem, ext = os.path.splitext(args.out)
        for i, (audio, pos) in enumerate(zip(audios, positions)):
            name = "%s_%d%s" % (stem, i, ext)
            peak = write_wav(name, audio, args.rate)
            print("wrote %s: receiver at node position (%.3f, %.3f, %.3f) (normalised, peak was %.3e)" % ((name,) + tuple(pos) + (peak,)))
        return
    if bands and any(k in plans for k in ("intensity", "arrival", "lateral")):
        ap.error("--intensity-map, --clarity-map, --lateral-map: single-band runs only")
    if bands and "modulation" in plans:
        ap.error("--modulation-map: single-band runs only")
    if bands:   # multiple_band_constant_spacing: one run per band with flat per-band walls
        env = W.Environment()
        vm = W.compute_voxels_and_mesh(v, t, absorptions, args.receiver,
                                       W.compute_sampling_frequency(args.cutoff, args.usable_portion), env.speed_of_sound)
        bands = W.canonical_multiband(vm, args.source, args.receiver, env, bands, args.cutoff, args.usable_portion,
                                      args.seconds, args.precision)
        audio = P.postprocess(bands, method, args.pointing, args.mic_shape or 0.0, env.acoustic_impedance, args.rate)
    else:
        audio_etc = W.impulse_response(v, t, absorptions, args.source, args.receiver, args.cutoff,
                                       args.usable_portion, args.seconds, args.rate, method=method,
                                       pointing=args.pointing, shape=args.mic_shape or 0.0,
                                       precision=args.precision, **plans)
        kind = next(iter(plans), None)   # the one plan of this run, if any
        out, captures = audio_etc[3] if kind else (None, None)
        env, mesh = W.Environment(), audio_etc[2].mesh
        rate = W.compute_sample_rate(mesh.spacing, env.speed_of_sound)
        name, positional, plan, shared = kind, (), None, None
        if kind in ("intensity", "arrival", "lateral", "modulation"):   # the arguments canonical gave Engine.set_<name>, once more
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")   # (canonical has said it already)
                name, positional, plan = W.plan_call(kind, plans[kind], mesh, rate, env, args.seconds)
        elif kind == "decay":
            plan = decay_plan
        if plan is not None:
            shared = npz_keys(plan, mesh, rate, captures)
        if kind == "modulation":
            from wayverb_amd import modulation as MOD
            energy, sums = one_plane(out[0]), one_plane(out[1])   # [K, ny, nx], [K, M, ny, nx]
            transfer = MOD.mtf(energy, sums)
            index = MOD.mti(transfer)
            extra = {}
            carried = {int(round(c)): index[k] for k, c in enumerate(modulation_centres)}
            if sti_rest is not None and all(c in carried or c in {int(round(r)) for r in sti_rest} for c in MOD.STI_OCTAVE_HZ):
                extra["sti"] = MOD.sti(carried, rest=sti_rest)
            elif sti_rest is not None:
                print("warning: --sti-rest and --modulation-bands leave octave bands of 125 Hz .. 8 kHz out: no sti is written", file=sys.stderr)
            np.savez(args.modulation_out, mtf=transfer, mti=index, energy=energy, bands_hz=np.array(modulation_centres),
                     freqs_hz=np.array(MOD.STI_MODULATION_HZ), **shared, **extra)
            print("wrote modulation maps of plane z=%d (%d bands, %d captures; median MTI per band %s%s) to %s"
                  % (shared["plane"], len(modulation_centres), captures,
                     ", ".join("%.3f" % np.nanmedian(m) if np.isfinite(m).any() else "not defined" for m in index),
                     "; median STI %.3f" % np.nanmedian(extra["sti"]) if "sti" in extra and np.isfinite(extra["sti"]).any() else "", args.modulation_out))
        if kind == "lateral":
            from wayverb_amd import lateral as L
            out = {k: one_plane(v) for k, v in out.items()}   # onset, pre [ny, nx]; velocity [3, ny, nx]; bins [10, n_bins, ny, nx]
            came_from = L.direct_direction(out)
            axis = L.lateral_axis(came_from)
            # J_LF: the figure-of-eight's energy in 5 - 80 ms over the omni's in 0 - 80 ms, where both edges are bins of the plan
            lf = L.lateral_fraction(out, axis, 1, (0, 1), env.ambient_density, env.speed_of_sound) if len(plan["edges"]) == 3 else \
                np.full(out["onset"].shape, np.nan)
            diffuse = L.diffuseness(out, env.ambient_density, env.speed_of_sound)
            np.savez(args.lateral_out, edges=np.array(plan["edges"]), lf=lf, direct_direction=came_from, lateral_axis=axis, diffuseness=diffuse,
                     **shared, **out)
            heard = out["onset"] != L.NONE
            print("wrote lateral maps of plane z=%d (%d captures; %d of %d nodes heard an arrival; median LF %s) to %s"
                  % (shared["plane"], captures, heard.sum(), heard.size, "%.3f" % np.nanmedian(lf) if np.isfinite(lf).any() else "not defined",
                     args.lateral_out))
        if kind == "arrival":
            from wayverb_amd import arrival as A
            # the one plane: onset, peak, peak_capture [ny, nx]; per band pre, moment [K, ny, nx]; bins [n_bins, ny, nx] or [K, n_bins, ny, nx]
            out = {k: one_plane(v) for k, v in out.items()}
            heard = out["onset"] != A.NONE
            period = plan["period"]
        if name == "arrival_bands":
            edges, tail = positional[0], plan["tail"]
            maps = dict(arrival_s=A.arrival_time(out["onset"], plan["first_step"], period, rate), direct_db=A.direct_level_db(out["peak"]),
                        c50_db=A.band_clarity(out["bins"], edges, 50.0, period, rate), c80_db=A.band_clarity(out["bins"], edges, 80.0, period, rate),
                        d50=A.band_definition(out["bins"], edges, 50.0, period, rate), ts_s=A.band_centre_time(out["moment"], out["bins"], period, rate))
            decays = A.band_decay_maps(out["bins"], edges, tail, period, rate)
            maps.update({k: decays[k] for k in ("edt_s", "t20_s", "t30_s")})
            np.savez(args.arrival_out, edges=np.array(edges), tail=np.array(tail or (0, 0, 0)), lag=np.array(plan["lag"]),
                     bands_hz=np.array([float(v) for v in args.clarity_bands.split(",")]), **shared, **out, **maps)
            print("wrote arrival maps of plane z=%d in %d bands (%d captures; %d of %d nodes heard an arrival; median C80 per band %s) to %s"
                  % (shared["plane"], out["bins"].shape[0], captures, heard.sum(), heard.size,
                     ", ".join("%.1f dB" % np.median(c[np.isfinite(c)]) if np.isfinite(c).any() else "not defined" for c in maps["c80_db"]),
                     args.arrival_out))
        elif name == "arrival":
            maps = A.arrival_maps(out, plan["edges"], plan["first_step"], period, rate)
            np.savez(args.arrival_out, edges=np.array(plan["edges"]), **shared, **out, **maps)
            c80 = maps["c80_db"][np.isfinite(maps["c80_db"])]
            print("wrote arrival maps of plane z=%d (%d captures; %d of %d nodes heard an arrival; median C80 %s) to %s"
                  % (shared["plane"], captures, heard.sum(), heard.size, "%.1f dB" % np.median(c80) if c80.size else "not defined",
                     args.arrival_out))
        if kind == "intensity":
            from wayverb_amd import intensity as I
            bins = one_plane(out)   # [4, n_bins, ny, nx]
            _, magnitude, direction = I.net_intensity(bins)
            diffuse = I.diffuseness(bins, env.speed_of_sound, env.ambient_density)
            np.savez(args.intensity_out, bins=bins, times=np.arange(bins.shape[1]) * plan["bin_captures"] * plan["period"] / rate,
                     net_direction=direction, net_magnitude=magnitude, diffuseness=diffuse, bin_captures=plan["bin_captures"], **shared)
            print("wrote intensity maps of plane z=%d (%d bins of %d captures, %d captures; median diffuseness %s) to %s"
                  % (shared["plane"], bins.shape[1], plan["bin_captures"], captures,
                     "%.3f" % np.nanmedian(diffuse) if np.isfinite(diffuse).any() else "not defined", args.intensity_out))
        if kind == "decay":
            from wayverb_amd import decay as D
            bins = one_plane(out)   # [n_bins, ny, nx], per band [K, n_bins, ny, nx]
            per_bin = plan["bin_captures"]
            extra = {}
            if decay_centres:   # per band: every map gets a leading band axis
                maps = D.band_decay_maps(bins, per_bin, args.decay_every, rate)
                extra = dict(band_centres_hz=np.array(decay_centres), band_edges_hz=np.array(D.octave_band_edges(decay_centres)))
            else:
                maps = D.decay_maps(bins, per_bin, args.decay_every, rate)
            np.savez(args.decay_out, bins=bins, bin_captures=per_bin, **shared, **extra, **maps)
            t30 = maps["t30_s"][np.isfinite(maps["t30_s"])]
            print("wrote decay maps of plane z=%d (%d bins of %d captures, %d captures; median T30 %s) to %s"
                  % (shared["plane"], bins.shape[-3], per_bin, captures, "%.3f s" % np.median(t30) if t30.size else "not defined", args.decay_out))
        if kind == "spectrum":
            np.savez(args.spectrum_out, spectrum=one_plane(out), freqs_hz=np.array(freqs_hz), captures=captures,
                     plane=spectrum_plane["plane"], z=spectrum_plane["z"])
            print("wrote %d complex maps of plane z=%d (%d captures) to %s" % (out.shape[0], spectrum_plane["plane"], captures, args.spectrum_out))
        if kind == "snapshots":
            fields, steps = audio_etc[3]
            os.makedirs(args.snapshot_out, exist_ok=True)
            for field, step in zip(fields, steps):
                np.save(os.path.join(args.snapshot_out, "step_%06d.npy" % int(step)), field[0])
            print("wrote %d snapshots of plane z=%d to %s" % (len(steps), plane, args.snapshot_out))
        audio, bands, vm = audio_etc[:3]
    dt = time.perf_counter() - t0
    mesh = vm.mesh
    print("mesh %dx%dx%d (%d nodes, spacing %.4f m), %d steps at %.1f Hz, %d samples at %.0f Hz, %.2f s wall"
          % (mesh.dims + (mesh.num_nodes, mesh.spacing, bands[0][0].shape[0], bands[0][1], audio.shape[0], args.rate, dt)))
    peak = write_wav(args.out, audio, args.rate)
    print("wrote %s (normalised, peak was %.3e)" % (args.out, peak))


if __name__ == "__main__":
    main()

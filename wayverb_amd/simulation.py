"""Caller glue around the engine: scene -> mesh -> run -> audio, in the
shape of the reference's host functions so that `src/combined`'s waveguide leg maps one to one.

  compute_voxels_and_mesh   src/waveguide/src/mesh.cpp:143-159 (+ compute_mesh, :54-141)
  canonical (single band)   src/waveguide/include/waveguide/canonical.h:29-127
  compute_index / locator   src/waveguide/src/mesh_descriptor.cpp:8-27
  single_band_parameters    src/waveguide/include/waveguide/simulation_parameters.h:9-16,65-68

Every stage that touches nodes runs on the GPU through the C ABI; there is no CPU path.
"""
import math

import numpy as np

from . import engine as E
from . import filters as F
from . import mesh as M
from . import postprocess as P
from . import scene as S


class Environment:
    """core::environment (src/core/include/core/environment.h:6-13)"""

    def __init__(self, speed_of_sound=340.0, acoustic_impedance=400.0):
        self.speed_of_sound = float(speed_of_sound)
        self.acoustic_impedance = float(acoustic_impedance)

    @property
    def ambient_density(self):
        return self.acoustic_impedance / self.speed_of_sound


def compute_sampling_frequency(cutoff, usable_portion):
    """single_band_parameters -> waveguide sample rate (simulation_parameters.h:65-68)"""
    return cutoff / (0.25 * usable_portion)


def grid_spacing(speed_of_sound, time_step):
    """config::grid_spacing (src/waveguide/src/config.cpp:23-25)"""
    return speed_of_sound * time_step * math.sqrt(3.0)


def compute_sample_rate(spacing, speed_of_sound):
    """compute_sample_rate (mesh_descriptor.cpp:70-72) = 1 / config::time_step"""
    return 1.0 / (spacing / (speed_of_sound * math.sqrt(3.0)))


class VoxelsAndMesh:
    """voxels_and_mesh (mesh.h): the voxelised scene the set-up kernels walked + the mesh."""

    def __init__(self, voxel_index, aabb, side, vertices, triangles, mesh, min_corner, surface_absorptions=None):
        self.surface_absorptions = surface_absorptions
        self.voxel_index = voxel_index
        self.aabb = aabb
        self.side = side
        self.vertices = vertices
        self.triangles = triangles
        self.mesh = mesh
        self.min_corner = np.asarray(min_corner, dtype=np.float32)

    def compute_locator(self, position):
        """compute_locator(descriptor, vec3) (mesh_descriptor.cpp:24-27): round((p - min) / spacing)"""
        t = (np.asarray(position, dtype=np.float32) - self.min_corner) / np.float32(self.mesh.spacing)
        # glm::round: half away from zero
        return tuple(int(v) for v in np.where(t >= 0, np.floor(t + np.float32(0.5)), np.ceil(t - np.float32(0.5))))

    def compute_index(self, position):
        x, y, z = self.compute_locator(position)
        return self.mesh.compute_index(x, y, z)

    def estimate_volume(self):
        """estimate_volume (mesh.cpp:40-49)"""
        inside = np.count_nonzero(self.mesh.nodes["boundary_type"] & M.ID_INSIDE)
        return float(self.mesh.spacing) ** 3 * inside


def compute_voxels_and_mesh(vertices, triangles, surface_absorptions, anchor, sample_rate, speed_of_sound,
                            octree_depth=5):
    """compute_voxels_and_mesh.  vertices float[n,4], triangles uint32[m,4] = {surface, v0, v1, v2},
    surface_absorptions [n_surfaces][8] band absorptions.  The mesh is laid so that a node
    coincides with `anchor` (the receiver, src/combined/src/engine.cpp:98-103)."""
    vertices = np.ascontiguousarray(vertices, dtype=np.float32)
    triangles = np.ascontiguousarray(triangles, dtype=np.uint32)
    spacing = np.float32(grid_spacing(speed_of_sound, 1.0 / sample_rate))   # passed on as float
    lo = vertices[:, :3].min(axis=0)
    hi = vertices[:, :3].max(axis=0)
    c0, c1 = S.compute_adjusted_boundary(lo, hi, np.asarray(anchor, dtype=np.float32), spacing)
    side = 1 << octree_depth
    vox = E.voxelise(vertices, triangles, (c0, c1), side)
    dims = tuple(int(v) for v in ((c1 - c0) / spacing).astype(np.int32))     # mesh.cpp:65-71
    # inside flags -> node types -> numbering -> surfaces per filter, chained in HBM (one call);
    # the host copy is what the Mesh object and the source / receiver placement checks read
    sm = E.SceneMesh(dims, c0, float(spacing), vox, (c0, c1), side, triangles, vertices)
    try:
        nodes, b = sm.fetch()
    finally:
        sm.close()
    n_surfaces = int(triangles[:, 0].max()) + 1
    absorptions = np.asarray(surface_absorptions, dtype=np.float64).reshape(-1, 8)
    if absorptions.shape[0] < n_surfaces:
        raise ValueError("scene uses %d surfaces but %d absorption sets were given" % (n_surfaces, absorptions.shape[0]))
    coeffs = np.zeros(absorptions.shape[0], dtype=M.coefficients_dtype)
    for i, a in enumerate(absorptions):
        coeffs[i] = F.surface_coefficients(a, speed_of_sound, float(spacing))   # mesh.cpp:126-138
    mesh = M.Mesh(dims, nodes, coeffs, b[0], b[1], b[2], spacing=float(spacing), min_corner=tuple(float(c) for c in c0))
    return VoxelsAndMesh(vox, (c0, c1), side, vertices, triangles, mesh, c0, absorptions)


def _keys_and_cadence(plan, who, keys, required=()):
    """What every plan dict of canonical's is checked for first: no key but `plane`, `box` and `keys`, one of `plane` and `box`, every
    one of `required` -- or the sentence that lists the keys -- and every >= 1.  Returns `every`."""
    if set(plan) - {"plane", "box"} - set(keys) or ("plane" in plan) == ("box" in plan) or any(k not in plan for k in required):
        raise ValueError("%s=dict(plane=<z in metres> or box=..., %s)" % (who, ", ".join(k + "=" for k in keys)))
    every = int(plan.get("every", 1))
    if every < 1:
        raise ValueError("%s: every must be >= 1" % who)
    return every


def _plane_or_box(plan, who, mesh, rimless):
    """The plan dict's box, or its `plane` (z in metres) as a box of the mesh: the whole horizontal plane, or, `rimless`, that plane less
    its rim, where every taken node has its six neighbours on the grid."""
    if "plane" not in plan:
        return plan["box"]
    plane = int(round((float(plan["plane"]) - mesh.min_corner[2]) / mesh.spacing))
    rim = 1 if rimless else 0
    if not rim <= plane <= mesh.dims[2] - 1 - rim:
        raise ValueError("%s: plane z=%g m %s" % (who, float(plan["plane"]),
                                                  "has no node with both neighbours in the mesh" if rimless else "is outside the mesh"))
    return ((1, 1, plane), (mesh.dims[0] - 2, mesh.dims[1] - 2, 1)) if rimless else ((0, 0, plane), (None, None, 1))


def octave_band_warnings(centres, edges, sample_rate, every, who="modulation: ", cadence="every=%d"):
    """What is to be said about octave bands the run cannot carry: a sentence per band whose upper edge lies above a quarter of the
    sample rate, where the waveguide is not trusted, and one per band above the Nyquist rate of the series captured every `every` steps,
    where it aliases.  `who` begins every sentence, `cadence` is how the caller spells `every`."""
    said = []
    for c, (lo, hi) in zip(centres, edges):
        if hi > 0.25 * sample_rate:
            said.append("%sthe %g Hz band reaches %.1f Hz, above a quarter of the sample rate (%.1f Hz): the waveguide is not trusted there"
                        % (who, c, hi, 0.25 * sample_rate))
        if hi > 0.5 * sample_rate / every:
            said.append("%sthe %g Hz band reaches %.1f Hz, above the Nyquist rate of the captured series (%.1f Hz with %s): it aliases"
                        % (who, c, hi, 0.5 * sample_rate / every, cadence % every))
    return said


def intensity_plan_arguments(intensity, mesh, sample_rate, environment, simulation_time):
    """canonical's `intensity` dict -> keyword arguments of Engine.set_intensity: dict(plane=z in metres | box=((x0, y0, z0), extent),
    stride=1, every=1, n_bins=None, bin_seconds=None).  `plane`: that horizontal plane less its rim (every taken node needs its six
    neighbours on the grid).  The bins are `bin_seconds` long (default: the run in `n_bins` bins, default 1); spacing, the rate of the
    captured series (sample_rate / every) and the environment's density are filled in."""
    every = _keys_and_cadence(intensity, "intensity", ("every", "n_bins", "bin_seconds", "stride", "first_step"))
    box = _plane_or_box(intensity, "intensity", mesh, rimless=True)
    captures = int(math.ceil(sample_rate * simulation_time)) // every + 1
    if intensity.get("bin_seconds") is not None:
        bin_captures = max(1, int(round(float(intensity["bin_seconds"]) * sample_rate / every)))
        n_bins = int(intensity["n_bins"]) if intensity.get("n_bins") is not None else max(1, min(4096, -(-captures // bin_captures)))
    else:
        n_bins = int(intensity.get("n_bins") or 1)
        bin_captures = max(1, -(-captures // n_bins))
    return dict(n_bins=n_bins, bin_captures=bin_captures, box=box, stride=intensity.get("stride", 1), first_step=int(intensity.get("first_step", 0)),
                period=every, spacing=mesh.spacing, sample_rate=sample_rate / every, ambient_density=environment.ambient_density)


def arrival_plan_arguments(arrival, mesh, sample_rate):
    """canonical's `arrival` dict -> keyword arguments of Engine.set_arrival: dict(plane=z in metres | box=((x0, y0, z0), extent),
    stride=1, every=1, threshold=, threshold_map=None, early_ms=(50, 80), first_step=0).  `plane`: that whole horizontal plane.  The
    bins begin at each node's onset and at every one of `early_ms` milliseconds behind it (arrival.edges_from_ms at the rate of the
    captured series, sample_rate / every); `threshold` is the pressure magnitude that counts as the arrival of the direct sound."""
    from . import arrival as A
    every = _keys_and_cadence(arrival, "arrival", ("threshold", "every", "early_ms", "threshold_map", "stride", "first_step"), required=("threshold",))
    box = _plane_or_box(arrival, "arrival", mesh, rimless=False)
    return dict(edges=A.edges_from_ms(arrival.get("early_ms", (50.0, 80.0)), every, sample_rate), threshold=float(arrival["threshold"]),
                threshold_map=arrival.get("threshold_map"), box=box, stride=arrival.get("stride", 1),
                first_step=int(arrival.get("first_step", 0)), period=every)


ARRIVAL_BANDS_KEYS = ("bands", "tail_ms", "tail_bin_ms", "lag")


def arrival_bands_plan_arguments(arrival, mesh, sample_rate):
    """canonical's `arrival` dict WITH `bands` -> keyword arguments of Engine.set_arrival_bands: everything arrival_plan_arguments takes,
    and bands=[(lo_hz, hi_hz), ...] (1 .. 8), tail_ms=None, tail_bin_ms=10, lag="group-delay" | 0.  Every band gets a 4th-order
    Butterworth band-pass designed at the rate of the CAPTURED series, sample_rate / every (decay.butterworth_bandpass); behind the
    early edges come uniform bins of tail_bin_ms out to tail_ms behind each node's onset (arrival.band_edges), from which
    arrival.band_decay_maps reads EDT / T20 / T30; "group-delay" starts every band's clock late by its cascade's group delay at the
    band's geometric centre, rounded to captures (arrival.lag_captures), 0 counts every band from the broadband onset."""
    from . import arrival as A
    from . import decay as D
    plain = arrival_plan_arguments({k: v for k, v in arrival.items() if k not in ARRIVAL_BANDS_KEYS}, mesh, sample_rate)
    bands = [(float(lo), float(hi)) for lo, hi in arrival["bands"]]
    lag = arrival.get("lag", "group-delay")
    if not 1 <= len(bands) <= 8 or any(not 0 < lo < hi for lo, hi in bands):
        raise ValueError("arrival: bands holds 1 .. 8 pairs (lo_hz, hi_hz) with 0 < lo < hi")
    if not (lag == "group-delay" or (not isinstance(lag, str) and int(lag) == 0)):
        raise ValueError('arrival: lag is "group-delay" or 0')
    every = plain["period"]
    series_rate = sample_rate / every
    sections = np.stack([D.butterworth_bandpass(lo, hi, series_rate) for lo, hi in bands])
    edges, tail = A.band_edges(arrival.get("early_ms", (50.0, 80.0)), arrival.get("tail_ms"), arrival.get("tail_bin_ms", 10.0), every, sample_rate)
    lags = [A.lag_captures(sections[k], math.sqrt(lo * hi), series_rate) if lag == "group-delay" else 0 for k, (lo, hi) in enumerate(bands)]
    return dict(plain, edges=edges, bands=sections, tail=tail, lag=lags)


def lateral_plan_arguments(lateral, mesh, sample_rate, environment):
    """canonical's `lateral` dict -> keyword arguments of Engine.set_lateral: dict(plane=z in metres | box=((x0, y0, z0), extent),
    stride=1, every=1, threshold=, threshold_map=None, edges_ms=(0, 5, 80), first_step=0).  `plane`: that horizontal plane less its
    rim (every taken node needs its six neighbours on the grid).  The bins begin at every one of `edges_ms` milliseconds behind each
    node's onset, the first of which is 0 (lateral.edges_from_ms at the rate of the captured series, sample_rate / every: with the
    default, bin 1 over bins 0 and 1 is J_LF's 5 .. 80 ms over 0 .. 80 ms); `threshold` is the pressure magnitude that counts as the
    arrival of the direct sound; spacing, the rate of the captured series and the environment's density are filled in."""
    from . import lateral as L
    every = _keys_and_cadence(lateral, "lateral", ("threshold", "every", "edges_ms", "threshold_map", "stride", "first_step"), required=("threshold",))
    edges_ms = [float(m) for m in lateral.get("edges_ms", (0.0, 5.0, 80.0))]
    if not edges_ms or edges_ms[0] != 0.0 or len(edges_ms) > L.MAX_BINS:
        raise ValueError("lateral: edges_ms begins with 0 and has 8 entries at the most")
    box = _plane_or_box(lateral, "lateral", mesh, rimless=True)
    return dict(edges=L.edges_from_ms(edges_ms[1:], every, sample_rate), threshold=float(lateral["threshold"]),
                threshold_map=lateral.get("threshold_map"), box=box, stride=lateral.get("stride", 1), first_step=int(lateral.get("first_step", 0)),
                period=every, spacing=mesh.spacing, sample_rate=sample_rate / every, ambient_density=environment.ambient_density)


def modulation_plan_arguments(modulation, mesh, sample_rate):
    """canonical's `modulation` dict -> keyword arguments of Engine.set_modulation: dict(plane=z in metres | box=((x0, y0, z0), extent),
    stride=1, every=1, bands_hz=(125, 250, 500), freqs_hz=modulation.STI_MODULATION_HZ, first_step=0).  `plane`: that whole horizontal
    plane.  The octave bands around `bands_hz` (decay.octave_band_edges) get a 4th-order Butterworth band-pass each, designed at the rate
    of the CAPTURED series, sample_rate / every (decay.butterworth_bandpass, which refuses a band at or above that series' Nyquist
    rate); the modulation frequencies become cycles per step of the mesh.  A band whose upper edge lies above a quarter of the sample
    rate, where the waveguide is not trusted, or above the captured series' Nyquist rate, where it aliases, is warned about."""
    import warnings
    from . import decay as D
    from . import modulation as MOD
    every = _keys_and_cadence(modulation, "modulation", ("every", "bands_hz", "freqs_hz", "stride", "first_step"))
    centres = [float(c) for c in np.atleast_1d(modulation.get("bands_hz", (125, 250, 500)))]
    freqs_hz = np.atleast_1d(np.asarray(modulation.get("freqs_hz", MOD.STI_MODULATION_HZ), dtype=np.float64))
    if not 1 <= len(centres) <= 8 or any(not c > 0 for c in centres):
        raise ValueError("modulation: bands_hz holds 1 .. 8 positive octave centres")
    if not 1 <= freqs_hz.shape[0] <= 16:
        raise ValueError("modulation: freqs_hz holds 1 .. 16 modulation frequencies")
    box = _plane_or_box(modulation, "modulation", mesh, rimless=False)
    series_rate = sample_rate / every
    edges = D.octave_band_edges(centres)
    for sentence in octave_band_warnings(centres, edges, sample_rate, every):
        warnings.warn(sentence)
    return dict(freqs=MOD.cycles_per_step(freqs_hz, sample_rate), bands=np.stack([D.butterworth_bandpass(lo, hi, series_rate) for lo, hi in edges]),
                box=box, stride=modulation.get("stride", 1), first_step=int(modulation.get("first_step", 0)), period=every)


WATERFALL_DEFAULT_BINS = 64     # bins of a waterfall plan that says only how long a bin is (bin_ms): the last is open-ended


def waterfall_plan_arguments(waterfall, mesh, sample_rate):
    """canonical's `waterfall` dict -> keyword arguments of Engine.set_waterfall: dict(freqs_hz=[...], plane=z in metres |
    box=((x0, y0, z0), extent), stride=1, every=1, bin_ms= | n_bins= and bin_captures=, first_step=0).  `plane`: that whole horizontal
    plane.  The frequencies (1 .. 64, in hertz) become cycles per step of the mesh, as spectrum_plan_arguments makes them; one above the
    Nyquist rate of the series captured every `every` steps, sample_rate / (2 every), would fold back onto a lower one: refused.  A bin
    is `bin_ms` milliseconds long, rounded to captures of that series and at least one (with n_bins= bins, by default 64 or as many as
    4096 sums per node allow), or `bin_captures` captures with `n_bins` of them; the last bin is open-ended either way."""
    every = _keys_and_cadence(waterfall, "waterfall", ("freqs_hz", "every", "bin_ms", "n_bins", "bin_captures", "stride", "first_step"), required=("freqs_hz",))
    freqs_hz = np.atleast_1d(np.asarray(waterfall["freqs_hz"], dtype=np.float64)).reshape(-1)
    if not 1 <= freqs_hz.shape[0] <= 64:
        raise ValueError("waterfall: freqs_hz holds 1 .. 64 frequencies")
    nyquist = float(sample_rate) / 2.0 / every
    for f in freqs_hz:
        if not 0.0 <= f <= nyquist:      # (a NaN is in no range)
            raise ValueError("waterfall: %.6g Hz is outside 0 .. %.6g Hz (half the sample rate %.6g Hz divided by every=%d)" % (f, nyquist, sample_rate, every))
    by_ms, by_captures = waterfall.get("bin_ms") is not None, waterfall.get("bin_captures") is not None
    if by_ms == by_captures or (by_captures and waterfall.get("n_bins") is None):
        raise ValueError("waterfall: a bin is bin_ms= long, or bin_captures= captures long with n_bins= of them")
    most = 4096 // freqs_hz.shape[0]
    if by_ms:
        bin_ms = float(waterfall["bin_ms"])
        if not (bin_ms > 0.0 and math.isfinite(bin_ms)):
            raise ValueError("waterfall: bin_ms must be > 0")
        bin_captures = max(1, int(round(bin_ms * 1e-3 * sample_rate / every)))
    else:
        bin_captures = int(waterfall["bin_captures"])
        if bin_captures < 1:
            raise ValueError("waterfall: bin_captures must be >= 1")
    n_bins = int(waterfall["n_bins"]) if waterfall.get("n_bins") is not None else min(WATERFALL_DEFAULT_BINS, most)
    if not 1 <= n_bins <= most:
        raise ValueError("waterfall: n_bins must be 1 .. %d with %d frequencies (4096 sums per node at the most)" % (most, freqs_hz.shape[0]))
    box = _plane_or_box(waterfall, "waterfall", mesh, rimless=False)
    return dict(freqs=freqs_hz / float(sample_rate), n_bins=n_bins, bin_captures=bin_captures, box=box, stride=waterfall.get("stride", 1),
                first_step=int(waterfall.get("first_step", 0)), period=every)


INTERAURAL_KEYS = ("threshold", "every", "edges_ms", "ear_axis", "ear_distance", "ears", "max_lag_ms", "band_hz", "threshold_map", "stride", "first_step")


def interaural_plan_arguments(interaural, mesh, sample_rate):
    """canonical's `interaural` dict -> keyword arguments of Engine.set_interaural: dict(plane=z in metres | box=((x0, y0, z0), extent),
    stride=1, every=1, threshold=, threshold_map=None, edges_ms=(0, 80), ear_axis=(0, 1, 0) with ear_distance=0.17 (metres) | ears=((x, y,
    z), (x, y, z)) in mesh nodes, max_lag_ms=1.0, band_hz=(lo, hi) | None, first_step=0).  `plane`: that whole horizontal plane (the ears
    of its outermost seats must still lie on the mesh: the engine refuses a plan one of whose ears leaves it).  The bins begin at every
    one of `edges_ms` milliseconds behind each node's onset, the first of which is 0 (with the default, bin 0 is IACC_E's 0 .. 80 ms, bin
    1 IACC_L's, both together IACC_A's); `threshold` is the pressure magnitude at either ear that counts as the arrival of the direct
    sound.  The ear distance is rounded to mesh nodes along the axis (interaural.ear_offsets): more than a quarter off the distance asked
    for is warned about.  The lags reach max_lag_ms at the rate of the captured series, sample_rate / every (interaural.max_lag): more
    than the engine's 16 captures are clipped to 16 with a warning -- a larger `every` reaches further.  `band_hz`: a 4th-order
    Butterworth band-pass both ears run through, designed at the rate of the captured series (decay.butterworth_bandpass).
    Checked in this order: the keys and `every`, edges_ms, the ears, max_lag_ms, band_hz, the plane."""
    import warnings
    from . import decay as D
    from . import interaural as IA
    every = _keys_and_cadence(interaural, "interaural", INTERAURAL_KEYS, required=("threshold",))
    edges_ms = [float(m) for m in interaural.get("edges_ms", (0.0, 80.0))]
    if not edges_ms or edges_ms[0] != 0.0 or len(edges_ms) > IA.MAX_BINS:
        raise ValueError("interaural: edges_ms begins with 0 and has 4 entries at the most")
    if interaural.get("ears") is not None:
        if "ear_axis" in interaural or "ear_distance" in interaural:
            raise ValueError("interaural: the ears are ears=((x, y, z), (x, y, z)) in mesh nodes, or ear_axis= and ear_distance= in metres")
        ears = [[int(v) for v in ear] for ear in interaural["ears"]]
        if len(ears) != 2 or any(len(ear) != 3 or any(abs(v) > IA.MAX_EAR for v in ear) for ear in ears):
            raise ValueError("interaural: ears holds two offsets (x, y, z) in mesh nodes, every component -8 .. 8")
        ear_a, ear_b = tuple(ears[0]), tuple(ears[1])
    else:
        distance = float(interaural.get("ear_distance", 0.17))
        try:
            ear_a, ear_b, rounded = IA.ear_offsets(mesh.spacing, interaural.get("ear_axis", (0.0, 1.0, 0.0)), distance)
        except ValueError:
            raise ValueError("interaural: ear_axis is a non-zero vector and ear_distance >= 0 metres")
        if any(abs(v) > IA.MAX_EAR for v in ear_a + ear_b):
            raise ValueError("interaural: ear_distance=%g m is more than 8 mesh nodes (spacing %g m) from the seat" % (distance, mesh.spacing))
        if abs(rounded - distance) > 0.25 * distance:
            warnings.warn("interaural: the ears are %g m apart on this mesh (spacing %g m), more than a quarter off the %g m asked for"
                          % (rounded, mesh.spacing, distance))
    lag_ms = float(interaural.get("max_lag_ms", 1.0))
    if not (lag_ms >= 0.0 and math.isfinite(lag_ms)):
        raise ValueError("interaural: max_lag_ms must be >= 0")
    lag = IA.max_lag(sample_rate, every, lag_ms)
    if lag > IA.MAX_LAG:
        warnings.warn("interaural: max_lag_ms=%g needs %d captures at every=%d, the engine holds 16: the lags end at %.3g ms"
                      % (lag_ms, lag, every, 16e3 * every / sample_rate))
        lag = IA.MAX_LAG
    sections = None
    if interaural.get("band_hz") is not None:
        band = tuple(float(v) for v in np.atleast_1d(interaural["band_hz"]))
        if len(band) != 2 or not 0 < band[0] < band[1]:
            raise ValueError("interaural: band_hz is (lo_hz, hi_hz) with 0 < lo < hi, or None")
        sections = D.butterworth_bandpass(band[0], band[1], sample_rate / every)
    box = _plane_or_box(interaural, "interaural", mesh, rimless=False)
    return dict(edges=IA.edges_from_ms(edges_ms[1:], every, sample_rate), ear_a=ear_a, ear_b=ear_b, max_lag=lag, threshold=float(interaural["threshold"]),
                sections=sections, threshold_map=interaural.get("threshold_map"), box=box, stride=interaural.get("stride", 1),
                first_step=int(interaural.get("first_step", 0)), period=every)


def _decay_plan(decay, mesh, sample_rate, environment, simulation_time):
    if decay.get("bands") is not None:
        from . import decay as D
        series_rate = sample_rate / int(decay.get("period", 1))
        decay = dict(decay, bands=np.stack([D.butterworth_bandpass(lo, hi, series_rate) for lo, hi in decay["bands"]]))
    return "decay", (), decay


def _arrival_plan(arrival, mesh, sample_rate, environment, simulation_time):
    if "bands" not in arrival:
        return "arrival", (), arrival_plan_arguments(arrival, mesh, sample_rate)
    plan = arrival_bands_plan_arguments(arrival, mesh, sample_rate)
    return "arrival_bands", (plan.pop("edges"), plan.pop("bands")), plan


# canonical's plan keywords in the order their plans are set and fetched: how (the caller's value, mesh, sample_rate, environment,
# simulation_time) becomes (<name>, positional, keyword arguments) of Engine.set_<name>, whose fetch is Engine.fetch_<name>
PLANS = (
    ("snapshots", lambda plan, *_: ("snapshots", (), plan)),
    ("spectrum", lambda plan, mesh, sample_rate, *_: ("spectrum", (), spectrum_plan_arguments(plan, sample_rate))),
    ("decay", _decay_plan),
    ("intensity", lambda plan, *run: ("intensity", (), intensity_plan_arguments(plan, *run))),
    ("arrival", _arrival_plan),
    ("lateral", lambda plan, mesh, sample_rate, environment, _: ("lateral", (), lateral_plan_arguments(plan, mesh, sample_rate, environment))),
    ("modulation", lambda plan, mesh, sample_rate, *_: ("modulation", (), modulation_plan_arguments(plan, mesh, sample_rate))),
    ("waterfall", lambda plan, mesh, sample_rate, *_: ("waterfall", (), waterfall_plan_arguments(plan, mesh, sample_rate))),
)
# (the plans that came after tests/test_waterfall_front.py and tests/test_waterfall_plan.py pinned PLANS row by row, the waterfall plan last:
# canonical and plan_call look in ALL_PLANS)
ALL_PLANS = PLANS + (
    ("interaural", lambda plan, mesh, sample_rate, *_: ("interaural", (), interaural_plan_arguments(plan, mesh, sample_rate))),
)


def plan_call(keyword, plan, mesh, sample_rate, environment, simulation_time):
    """What canonical does with the value of one plan keyword: (name, positional, keyword arguments) -- Engine.set_<name>(*positional,
    **keyword arguments) sets the plan, Engine.fetch_<name>() fetches it.  A banded arrival plan's bin edges are positional[0]."""
    return dict(ALL_PLANS)[keyword](plan, mesh, sample_rate, environment, simulation_time)


# what the refusal of slabs > 1 calls each of them, in the order it looks
SLABS_REFUSALS = {"modulation": "modulation maps are accumulated", "lateral": "lateral maps are accumulated", "arrival": "arrival maps are accumulated",
                  "intensity": "intensity bins are accumulated", "decay": "decay bins are accumulated", "snapshots": "snapshots are taken",
                  "spectrum": "a spectrum is accumulated", "waterfall": "waterfall sums are accumulated"}
# (and of the plans behind the pinned ones, as ALL_PLANS)
ALL_SLABS_REFUSALS = dict(SLABS_REFUSALS, interaural="interaural maps are accumulated")


def canonical(vm, source, receiver, environment, cutoff, usable_portion, simulation_time, precision="f64",
              device=-1, keep_going=lambda: True, slabs=1, devices=None, snapshots=None, spectrum=None, decay=None, intensity=None,
              arrival=None, lateral=None, modulation=None, waterfall=None, interaural=None):
    """canonical (single band): hard source at `source`, directional receiver at `receiver`, for
    ceil(sample_rate * simulation_time) steps.  Returns [(directional records, sample_rate,
    (0, cutoff))] -- the bandpass_band list waveguide::postprocess takes -- or None when stopped early.
    `precision`: "f32" is the reference's pressure type; "f64" the fp64 engine.
    `slabs` > 1: the mesh is cut into that many z-slabs, on the GPUs in `devices` (BASELINE configs[4], "1 -> 8
    GPUs"; engine.run_fast_slabs) -- same records, bit for bit.
    `snapshots`: keyword arguments of Engine.set_snapshots (box, stride, first_step, period, keep) -- the engine records that part
    of the field on the device while the run goes on (what the reference's visualiser takes from the per-step callback,
    src/combined/src/engine.cpp:158-169); the return value is then (bands, (float32[n, nz, ny, nx], steps[n])), or None when stopped
    early.  A snapshot of step s is the field after s completed steps: the hard source's sample of step s, which the reference's
    callback finds in the source node, is not in it yet (the C++ mirror, cl_mirror_cadence(), puts it there).  One domain only.
    `spectrum`: dict(freqs_hz=[...], box=..., stride=..., first_step=..., period=...) -- the engine Fourier-transforms that part of
    the field on the device at those frequencies while the run goes on (Engine.set_spectrum; Hz become cycles per step with the
    run's sample rate); the return value is then (bands, (complex128[K, nz, ny, nx], captures)).  One domain only, and not together
    with `snapshots`.
    `decay`: keyword arguments of Engine.set_decay (n_bins, bin_captures, box, stride, first_step, period) -- the engine sums the
    squared field of that box into time bins on the device while the run goes on; the return value is then (bands, (float64[n_bins,
    nz, ny, nx], captures)), which wayverb_amd.decay.decay_maps turns into EDT / T20 / T30 and level maps.  One domain only; together
    with `snapshots` or `spectrum` the engine refuses the second plan (engine.WaveguideError, with the plan to stop in its message).
    With `bands=[(lo_hz, hi_hz), ...]` in it (8 at the most) every node's captures go through a 4th-order Butterworth band-pass per
    band before the square (Engine.set_decay(bands=...); wayverb_amd.decay.butterworth_bandpass designs the sections at the rate of
    the captured series, sample_rate / period) and the bins are float64[K, n_bins, nz, ny, nx] (decay.band_decay_maps).
    `intensity`: dict(plane=<z in metres> or box=..., every=, n_bins=, bin_seconds=) (intensity_plan_arguments) -- the engine runs the
    directional receiver's integrator at every node of that plane or box and sums the sound intensity and the squared pressure into
    time bins on the device (Engine.set_intensity; spacing, sample_rate / every and the environment's density are filled in); the
    return value is then (bands, (float64[4, n_bins, nz, ny, nx], captures)), which wayverb_amd.intensity turns into direction and
    diffuseness maps.  One domain only, and not together with another plan.
    `arrival`: dict(plane=<z in metres> or box=..., every=, threshold=, early_ms=(50, 80)) (arrival_plan_arguments) -- the engine keeps,
    per node of that plane or box and on the device, the capture at which the direct sound arrived, the peak, and the squared pressure
    in bins counted from the node's OWN arrival (Engine.set_arrival); the return value is then (bands, (dict(onset, peak, peak_capture,
    pre, moment, bins), captures)), which wayverb_amd.arrival turns into arrival time, C50 / C80, D50 and centre time.  With
    bands=[(lo_hz, hi_hz), ...] in the dict (and tail_ms=, tail_bin_ms=, lag="group-delay" | 0: arrival_bands_plan_arguments) the plan is
    Engine.set_arrival_bands: pre, moment and bins per octave band, with a uniform tail for EDT / T20 / T30 from the same run.  One domain
    only, and not together with another plan.
    `lateral`: dict(plane=<z in metres> or box=..., every=, threshold=, edges_ms=(0, 5, 80)) (lateral_plan_arguments) -- the engine
    runs the directional receiver's integrator at every node of that plane or box and keeps, on the device and in bins counted from
    the node's OWN arrival, the squared pressure, the intensity and the second moments of the particle velocity (Engine.set_lateral);
    the return value is then (bands, (dict(onset, pre, velocity, bins), captures)), which wayverb_amd.lateral turns into the early
    lateral energy fraction, the direct sound's direction and the diffuseness.  One domain only, and not together with another plan.
    `modulation`: dict(plane=<z in metres> or box=..., every=, bands_hz=(125, 250, 500), freqs_hz=STI_MODULATION_HZ)
    (modulation_plan_arguments) -- the engine runs every node's captures through an octave band-pass per band and keeps, on the device,
    the band's energy and the Fourier sums of the squared output at the modulation frequencies (Engine.set_modulation); the return
    value is then (bands, ((energy float64[K, nz, ny, nx], sums complex128[K, M, nz, ny, nx]), captures)), which wayverb_amd.modulation
    turns into the modulation transfer function and the speech transmission index.  One domain only, and not together with another
    plan.
    `waterfall`: dict(freqs_hz=[...], plane=<z in metres> or box=..., every=, bin_ms= | n_bins= and bin_captures=)
    (waterfall_plan_arguments) -- the engine Fourier-transforms every node of that plane or box at those frequencies per time bin, on the
    device (Engine.set_waterfall); the return value is then (bands, (complex128[n_bins, K, nz, ny, nx], captures)), which
    wayverb_amd.waterfall turns into the short-time spectrum, the cumulative spectral decay and the decay time of single modes.  One
    domain only, and not together with another plan.
    `interaural`: dict(plane=<z in metres> or box=..., every=, threshold=, edges_ms=(0, 80), ear_axis=(0, 1, 0), ear_distance=0.17 |
    ears=((..), (..)), max_lag_ms=1.0, band_hz=(lo, hi) | None) (interaural_plan_arguments) -- for every node of that plane or box the
    engine correlates the field at two nodes an ear-distance apart, on the device, in bins counted from the node's own onset
    (Engine.set_interaural); the return value is then (bands, (dict(onset, pre, bins), captures)), which wayverb_amd.interaural turns into
    IACF, IACC_E / IACC_L / IACC_A and the lag of the maximum: ISO 3382-1 Annex B in its head-less (spaced omni) form -- not a dummy
    head.  One domain only, and not together with another plan."""
    asked = {keyword: plan for keyword, plan in (("snapshots", snapshots), ("spectrum", spectrum), ("decay", decay), ("intensity", intensity),
                                                 ("arrival", arrival), ("lateral", lateral), ("modulation", modulation), ("waterfall", waterfall),
                                                 ("interaural", interaural))
             if plan is not None}
    for keyword in ALL_SLABS_REFUSALS:
        if keyword in asked and slabs > 1:
            raise ValueError("%s on one domain only (slabs=1)" % ALL_SLABS_REFUSALS[keyword])
    if "spectrum" in asked and "snapshots" in asked:
        raise ValueError("a spectrum plan and a snapshot plan exclude each other")
    mesh = vm.mesh
    sample_rate = compute_sample_rate(mesh.spacing, environment.speed_of_sound)
    # (name of the Engine's plan, positional and keyword arguments of its set_*), in PLANS' order
    plans = [plan_call(keyword, asked[keyword], mesh, sample_rate, environment, simulation_time) for keyword, _ in ALL_PLANS if keyword in asked]

    def mesh_index(pt):
        idx = vm.compute_index(pt)
        if idx >= mesh.num_nodes or not (mesh.nodes["boundary_type"][idx] & M.ID_INSIDE):
            raise RuntimeError("Source/receiver node position appears to be outside mesh.")
        return idx

    ideal_steps = int(math.ceil(sample_rate * simulation_time))
    signal = np.zeros(ideal_steps, dtype=np.float64)
    if ideal_steps:
        signal[0] = np.float32(M.rectilinear_calibration_factor(mesh.spacing, environment.acoustic_impedance))
    receiver_index = mesh_index(receiver)
    neighbours = mesh.compute_neighbors(receiver_index)
    if any(n == 0xFFFFFFFF for n in neighbours):
        raise RuntimeError("Can't place directional_receiver at this node as it is adjacent to a boundary.")
    if slabs > 1:
        done, traces = E.run_fast_slabs(mesh, slabs, E.SOURCE_HARD, mesh_index(source), signal,
                                        [receiver_index] + list(neighbours), precision=precision,
                                        devices=devices or [device], keep_going=keep_going)
    else:
        eng = E.Engine(mesh, precision=precision, device=device)
        try:
            for name, positional, keywords in plans:
                getattr(eng, "set_" + name)(*positional, **keywords)
            done, traces = E.run_fast(eng, E.SOURCE_HARD, mesh_index(source), signal, [receiver_index] + list(neighbours),
                                      keep_going=keep_going)
            for name, _, _ in plans:   # (of two plans the later one's is returned)
                taken = (eng.fetch_modulation(), eng.modulation_count()[0]) if name == "modulation" else getattr(eng, "fetch_" + name)()
        finally:
            eng.close()
    if done != ideal_steps:
        return None
    directional = P.directional_receiver(traces, mesh.spacing, sample_rate, environment.ambient_density)
    bands = [(directional, sample_rate, (0.0, float(cutoff)))]
    return (bands, taken) if asked else bands


def spectrum_plan_arguments(spectrum, sample_rate):
    """canonical's `spectrum` dict -> keyword arguments of Engine.set_spectrum: freqs_hz / sample_rate = cycles per step.  The field is
    sampled every `period` steps, so a frequency above sample_rate / (2 * period) would fold back onto a lower one: refused."""
    plan = dict(spectrum)
    if "freqs_hz" not in plan:
        raise ValueError("spectrum: freqs_hz=[...] is required")
    freqs_hz = np.atleast_1d(np.asarray(plan.pop("freqs_hz"), dtype=np.float64))
    period = int(plan.get("period", 1))
    if period < 1:
        raise ValueError("spectrum: period must be >= 1")
    nyquist = float(sample_rate) / 2.0 / period
    for f in freqs_hz:
        if not np.isfinite(f):
            raise ValueError("spectrum: %r is not a frequency" % float(f))
        if not 0.0 <= f <= nyquist:
            alias = abs(f - round(f * period / sample_rate) * sample_rate / period)
            raise ValueError("spectrum: %.6g Hz is outside 0 .. %.6g Hz (half the sample rate %.6g Hz divided by period %d): "
                             "sampled every %d steps it aliases to %.6g Hz" % (f, nyquist, sample_rate, period, period, alias))
    plan["freqs"] = freqs_hz / float(sample_rate)
    return plan


def canonical_many(vm, source, receivers, environment, cutoff, usable_portion, simulation_time, precision="f64",
                   device=-1, keep_going=lambda: True, slabs=1, devices=None, chunk=1024):
    """canonical for MANY receivers out of ONE run of the mesh (the reference's application runs the whole mesh once per
    source-receiver pair, src/combined/src/threaded_engine.cpp:155-162; a run costs the same however many points listen): a list,
    one entry per receiver, of what canonical() returns for that receiver, bit for bit -- or None when stopped early.
    One domain: the receivers are recorded and integrated on the device (Engine.set_directional_receivers).  `slabs` > 1: the chain
    records the 7 columns of every receiver (engine.run_fast_slabs) and the library's host integrator turns them into the same
    records (postprocess.directional_accumulate)."""
    mesh = vm.mesh
    sample_rate = compute_sample_rate(mesh.spacing, environment.speed_of_sound)

    def mesh_index(pt):
        idx = vm.compute_index(pt)
        if idx >= mesh.num_nodes or not (mesh.nodes["boundary_type"][idx] & M.ID_INSIDE):
            raise RuntimeError("Source/receiver node position appears to be outside mesh.")
        return idx

    ideal_steps = int(math.ceil(sample_rate * simulation_time))
    signal = np.zeros(ideal_steps, dtype=np.float64)
    if ideal_steps:
        signal[0] = np.float32(M.rectilinear_calibration_factor(mesh.spacing, environment.acoustic_impedance))
    centres, columns = [], []
    for receiver in receivers:
        idx = mesh_index(receiver)
        neighbours = mesh.compute_neighbors(idx)
        if any(n == 0xFFFFFFFF for n in neighbours):
            raise RuntimeError("Can't place directional_receiver at this node as it is adjacent to a boundary.")
        centres.append(idx)
        columns += [idx] + list(neighbours)
    source_index = mesh_index(source)
    if not centres:
        return []
    if slabs > 1:
        done, traces = E.run_fast_slabs(mesh, slabs, E.SOURCE_HARD, source_index, signal, columns, precision=precision,
                                        devices=devices or [device], keep_going=keep_going, chunk=chunk)
        if done != ideal_steps:
            return None
        records = [P.directional_accumulate(traces[:, 7 * i:7 * i + 7], mesh.spacing, sample_rate, environment.ambient_density)
                   for i in range(len(centres))]
    else:
        eng = E.Engine(mesh, precision=precision, device=device)
        try:
            eng.set_source(E.SOURCE_HARD, source_index, signal)
            eng.set_directional_receivers(centres, mesh.spacing, sample_rate, environment.ambient_density)
            first = eng.step_count()
            done = 0
            while done < ideal_steps and keep_going():
                took, flag = eng.run_steps(min(chunk, ideal_steps - done))
                done += took
                E.raise_for_flag(flag)
                if took == 0:
                    break
            if done != ideal_steps:
                return None
            got = eng.fetch_directional(first, done)
        finally:
            eng.close()
        records = [np.ascontiguousarray(got[:, i]) for i in range(len(centres))]
    return [[(r, sample_rate, (0.0, float(cutoff)))] for r in records]


def band_edges_hz(bands=8, lo=20.0, hi=20000.0):
    """hrtf_band_params_hz().edges: band_edge_frequency(i, 8, {20, 20000})
    (src/frequency_domain/src/envelope.cpp:50-53, src/hrtf/lib/include/hrtf/multiband.h:22-25)"""
    return [lo * (hi / lo) ** (i / float(bands)) for i in range(bands + 1)]


def canonical_multiband(vm, source, receiver, environment, bands, cutoff, usable_portion, simulation_time,
                        precision="f64", device=-1, keep_going=lambda: True):
    """canonical for multiple_band_constant_spacing_parameters (canonical.h:138-176): one run per
    band with every surface's filter replaced by the flat filter of that band's absorption
    (set_flat_coefficients_for_band, :127-135); band i is valid on [edge_i, edge_i+1)."""
    if vm.surface_absorptions is None:
        raise ValueError("this VoxelsAndMesh carries no surface absorptions")
    edges = band_edges_hz()
    keep = vm.mesh.coefficients
    out = []
    try:
        for band in range(int(bands)):
            flat = np.zeros(len(vm.surface_absorptions), dtype=M.coefficients_dtype)
            for i, a in enumerate(vm.surface_absorptions):
                flat[i] = M.flat_coefficients(float(a[band]))
            vm.mesh.coefficients = flat
            r = canonical(vm, source, receiver, environment, cutoff, usable_portion, simulation_time, precision, device,
                          keep_going)
            if r is None:
                return None
            out.append((r[0][0], r[0][1], (edges[band], edges[band + 1])))
    finally:
        vm.mesh.coefficients = keep
    return out


def impulse_response(vertices, triangles, surface_absorptions, source, receiver, cutoff=200.0, usable_portion=0.6,
                     simulation_time=1.0, output_sample_rate=44100.0, environment=None, method=P.ATTENUATOR_NULL,
                     pointing=(0.0, 0.0, 1.0), shape=0.0, precision="f64", device=-1, snapshots=None, spectrum=None, decay=None,
                     intensity=None, arrival=None, lateral=None, modulation=None, waterfall=None, interaural=None):
    """The waveguide leg of combined::engine (engine.cpp:90-188) end to end: scene -> audio.
    `snapshots`: a function mesh -> keyword arguments of Engine.set_snapshots (the mesh's size is not known before it is built),
    or those arguments themselves; the return value then has the (snapshots, steps) pair as a fourth member.
    `spectrum`: a function mesh -> canonical's `spectrum` dict, or the dict; the fourth member is then (spectrum, captures).
    `decay`: a function (mesh, sample_rate) -> canonical's `decay` dict, or the dict; the fourth member is then (bins, captures).
    `intensity`: canonical's `intensity` dict; the fourth member is then (bins [4, n_bins, nz, ny, nx], captures).
    `arrival`: canonical's `arrival` dict; the fourth member is then (dict(onset, peak, peak_capture, pre, moment, bins), captures).
    `lateral`: canonical's `lateral` dict; the fourth member is then (dict(onset, pre, velocity, bins), captures).
    `modulation`: canonical's `modulation` dict; the fourth member is then ((energy, sums), captures).
    `waterfall`: canonical's `waterfall` dict; the fourth member is then (bins complex128[n_bins, K, nz, ny, nx], captures).
    `interaural`: canonical's `interaural` dict; the fourth member is then (dict(onset, pre, bins), captures)."""
    environment = environment or Environment()
    vm = compute_voxels_and_mesh(vertices, triangles, surface_absorptions, receiver,
                                 compute_sampling_frequency(cutoff, usable_portion), environment.speed_of_sound)
    if spectrum is not None and snapshots is not None:
        raise ValueError("a spectrum plan and a snapshot plan exclude each other")
    plans = {keyword: plan for keyword, plan in (("snapshots", snapshots), ("spectrum", spectrum), ("decay", decay), ("intensity", intensity),
                                                 ("arrival", arrival), ("lateral", lateral), ("modulation", modulation), ("waterfall", waterfall),
                                                 ("interaural", interaural))
             if plan is not None}
    for keyword in ("snapshots", "spectrum"):
        if callable(plans.get(keyword)):
            plans[keyword] = plans[keyword](vm.mesh)
    if callable(plans.get("decay")):
        plans["decay"] = decay(vm.mesh, compute_sample_rate(vm.mesh.spacing, environment.speed_of_sound))
    got = canonical(vm, source, receiver, environment, cutoff, usable_portion, simulation_time, precision, device, **plans)
    if plans and got is None:
        raise RuntimeError("the waveguide run was stopped early")
    bands, taken = got if plans else (got, None)
    audio = P.postprocess(bands, method, pointing, shape, environment.acoustic_impedance, output_sample_rate)
    return (audio, bands, vm) if taken is None else (audio, bands, vm, taken)


def impulse_responses(vertices, triangles, surface_absorptions, source, receivers, cutoff=200.0, usable_portion=0.6,
                      simulation_time=1.0, output_sample_rate=44100.0, environment=None, method=P.ATTENUATOR_NULL,
                      pointing=(0.0, 0.0, 1.0), shape=0.0, precision="f64", device=-1, slabs=1, devices=None):
    """impulse_response for several receivers out of one run of the mesh.  The mesh is anchored at the FIRST receiver (as the
    reference anchors it at its only one, engine.cpp:98-103): a node coincides with it; the others snap to their nearest node, as the
    source does (compute_index).  `method`, `pointing`, `shape` may be lists, one entry per receiver.
    Returns (audio per receiver, bands per receiver, the node positions used float32[R, 3], vm)."""
    environment = environment or Environment()
    receivers = [tuple(r) for r in receivers]
    if not receivers:
        raise ValueError("no receivers")
    vm = compute_voxels_and_mesh(vertices, triangles, surface_absorptions, receivers[0],
                                 compute_sampling_frequency(cutoff, usable_portion), environment.speed_of_sound)
    per = canonical_many(vm, source, receivers, environment, cutoff, usable_portion, simulation_time, precision, device,
                         slabs=slabs, devices=devices)
    if per is None:
        raise RuntimeError("the waveguide run was stopped early")

    def of(value, i, scalar):
        return value[i] if isinstance(value, (list, tuple)) and not scalar(value) else value

    is_vec = lambda v: len(v) == 3 and all(np.isscalar(c) for c in v)   # noqa: E731  (one pointing, not a list of them)
    never = lambda v: False   # noqa: E731
    audio = [P.postprocess(bands, of(method, i, never), of(pointing, i, is_vec), of(shape, i, never),
                           environment.acoustic_impedance, output_sample_rate) for i, bands in enumerate(per)]
    positions = np.stack([vm.min_corner + np.asarray(vm.compute_locator(r), dtype=np.float32) * np.float32(vm.mesh.spacing)
                          for r in receivers])
    return audio, per, positions, vm

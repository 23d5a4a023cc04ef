"""ctypes binding of the C ABI (include/wayverb_amd.h) + a Python mirror of `waveguide::run`.

The library is the product; this file is plumbing.  There is no fallback: if
libwayverb_amd.so is missing or no HIP device is visible, constructing an Engine raises.
"""
import ctypes as C
import os

import numpy as np

from . import mesh as M

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libwayverb_amd.so")

WV_OK = 0
PRECISION_F32 = 0
PRECISION_F64 = 1
BUF_CURRENT = 0
BUF_PREVIOUS = 1
SOURCE_NONE, SOURCE_HARD, SOURCE_SOFT = 0, 1, 2
NO_NODE = 0xFFFFFFFFFFFFFFFF
DIRECTIONAL_OUTPUT_DTYPE = np.dtype([("intensity", "<f4", (3,)), ("pressure", "<f4")])   # wv_directional_output
UNIQUE_ID_BYTES = 128

EXPORTS = [
    "wv_create", "wv_destroy", "wv_last_error", "wv_default_options", "wv_read_value", "wv_write_value",
    "wv_read_field", "wv_write_field", "wv_read_planes", "wv_write_planes", "wv_read_boundary_data", "wv_write_boundary_data",
    "wv_set_coefficients", "wv_device_buffer", "wv_step", "wv_swap", "wv_set_source",
    "wv_set_receivers", "wv_run", "wv_fetch_receivers", "wv_step_count", "wv_kernel_time_ms",
    "wv_enable_kernel_timing", "wv_kernel_time_detail", "wv_query", "wv_measure_triad", "wv_synchronize", "wv_comm_unique_id", "wv_comm_init",
    "wv_comm_destroy", "wv_comm_use_library", "wv_comm_init_local", "wv_run_group", "wv_make_box_nodes", "wv_set_stream_tuning", "wv_filter_test_2", "wv_field_pitch", "wv_classify_nodes", "wv_voxelise", "wv_nodes_inside",
    "wv_boundary_index_data", "wv_arbitrary_magnitude_filter", "wv_is_stable", "wv_band_centres",
    "wv_reflectance_filter", "wv_impedance_coefficients", "wv_attenuate", "wv_adjust_sampling_rate",
    "wv_frequency_domain_filter", "wv_postprocess_waveguide", "wv_hrtf_attenuation", "wv_hrtf_ear_position",
    "wv_attenuate_hrtf", "wv_multiband_filter_and_mixdown", "wv_postprocess_waveguide_hrtf", "wv_scene_mesh_create", "wv_scene_mesh_fetch",
    "wv_scene_mesh_create_engine", "wv_scene_mesh_destroy", "wv_checkpoint", "wv_rollback", "wv_drop_checkpoint", "wv_host_register", "wv_host_unregister",
    "wv_compressed_waveguide_run", "wv_make_transparent", "wv_set_snapshots", "wv_snapshot_count", "wv_fetch_snapshots",
    "wv_set_directional_receivers", "wv_fetch_directional", "wv_directional_accumulate",
    "wv_set_spectrum", "wv_spectrum_count", "wv_fetch_spectrum", "wv_spectrum_twiddle",
    "wv_set_decay", "wv_decay_count", "wv_fetch_decay",
    "wv_set_decay_bands", "wv_fetch_decay_bands", "wv_biquad_run", "wv_butterworth_bandpass", "wv_bandpass_biquad",
    "wv_set_intensity", "wv_intensity_count", "wv_fetch_intensity", "wv_fetch_intensity_velocity", "wv_fetch_directional_velocity",
    "wv_set_arrival", "wv_arrival_count", "wv_fetch_arrival",
    "wv_set_lateral", "wv_lateral_count", "wv_fetch_lateral",
    "wv_set_modulation", "wv_modulation_count", "wv_fetch_modulation",
    "wv_set_arrival_bands", "wv_arrival_bands_count", "wv_fetch_arrival_bands",
    "wv_set_waterfall", "wv_waterfall_count", "wv_fetch_waterfall",
    "wv_set_interaural", "wv_interaural_count", "wv_fetch_interaural",
]


class WvMesh(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("nodes", C.c_void_p), ("coefficients", C.c_void_p), ("num_coefficients", C.c_uint32),
                ("boundary_indices_1", C.c_void_p), ("boundary_indices_2", C.c_void_p),
                ("boundary_indices_3", C.c_void_p),
                ("num_boundary_1", C.c_uint64), ("num_boundary_2", C.c_uint64), ("num_boundary_3", C.c_uint64)]


TUNING_FIELDS = ("pair", "pair_chunks", "pair_inner_fix", "pair_wide", "pair_unit_waves", "pair_unit_planes", "pair_units_by_chunk", "tile_lists",
                 "fuse_pre_post", "graph", "boundary_lds", "boundary_order", "boundary_xwall",
                 "stream_ry", "stream_nwx", "stream_nwy", "stream_zchunks", "slab_early", "pair_split_rows", "fuse_planes", "whole_step", "triple",
                 "triple_chunks", "triple_lanes")


class WvTuning(C.Structure):
    """wv_tuning (include/wayverb_amd.h): how the engine does its work, never what it computes."""
    _fields_ = [(name, C.c_int32) for name in TUNING_FIELDS]


class WvOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("precision", C.c_int32), ("device", C.c_int32),
                ("ghost_lo", C.c_int32), ("ghost_hi", C.c_int32), ("flag_interval", C.c_int32),
                ("stream_variant", C.c_int32), ("all_tiles", C.c_int32), ("nodes_on_device", C.c_int32), ("comm_timeout_s", C.c_int32), ("transport", C.c_int32), ("reserved_", C.c_int32 * 5),
                ("tuning", WvTuning)]


# what every capture plan begins with: a box of the mesh, a stride per axis, a cadence in steps
_BOX_AND_CADENCE = [(name, C.c_int32) for name in ("x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz")] + [("first_step", C.c_uint64), ("period", C.c_uint64)]


class WvSnapshotPlan(C.Structure):
    """wv_snapshot_plan (include/wayverb_amd.h): a box of the mesh, a stride per axis, a cadence in steps."""
    _fields_ = _BOX_AND_CADENCE + [("keep", C.c_uint32), ("reserved", C.c_uint32)]


class WvSpectrumPlan(C.Structure):
    """wv_spectrum_plan (include/wayverb_amd.h): the snapshot plan's box, strides and cadence, and the number of frequencies."""
    _fields_ = _BOX_AND_CADENCE + [("n_freqs", C.c_uint32), ("reserved", C.c_uint32)]


class WvDecayPlan(C.Structure):
    """wv_decay_plan (include/wayverb_amd.h): the snapshot plan's box, strides and cadence, the number of time bins and the captures
    per bin."""
    _fields_ = _BOX_AND_CADENCE + [("n_bins", C.c_uint32), ("bin_captures", C.c_uint32)]


class WvIntensityPlan(C.Structure):
    """wv_intensity_plan (include/wayverb_amd.h): wv_decay_plan's fields, then the three arguments of the reference's
    directional_receiver constructor."""
    _fields_ = WvDecayPlan._fields_ + [("spacing", C.c_double), ("sample_rate", C.c_double), ("ambient_density", C.c_double)]


class WvArrivalPlan(C.Structure):
    """wv_arrival_plan (include/wayverb_amd.h): the box and the cadence as wv_decay_plan has them, then n_bins, the scalar threshold
    and the 16 bin edges in captures behind a node's onset."""
    _fields_ = _BOX_AND_CADENCE + [("n_bins", C.c_uint32), ("threshold", C.c_float), ("edges", C.c_uint32 * 16)]


class WvLateralPlan(C.Structure):
    """wv_lateral_plan (include/wayverb_amd.h): the box and the cadence as wv_decay_plan has them, n_bins, the scalar threshold and
    the 8 bin edges in captures behind a node's onset, then the three arguments of the reference's directional_receiver constructor."""
    _fields_ = _BOX_AND_CADENCE + [("n_bins", C.c_uint32), ("threshold", C.c_float), ("edges", C.c_uint32 * 8),
                                   ("spacing", C.c_double), ("sample_rate", C.c_double), ("ambient_density", C.c_double)]


class WvModulationPlan(C.Structure):
    """wv_modulation_plan (include/wayverb_amd.h): the spectrum plan's fields -- box, strides, cadence, the number of modulation
    frequencies."""
    _fields_ = WvSpectrumPlan._fields_


class WvArrivalBandsPlan(C.Structure):
    """wv_arrival_bands_plan (include/wayverb_amd.h): the box and the cadence as wv_decay_plan has them, n_edges, the scalar threshold and
    the 16 explicit edges as wv_arrival_plan has n_bins and its edges, then the uniform tail, the lag per band and a reserved word."""
    _fields_ = _BOX_AND_CADENCE + [("n_edges", C.c_uint32), ("threshold", C.c_float), ("edges", C.c_uint32 * 16),
                                   ("n_tail", C.c_uint32), ("tail_first", C.c_uint32), ("tail_captures", C.c_uint32),
                                   ("lag", C.c_uint32 * 8), ("reserved", C.c_uint32)]


class WvWaterfallPlan(C.Structure):
    """wv_waterfall_plan (include/wayverb_amd.h): the spectrum plan's box, strides, cadence and number of frequencies, then the decay
    plan's number of time bins and captures per bin, and a reserved word."""
    _fields_ = _BOX_AND_CADENCE + [("n_freqs", C.c_uint32), ("n_bins", C.c_uint32), ("bin_captures", C.c_uint32), ("reserved", C.c_uint32)]


class WvInterauralPlan(C.Structure):
    """wv_interaural_plan (include/wayverb_amd.h): box, strides and cadence, the two ear offsets in mesh nodes, the largest lag, the
    arrival plan's number of bins, threshold and edges (four of them), and the number of biquad sections both ears share."""
    _fields_ = _BOX_AND_CADENCE + [("ear_a", C.c_int32 * 3), ("ear_b", C.c_int32 * 3), ("max_lag", C.c_uint32), ("n_bins", C.c_uint32),
                                   ("threshold", C.c_float), ("edges", C.c_uint32 * 4), ("n_sections", C.c_uint32)]


ARRIVAL_NONE = 0xFFFFFFFF   # onset / peak_capture of a node that has none yet

# The capture plans as this layer remembers them (Engine.<name>_shape) and as the library counts them (wv_<name>_count) ...
PLAN_NAMES = ("snapshot", "spectrum", "decay", "intensity", "arrival", "lateral", "modulation", "arrival_bands", "interaural", "waterfall")
# ... and their calls: wv_set_<key>(engine, plan, *what is listed first) and wv_fetch_<key>(engine, *what is listed second)
_POINTER, _WORD, _RESULT = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)
_PLAN_CALLS = {
    "snapshots": (WvSnapshotPlan, [], [C.c_uint64, C.c_uint64, _POINTER, _POINTER]),
    "spectrum": (WvSpectrumPlan, [_POINTER], [_POINTER, _RESULT]),
    "decay": (WvDecayPlan, [], [_POINTER, _RESULT]),
    "decay_bands": (WvDecayPlan, [_POINTER, _WORD, _WORD], [_POINTER, _RESULT]),
    "intensity": (WvIntensityPlan, [], [_POINTER, _RESULT]),
    "arrival": (WvArrivalPlan, [_POINTER], [_POINTER] * 6 + [_RESULT]),
    "lateral": (WvLateralPlan, [_POINTER], [_POINTER] * 4 + [_RESULT]),
    "modulation": (WvModulationPlan, [_POINTER, _POINTER, _WORD, _WORD], [_POINTER, _POINTER, _RESULT]),
    "arrival_bands": (WvArrivalBandsPlan, [_POINTER, _POINTER, _WORD, _WORD], [_POINTER] * 6 + [_RESULT]),
    # (tests/test_waterfall_plan.py pins the waterfall plan as the last name and the last row: a later plan stands ahead of it)
    "interaural": (WvInterauralPlan, [_POINTER, _POINTER], [_POINTER] * 3 + [_RESULT]),
    "waterfall": (WvWaterfallPlan, [_POINTER], [_POINTER, _RESULT]),
}


# Tuning applied to every engine this module creates unless the call says otherwise: {field of wv_tuning: value}, plus
# "stream_variant" (wv_options).  Empty = the library's defaults.  Tests and tools steer the engine through this (the
# library itself reads no environment variables).
default_tuning = {}


def tuning_from_env(environ=None):
    """For the scripts under tools/: WV_PAIR=0 WV_STREAM_RY=2 ... in the environment -> a tuning dict."""
    environ = os.environ if environ is None else environ
    out = {}
    for name in TUNING_FIELDS + ("stream_variant",):
        v = environ.get("WV_" + name.upper())
        if v is not None:
            out[name] = int(v)
    return out


def apply_tuning(opt, tuning=None):
    merged = dict(default_tuning)
    merged.update(tuning or {})
    for name, value in merged.items():
        if name == "stream_variant":
            opt.stream_variant = int(value)
        elif name in TUNING_FIELDS:
            setattr(opt.tuning, name, int(value))
        else:
            raise ValueError("unknown tuning field %r" % name)


class WaveguideError(RuntimeError):
    pass


class ValueIsInf(WaveguideError):
    """core::exceptions::value_is_inf (src/core/include/core/exceptions.h:28-30)"""


class ValueIsNan(WaveguideError):
    """core::exceptions::value_is_nan (exceptions.h:24-26)"""


_lib = None


def load_library():
    """Load libwayverb_amd.so.  If torch is installed it is imported first so that both share
    one HIP runtime (torch bundles its own libamdhip64 with the same soname)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise WaveguideError(
            "%s not built: run `python -m wayverb_amd.build` (there is no CPU fallback)" % _LIB_PATH)
    if os.environ.get("WV_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
    lib.wv_last_error.restype = C.c_char_p
    lib.wv_create.argtypes = [C.POINTER(WvMesh), C.POINTER(WvOptions), C.POINTER(C.c_void_p)]
    lib.wv_destroy.argtypes = [C.c_void_p]
    lib.wv_destroy.restype = None
    lib.wv_default_options.argtypes = [C.POINTER(WvOptions)]
    lib.wv_default_options.restype = None
    lib.wv_read_value.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_double)]
    lib.wv_write_value.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_double]
    lib.wv_read_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.wv_write_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.wv_read_planes.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_int]
    lib.wv_write_planes.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_int]
    lib.wv_read_boundary_data.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.wv_write_boundary_data.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.wv_set_coefficients.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.wv_device_buffer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.wv_step.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.wv_checkpoint.argtypes = [C.c_void_p]
    lib.wv_rollback.argtypes = [C.c_void_p]
    lib.wv_drop_checkpoint.argtypes = [C.c_void_p]
    lib.wv_swap.argtypes = [C.c_void_p]
    lib.wv_set_source.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.wv_set_receivers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.wv_run.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    lib.wv_fetch_receivers.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.wv_step_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.wv_kernel_time_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.wv_enable_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    lib.wv_kernel_time_detail.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.wv_synchronize.argtypes = [C.c_void_p]
    lib.wv_set_stream_tuning.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.wv_filter_test_2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.wv_field_pitch.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.wv_classify_nodes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.wv_comm_unique_id.argtypes = [C.c_void_p]
    lib.wv_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.wv_comm_destroy.argtypes = [C.c_void_p]
    lib.wv_comm_init_local.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
    lib.wv_run_group.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    lib.wv_make_box_nodes.argtypes = [C.c_int32] * 7 + [C.c_void_p, C.POINTER(C.c_uint64)]
    for key, (plan, beside_the_plan, fetched) in _PLAN_CALLS.items():
        getattr(lib, "wv_set_" + key).argtypes = [C.c_void_p, C.POINTER(plan)] + beside_the_plan
        getattr(lib, "wv_fetch_" + key).argtypes = [C.c_void_p] + fetched
    for name in PLAN_NAMES:
        getattr(lib, "wv_%s_count" % name).argtypes = [C.c_void_p, _RESULT, _RESULT]
    lib.wv_spectrum_twiddle.argtypes = [C.c_double, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.wv_spectrum_twiddle.restype = None
    lib.wv_fetch_intensity_velocity.argtypes = [C.c_void_p, C.c_void_p]
    lib.wv_fetch_directional_velocity.argtypes = [C.c_void_p, C.c_void_p]
    lib.wv_biquad_run.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.wv_butterworth_bandpass.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.wv_bandpass_biquad.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.wv_set_directional_receivers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_double]
    lib.wv_fetch_directional.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.wv_directional_accumulate.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def _check(rc):
    if rc != WV_OK:
        raise WaveguideError("wayverb_amd error %d: %s" % (rc, load_library().wv_last_error().decode()))


def spectrum_twiddle(cycles_per_step, step):
    """wv_spectrum_twiddle: (cos, sin) of 2 pi frac(cycles_per_step * step), the very doubles the engine folds a capture of `step`
    with at that frequency (Engine.set_spectrum)."""
    c, s = C.c_double(), C.c_double()
    load_library().wv_spectrum_twiddle(float(cycles_per_step), int(step), C.byref(c), C.byref(s))
    return c.value, s.value


def raise_for_flag(flag):
    """The flag -> exception mapping of waveguide.h:102-118."""
    if flag & M.ERR_INF:
        raise ValueIsInf("Pressure value is inf, check filter coefficients.")
    if flag & M.ERR_NAN:
        raise ValueIsNan("Pressure value is nan, check filter coefficients.")
    if flag & M.ERR_OUTSIDE_MESH:
        raise WaveguideError("Tried to read non-existant node.")
    if flag & M.ERR_SUSPICIOUS_BOUNDARY:
        raise WaveguideError("Suspicious boundary read.")


def make_box_nodes(nx, ny, nz_global, z_begin=0, z_count=None, number_from=None, number_to=None):
    """wv_make_box_nodes -> (nodes[z_count*ny*nx], (n1, n2, n3))."""
    lib = load_library()
    if z_count is None:
        z_count = nz_global - z_begin
    if number_from is None:
        number_from = z_begin
    if number_to is None:
        number_to = z_begin + z_count
    nodes = np.empty(z_count * ny * nx, dtype=M.condensed_node_dtype)
    counts = (C.c_uint64 * 3)()
    _check(lib.wv_make_box_nodes(nx, ny, nz_global, z_begin, z_count, number_from, number_to,
                                 nodes.ctypes.data_as(C.c_void_p), counts))
    return nodes, tuple(int(c) for c in counts)


def classify_nodes(inside_mask):
    """wv_classify_nodes: inside mask [nz, ny, nx] -> (condensed nodes, (n1, n2, n3))."""
    lib = load_library()
    mask = np.ascontiguousarray(inside_mask, dtype=np.uint8)
    nz, ny, nx = mask.shape
    nodes = np.zeros(nx * ny * nz, dtype=M.condensed_node_dtype)
    counts = (C.c_uint64 * 3)()
    _check(lib.wv_classify_nodes(nx, ny, nz, mask.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p), counts))
    return nodes, tuple(int(c) for c in counts)


def voxelise(vertices, triangles, aabb, side=32):
    """wv_voxelise: flattened voxel -> triangle lists (uint32 array) for a triangle soup.
    vertices float32[n, 4] (cl_float3), triangles uint32[m, 4] = {surface, v0, v1, v2}."""
    lib = load_library()
    lib.wv_voxelise.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    t = np.ascontiguousarray(triangles, dtype=np.uint32)
    a0 = np.ascontiguousarray(aabb[0], dtype=np.float32)
    a1 = np.ascontiguousarray(aabb[1], dtype=np.float32)
    need = C.c_uint64()
    args = [v.ctypes.data_as(C.c_void_p), v.shape[0], t.ctypes.data_as(C.c_void_p), t.shape[0],
            a0.ctypes.data_as(C.c_void_p), a1.ctypes.data_as(C.c_void_p), side]
    _check(lib.wv_voxelise(*args, None, 0, C.byref(need)))
    out = np.zeros(need.value, dtype=np.uint32)
    _check(lib.wv_voxelise(*args, out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(need)))
    return out


def nodes_inside(dims, min_corner, spacing, voxel_index, aabb, side, triangles, vertices):
    """wv_nodes_inside: uint8 inside mask [nz, ny, nx] of the mesh nodes."""
    lib = load_library()
    lib.wv_nodes_inside.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_uint64,
                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.c_void_p]
    nx, ny, nz = dims
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    t = np.ascontiguousarray(triangles, dtype=np.uint32)
    vox = np.ascontiguousarray(voxel_index, dtype=np.uint32)
    mc = np.ascontiguousarray(min_corner, dtype=np.float32)
    a0 = np.ascontiguousarray(aabb[0], dtype=np.float32)
    a1 = np.ascontiguousarray(aabb[1], dtype=np.float32)
    out = np.zeros(nx * ny * nz, dtype=np.uint8)
    _check(lib.wv_nodes_inside(nx, ny, nz, mc.ctypes.data_as(C.c_void_p), float(spacing), vox.ctypes.data_as(C.c_void_p),
                               vox.shape[0], a0.ctypes.data_as(C.c_void_p), a1.ctypes.data_as(C.c_void_p), side,
                               t.ctypes.data_as(C.c_void_p), t.shape[0], v.ctypes.data_as(C.c_void_p), v.shape[0],
                               out.ctypes.data_as(C.c_void_p)))
    return out.reshape(nz, ny, nx)


def boundary_index_data(dims, min_corner, spacing, nodes, triangles, vertices):
    """wv_boundary_index_data: surface index per boundary filter.  `nodes` (types set) get their
    final boundary_index in place.  Returns [b1 [n1,1], b2 [n2,2], b3 [n3,3]] uint32."""
    lib = load_library()
    lib.wv_boundary_index_data.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    nx, ny, nz = dims
    assert nodes.dtype == M.condensed_node_dtype and nodes.flags.c_contiguous and nodes.shape[0] == nx * ny * nz
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    t = np.ascontiguousarray(triangles, dtype=np.uint32)
    mc = np.ascontiguousarray(min_corner, dtype=np.float32)
    counts = (C.c_uint64 * 3)()
    args = (nx, ny, nz, mc.ctypes.data_as(C.c_void_p), float(spacing), nodes.ctypes.data_as(C.c_void_p),
            t.ctypes.data_as(C.c_void_p), t.shape[0], v.ctypes.data_as(C.c_void_p), v.shape[0])
    _check(lib.wv_boundary_index_data(*args, None, 0, None, 0, None, 0, counts))     # size query
    cap = [max(1, int(counts[d])) for d in range(3)]
    out = [np.zeros((cap[d], d + 1), dtype=np.uint32) for d in range(3)]
    _check(lib.wv_boundary_index_data(*args, out[0].ctypes.data_as(C.c_void_p), cap[0],
                                      out[1].ctypes.data_as(C.c_void_p), cap[1],
                                      out[2].ctypes.data_as(C.c_void_p), cap[2], counts))
    return [out[d][:int(counts[d])].copy() for d in range(3)]


def measure_triad(device=-1, n_doubles=1 << 28, iters=10):
    """wv_measure_triad: GB/s of the device triad (2 reads + 1 write per element)."""
    lib = load_library()
    lib.wv_measure_triad.argtypes = [C.c_int32, C.c_uint64, C.c_int32, C.POINTER(C.c_double)]
    out = C.c_double()
    _check(lib.wv_measure_triad(device, n_doubles, iters, C.byref(out)))
    return out.value


def filter_test_2(inputs, memory, coeffs):
    """wv_filter_test_2: inputs float32[n_samples, n_filters]; memory float64[n_filters, 6] is
    advanced in place; returns outputs float32[n_samples, n_filters]."""
    lib = load_library()
    inputs = np.ascontiguousarray(inputs, dtype=np.float32)
    coeffs = np.ascontiguousarray(coeffs, dtype=M.coefficients_dtype)
    assert memory.dtype == np.float64 and memory.flags.c_contiguous
    out = np.zeros_like(inputs)
    _check(lib.wv_filter_test_2(inputs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                memory.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p),
                                inputs.shape[1], inputs.shape[0]))
    return out


class Engine:
    """One `run` worth of device state: the buffers of waveguide.h:43-76."""

    def __init__(self, mesh, precision="f64", device=-1, ghost_lo=False, ghost_hi=False,
                 flag_interval=0, stream_variant=2, all_tiles=False, tuning=None, comm_timeout_s=0, transport="rccl"):
        self.lib = load_library()
        self.mesh = mesh
        self.precision = precision
        self.dtype = np.float32 if precision == "f32" else np.float64
        nx, ny, nz = mesh.dims
        wm = WvMesh()
        wm.nx, wm.ny, wm.nz = nx, ny, nz
        wm.nodes = mesh.nodes.ctypes.data
        wm.coefficients = mesh.coefficients.ctypes.data
        wm.num_coefficients = mesh.coefficients.shape[0]
        for d in range(3):
            setattr(wm, "boundary_indices_%d" % (d + 1), mesh.bidx[d].ctypes.data if mesh.bidx[d].size else None)
            setattr(wm, "num_boundary_%d" % (d + 1), mesh.bidx[d].shape[0])
        opt = WvOptions()
        self.lib.wv_default_options(C.byref(opt))
        opt.precision = PRECISION_F32 if precision == "f32" else PRECISION_F64
        opt.device = device
        opt.ghost_lo = int(ghost_lo)
        opt.ghost_hi = int(ghost_hi)
        opt.flag_interval = flag_interval
        opt.stream_variant = stream_variant
        opt.all_tiles = 1 if all_tiles else 0
        opt.transport = {"rccl": 0, "ipc": 1}[transport]   # wv_comm_init chains: how the face planes travel (WV_TRANSPORT_*)
        opt.comm_timeout_s = int(comm_timeout_s)   # RCCL chains: seconds before a rank gives up on its peers (0: 180 s, < 0: never)
        apply_tuning(opt, tuning)
        handle = C.c_void_p()
        _check(self.lib.wv_create(C.byref(wm), C.byref(opt), C.byref(handle)))
        self.h = handle
        self.n_recv = 0
        self.n_directional = 0
        self._plan_state()

    @classmethod
    def from_handle(cls, handle, mesh, precision):
        """Wrap an engine the library has already created (SceneMesh.engine)."""
        eng = cls.__new__(cls)
        eng.lib = load_library()
        eng.mesh = mesh
        eng.precision = precision
        eng.dtype = np.float32 if precision == "f32" else np.float64
        eng.h = handle
        eng.n_recv = 0
        eng.n_directional = 0
        eng._plan_state()
        return eng

    def _plan_state(self):
        """What this layer remembers of the capture plans: the shape a fetch returns, None while the plan is not set."""
        for name in PLAN_NAMES:
            if not hasattr(type(self), name + "_shape"):   # (waterfall_shape, interaural_shape: the class has their None)
                setattr(self, name + "_shape", None)
        self.decay_banded = False

    def close(self):
        if getattr(self, "h", None):
            self.lib.wv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- buffer helpers (core::read_value / write_value / read_from_buffer) -----------------
    def read_value(self, index, buffer=BUF_CURRENT):
        v = C.c_double()
        _check(self.lib.wv_read_value(self.h, buffer, index, C.byref(v)))
        return v.value

    def write_value(self, index, value, buffer=BUF_CURRENT):
        _check(self.lib.wv_write_value(self.h, buffer, index, float(value)))

    def read_field(self, buffer=BUF_CURRENT, dtype=None):
        dtype = np.dtype(dtype or self.dtype)
        out = np.empty(self.mesh.num_nodes, dtype=dtype)
        _check(self.lib.wv_read_field(self.h, buffer, out.ctypes.data_as(C.c_void_p), dtype.itemsize))
        return out

    def write_field(self, values, buffer=BUF_CURRENT):
        values = np.ascontiguousarray(values)
        assert values.shape == (self.mesh.num_nodes,) and values.dtype in (np.float32, np.float64)
        _check(self.lib.wv_write_field(self.h, buffer, values.ctypes.data_as(C.c_void_p), values.dtype.itemsize))

    def read_planes(self, z_begin, z_count, buffer=BUF_CURRENT, dtype=None):
        """Planes [z_begin, z_begin + z_count) of a field as [z_count, ny, nx]."""
        dtype = np.dtype(dtype or self.dtype)
        nx, ny, _ = self.mesh.dims
        out = np.empty((z_count, ny, nx), dtype=dtype)
        _check(self.lib.wv_read_planes(self.h, buffer, z_begin, z_count, out.ctypes.data_as(C.c_void_p), dtype.itemsize))
        return out

    def write_planes(self, z_begin, values, buffer=BUF_CURRENT):
        values = np.ascontiguousarray(values)
        nx, ny, _ = self.mesh.dims
        assert values.shape[1:] == (ny, nx) and values.dtype in (np.float32, np.float64)
        _check(self.lib.wv_write_planes(self.h, buffer, z_begin, values.shape[0], values.ctypes.data_as(C.c_void_p),
                                        values.dtype.itemsize))

    def read_boundary_data(self, d):
        out = np.zeros((self.mesh.bidx[d - 1].shape[0], d), dtype=M.boundary_data_dtype)
        if out.size:
            _check(self.lib.wv_read_boundary_data(self.h, d, out.ctypes.data_as(C.c_void_p)))
        return out

    def write_boundary_data(self, d, data):
        data = np.ascontiguousarray(data, dtype=M.boundary_data_dtype)
        if data.size:
            _check(self.lib.wv_write_boundary_data(self.h, d, data.ctypes.data_as(C.c_void_p)))

    def set_coefficients(self, coeffs):
        coeffs = np.ascontiguousarray(coeffs, dtype=M.coefficients_dtype)
        _check(self.lib.wv_set_coefficients(self.h, coeffs.ctypes.data_as(C.c_void_p), coeffs.shape[0]))

    def device_buffer(self, buffer=BUF_CURRENT):
        p = C.c_void_p()
        _check(self.lib.wv_device_buffer(self.h, buffer, C.byref(p)))
        return p.value

    # ---- stepping ---------------------------------------------------------------------------
    def checkpoint(self):
        """wv_checkpoint: the fields, filter memories and the position in the run copied aside on the device."""
        _check(self.lib.wv_checkpoint(self.h))

    def rollback(self):
        """wv_rollback: back to the last checkpoint (the engine then reproduces the abandoned steps bit for bit)."""
        _check(self.lib.wv_rollback(self.h))

    def drop_checkpoint(self):
        _check(self.lib.wv_drop_checkpoint(self.h))

    def step(self):
        flag = C.c_int32()
        _check(self.lib.wv_step(self.h, C.byref(flag)))
        return flag.value

    def swap(self):
        _check(self.lib.wv_swap(self.h))

    def set_source(self, kind, node=0, signal=None):
        if kind == SOURCE_NONE:
            _check(self.lib.wv_set_source(self.h, kind, 0, None, 0))
            return
        sig = np.ascontiguousarray(signal, dtype=np.float64)
        _check(self.lib.wv_set_source(self.h, kind, int(node), sig.ctypes.data_as(C.c_void_p), sig.shape[0]))

    def set_receivers(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        _check(self.lib.wv_set_receivers(self.h, nodes.ctypes.data_as(C.c_void_p) if nodes.shape[0] else None,
                                         nodes.shape[0]))
        self.n_recv = nodes.shape[0]
        self.n_directional = 0

    def set_directional_receivers(self, nodes, spacing, sample_rate, ambient_density):
        """wv_set_directional_receivers: `nodes` are the centre nodes of R directional receivers, recorded and integrated on the
        device; fetch_directional has their records.  An empty list leaves the mode (as set_receivers does)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        _check(self.lib.wv_set_directional_receivers(self.h, nodes.ctypes.data_as(C.c_void_p) if nodes.shape[0] else None,
                                                     nodes.shape[0], float(spacing), float(sample_rate), float(ambient_density)))
        self.n_directional = nodes.shape[0]
        self.n_recv = 7 * nodes.shape[0]

    def fetch_directional(self, first, n):
        """wv_fetch_directional: records of steps [first, first + n) as postprocess.directional_output_dtype[n, R]."""
        out = np.zeros((n, self.n_directional), dtype=DIRECTIONAL_OUTPUT_DTYPE)
        _check(self.lib.wv_fetch_directional(self.h, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out

    def run_steps(self, n_steps):
        """wv_run: returns (steps_done, flag)."""
        done = C.c_uint64()
        flag = C.c_int32()
        _check(self.lib.wv_run(self.h, int(n_steps), C.byref(done), C.byref(flag)))
        return done.value, flag.value

    def fetch_receivers(self, first, n):
        out = np.zeros((n, self.n_recv), dtype=np.float64)
        if out.size:
            _check(self.lib.wv_fetch_receivers(self.h, first, n, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- field snapshots taken on the device while wv_run goes on ---------------------------------
    def set_snapshots(self, box="mesh", stride=1, first_step=0, period=1, keep=0):
        """wv_set_snapshots.  `box` = ((x0, y0, z0), (ex, ey, ez)): first node and extent in NODES OF THE MESH ("mesh": the whole mesh;
        an extent of None: up to the mesh's far face); `stride` = s or (sx, sy, sz): every s-th node of the box is taken, the first
        included, so an axis yields ceil(extent / s) nodes.  Snapshots at steps first_step + j * period; the host holds the last
        `keep` (0: all).  A snapshot of step s is the field after s completed steps -- what read_planes returns at step_count() == s;
        the source's sample of step s is not in it yet (the loop puts it into its node after the snapshot is taken, before the
        update).  set_snapshots(None) stops recording and forgets what is held.  Returns the shape
        (nz, ny, nx) of one snapshot."""
        if box is None:
            return self._stop_plan("snapshot", self.lib.wv_set_snapshots, None)
        plan = WvSnapshotPlan()
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.keep = int(keep)
        _check(self.lib.wv_set_snapshots(self.h, C.byref(plan)))
        self.snapshot_shape = (taken[2], taken[1], taken[0])
        return self.snapshot_shape

    def _fill_box(self, plan, box, stride, first_step, period):
        """(origin, extent, stride) -> the plan's first node, nodes taken and strides, and its cadence; returns the nodes taken (x, y, z)."""
        dims = self.mesh.dims
        origin, extent = ((0, 0, 0), None) if isinstance(box, str) and box == "mesh" else box
        extent = tuple(extent) if extent is not None else (None, None, None)
        stride = (stride,) * 3 if np.isscalar(stride) else tuple(stride)
        taken = []
        for axis in range(3):
            ext = dims[axis] - origin[axis] if extent[axis] is None else extent[axis]
            s = int(stride[axis])
            taken.append((int(ext) + s - 1) // s if s >= 1 and ext >= 1 else 0)   # (a bad stride or extent is the library's to refuse)
        plan.x0, plan.y0, plan.z0 = (int(v) for v in origin)
        plan.nx, plan.ny, plan.nz = taken
        plan.sx, plan.sy, plan.sz = (int(v) for v in stride)
        plan.first_step, plan.period = int(first_step), int(period)
        return taken

    def _stop_plan(self, name, setter, *nulls):
        """A setter given None: the plan stops and its state is forgotten, here and in the library."""
        _check(setter(self.h, *nulls))
        setattr(self, name + "_shape", None)

    def _count(self, fn):
        """A wv_*_count call: its two uint64 results."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(fn(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _interior_box(self):
        """The mesh without its faces: every node of it has its six neighbours on the grid."""
        return ((1, 1, 1), tuple(d - 2 for d in self.mesh.dims))

    @staticmethod
    def _fill_edges(plan, edges, most, who, count="n_bins", what="bins"):
        """The bin edges counted from a node's own onset -> the plan's edges and their number, which it calls `count`; returns the number."""
        edges = [int(v) for v in edges]
        if len(edges) > most:
            raise ValueError("%s: %d %s at the most" % (who, most, what))
        setattr(plan, count, len(edges))
        for k, v in enumerate(edges):
            plan.edges[k] = v
        return len(edges)

    @staticmethod
    def _sections(bands, who):
        """A filter bank as the library takes it: float64[K][S][5], contiguous."""
        sections = np.ascontiguousarray(bands, dtype=np.float64)
        if sections.ndim != 3 or sections.shape[2] != 5:
            raise ValueError("%s: bands is float64[K][S][5], got shape %r" % (who, sections.shape))
        return sections

    def _fetch(self, fn, *arrays):
        """A wv_fetch_* call that fills `arrays` and ends in a word for the captures in them, which is returned."""
        captures = C.c_uint64()
        _check(fn(self.h, *[a.ctypes.data_as(C.c_void_p) for a in arrays], C.byref(captures)))
        return captures.value

    @staticmethod
    def _fill_constants(plan, spacing, sample_rate, ambient_density):
        plan.spacing, plan.sample_rate, plan.ambient_density = float(spacing), float(sample_rate), float(ambient_density)

    @staticmethod
    def _threshold_map(threshold_map, taken, who):
        """A per-node threshold map as the library takes it: (the float32 array, which has to outlive the call; its pointer) or (None, None)."""
        if threshold_map is None:
            return None, None
        threshold_map = np.ascontiguousarray(threshold_map, dtype=np.float32)
        if threshold_map.shape != (taken[2], taken[1], taken[0]):
            raise ValueError("%s: the threshold map must have the box's shape %r" % (who, (taken[2], taken[1], taken[0])))
        return threshold_map, threshold_map.ctypes.data_as(C.c_void_p)

    def snapshot_count(self):
        """wv_snapshot_count: (snapshots taken since the plan was set, index of the oldest one still held)."""
        return self._count(self.lib.wv_snapshot_count)

    def fetch_snapshots(self, first=None, n=None):
        """wv_fetch_snapshots: snapshots [first, first + n) as (float32[n, nz, ny, nx], steps uint64[n]); by default all that are held."""
        if first is None or n is None:
            taken, first_held = self.snapshot_count()
            first = first_held if first is None else first
            n = taken - first if n is None else n
        out = np.empty((n,) + tuple(self.snapshot_shape or (0, 0, 0)), dtype=np.float32)   # (no plan: the library says so)
        steps = np.empty(n, dtype=np.uint64)
        _check(self.lib.wv_fetch_snapshots(self.h, int(first), int(n), out.ctypes.data_as(C.c_void_p), steps.ctypes.data_as(C.c_void_p)))
        return out, steps

    # ---- field spectra accumulated on the device while wv_run goes on -------------------------------
    def set_spectrum(self, freqs, box="mesh", stride=1, first_step=0, period=1):
        """wv_set_spectrum.  `freqs`: K frequencies in CYCLES PER STEP, 0 .. 0.5 (K <= 64); `box`, `stride`, `first_step`, `period` as
        for set_snapshots.  At every plan step the engine captures the box as a snapshot would and adds it, on the device, to a running
        Fourier sum per node and frequency: X_k = sum_j p_j exp(-2 pi i f_k n_j) over the captures j of steps n_j, in capture order, with
        the twiddles spectrum_twiddle gives -- a NumPy loop over the snapshots of the same plan reproduces it bit for bit.  No window.
        Excludes a snapshot plan.  set_spectrum(None) stops and forgets.  Returns the shape (K, nz, ny, nx)."""
        if freqs is None:
            return self._stop_plan("spectrum", self.lib.wv_set_spectrum, None, None)
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        plan = WvSpectrumPlan()
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.n_freqs = f.shape[0]
        _check(self.lib.wv_set_spectrum(self.h, C.byref(plan), f.ctypes.data_as(C.c_void_p)))
        self.spectrum_shape = (f.shape[0], taken[2], taken[1], taken[0])
        return self.spectrum_shape

    def spectrum_count(self):
        """wv_spectrum_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_spectrum_count)

    def fetch_spectrum(self):
        """wv_fetch_spectrum: (complex128[K, nz, ny, nx], captures in it).  The plan keeps running."""
        out = np.zeros(tuple(self.spectrum_shape or (0, 0, 0, 0)), dtype=np.complex128)   # (no plan: the library says so)
        return out, self._fetch(self.lib.wv_fetch_spectrum, out)

    # ---- time-binned field energy accumulated on the device while wv_run goes on ----------------------
    def set_decay(self, n_bins, bin_captures=1, box="mesh", stride=1, first_step=0, period=1, bands=None):
        """wv_set_decay.  `box`, `stride`, `first_step`, `period` as for set_snapshots.  At every plan step the engine captures the box
        as a snapshot would and adds its square, on the device, to the time bin of the capture: capture j (0, 1, ... since the plan was
        set) goes to bin min(j // bin_captures, n_bins - 1), E[b] = E[b] + p * p in double, in capture order -- a NumPy loop over the
        snapshots of the same plan reproduces the bins bit for bit.  The last bin is open-ended.  wayverb_amd.decay turns the bins into
        the decay curve, EDT / T20 / T30 and level maps.  Excludes a snapshot plan and a spectrum plan.  set_decay(None) stops and
        forgets.  Returns the shape (n_bins, nz, ny, nx).

        `bands`: float64[K][S][5], K <= 8 cascades of S <= 4 biquad sections (b0, b1, b2, a1, a2; wayverb_amd.decay designs them) ->
        wv_set_decay_bands: every node runs its captures through each cascade, in double, before the square, and each band has bins of
        its own (decay.banded_bins is the same in NumPy, bit for bit).  The series the filters see is sampled every `period` steps:
        design the sections for sample_rate / period.  Returns the shape (K, n_bins, nz, ny, nx).  None: the plain plan."""
        if n_bins is None:
            self._stop_plan("decay", self.lib.wv_set_decay, None)   # (stops either kind of plan)
            self.decay_banded = False
            return None
        sections = self._sections(bands, "set_decay") if bands is not None else None
        plan = WvDecayPlan()
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.n_bins, plan.bin_captures = int(n_bins), int(bin_captures)
        if sections is not None:
            _check(self.lib.wv_set_decay_bands(self.h, C.byref(plan), sections.ctypes.data_as(C.c_void_p), sections.shape[0], sections.shape[1]))
        else:
            _check(self.lib.wv_set_decay(self.h, C.byref(plan)))
        self.decay_shape = (() if sections is None else sections.shape[:1]) + (int(n_bins), taken[2], taken[1], taken[0])
        self.decay_banded = sections is not None
        return self.decay_shape

    def decay_count(self):
        """wv_decay_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_decay_count)

    def fetch_decay(self, banded=None):
        """wv_fetch_decay: (float64[n_bins, nz, ny, nx], captures in it); under a banded plan wv_fetch_decay_bands:
        (float64[K, n_bins, nz, ny, nx], captures).  The plan keeps running.  `banded` = True / False asks for that call whatever the
        plan (the library refuses the wrong one)."""
        out = np.zeros(tuple(self.decay_shape or (0, 0, 0, 0)), dtype=np.float64)   # (no plan: the library says so)
        banded = self.decay_banded if banded is None else banded
        return out, self._fetch(self.lib.wv_fetch_decay_bands if banded else self.lib.wv_fetch_decay, out)

    # ---- time-binned sound intensity accumulated on the device while wv_run goes on ------------------
    def set_intensity(self, n_bins, bin_captures=1, box=None, stride=1, first_step=0, period=1, spacing=None, sample_rate=None,
                      ambient_density=None):
        """wv_set_intensity.  `box`, `stride`, `first_step`, `period` as for set_snapshots (None: the mesh's interior -- every taken
        node needs its six neighbours on the grid).  At every plan step the engine runs the reference's directional_receiver
        integrator at every node taken -- velocity from the pressure differences to the six neighbours, with `spacing`,
        `sample_rate` (of the CAPTURED series: the mesh's rate / period) and `ambient_density` -- and adds v * p per axis and p * p
        to the time bin of the capture, in double, in capture order; intensity.intensity_bins over snapshots of the box's hull
        reproduces bins and velocities bit for bit.  Excludes every other plan.  set_intensity(None) stops and forgets.  Returns the
        shape (4, n_bins, nz, ny, nx): Ix, Iy, Iz, E."""
        if n_bins is None:
            return self._stop_plan("intensity", self.lib.wv_set_intensity, None)
        if box is None:
            box = self._interior_box()
        plan = WvIntensityPlan()
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.n_bins, plan.bin_captures = int(n_bins), int(bin_captures)
        self._fill_constants(plan, spacing, sample_rate, ambient_density)
        _check(self.lib.wv_set_intensity(self.h, C.byref(plan)))
        self.intensity_shape = (4, int(n_bins), taken[2], taken[1], taken[0])
        return self.intensity_shape

    def intensity_count(self):
        """wv_intensity_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_intensity_count)

    def fetch_intensity(self):
        """wv_fetch_intensity: (float64[4, n_bins, nz, ny, nx] = Ix, Iy, Iz, E, captures in it).  The plan keeps running."""
        out = np.zeros(tuple(self.intensity_shape or (0, 0, 0, 0, 0)), dtype=np.float64)   # (no plan: the library says so)
        return out, self._fetch(self.lib.wv_fetch_intensity, out)

    def fetch_intensity_velocity(self):
        """wv_fetch_intensity_velocity: float64[3, nz, ny, nx], the velocities the integrator carries, after the captures folded so far."""
        shape = self.intensity_shape
        out = np.zeros((3,) + tuple(shape[2:]) if shape else (0, 0, 0, 0), dtype=np.float64)
        _check(self.lib.wv_fetch_intensity_velocity(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def fetch_directional_velocity(self, n):
        """wv_fetch_directional_velocity: float64[n, 3], the carried velocities of the n directional receivers."""
        out = np.zeros((int(n), 3), dtype=np.float64)
        _check(self.lib.wv_fetch_directional_velocity(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- arrival-aligned energy maps accumulated on the device while wv_run goes on ------------------
    def set_arrival(self, edges, threshold=0.0, box="mesh", stride=1, first_step=0, period=1, threshold_map=None):
        """wv_set_arrival.  `box`, `stride`, `first_step`, `period` as for set_snapshots.  `edges`: 1 .. 16 integers, edges[0] == 0,
        strictly increasing: the first capture of bin k counted from the node's OWN onset, the first capture at which |p| >=
        `threshold` (or the node's entry of `threshold_map`, float32 [nz, ny, nx]).  Per node the engine keeps onset, peak,
        peak_capture, the energy ahead of the onset, the bins and the first time moment; arrival.arrival_fold over the snapshots
        reproduces all of it bit for bit.  Excludes every other plan.  set_arrival(None) stops and forgets.  Returns the shape of the
        bins, (n_bins, nz, ny, nx)."""
        if edges is None:
            return self._stop_plan("arrival", self.lib.wv_set_arrival, None, None)
        plan = WvArrivalPlan()
        n_bins = self._fill_edges(plan, edges, 16, "set_arrival")
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.threshold = float(threshold)
        threshold_map, map_pointer = self._threshold_map(threshold_map, taken, "set_arrival")
        _check(self.lib.wv_set_arrival(self.h, C.byref(plan), map_pointer))
        self.arrival_shape = (n_bins, taken[2], taken[1], taken[0])
        return self.arrival_shape

    def arrival_count(self):
        """wv_arrival_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_arrival_count)

    def fetch_arrival(self):
        """wv_fetch_arrival: (dict(onset=uint32[nz, ny, nx], peak=float32, peak_capture=uint32, pre=float64, moment=float64,
        bins=float64[n_bins, nz, ny, nx]), captures in them).  ARRIVAL_NONE marks a node without an onset.  The plan keeps running."""
        shape = tuple(self.arrival_shape or (0, 0, 0, 0))   # (no plan: the library says so)
        out = dict(onset=np.zeros(shape[1:], np.uint32), peak=np.zeros(shape[1:], np.float32), peak_capture=np.zeros(shape[1:], np.uint32),
                   pre=np.zeros(shape[1:], np.float64), moment=np.zeros(shape[1:], np.float64), bins=np.zeros(shape, np.float64))
        return out, self._fetch(self.lib.wv_fetch_arrival, *out.values())   # (in the order the library takes them)

    # ---- lateral maps accumulated on the device while wv_run goes on ---------------------------------
    def set_lateral(self, edges, threshold=0.0, box=None, stride=1, first_step=0, period=1, threshold_map=None, spacing=None,
                    sample_rate=None, ambient_density=None):
        """wv_set_lateral.  `box`, `stride`, `first_step`, `period`, `spacing`, `sample_rate` (of the CAPTURED series) and
        `ambient_density` as for set_intensity (box None: the mesh's interior -- every taken node needs its six neighbours on the
        grid); `edges` (8 at the most), `threshold` and `threshold_map` as for set_arrival.  Per node the engine runs the reference's
        directional_receiver integrator and keeps the onset, the energy ahead of it, the velocities and, in bins counted from the
        node's OWN onset, p^2, p v and the six distinct entries of v v^T; lateral.lateral_fold over snapshots of the box's hull
        reproduces all of it bit for bit.  Excludes every other plan.  set_lateral(None) stops and forgets.  Returns the shape of the
        bins, (10, n_bins, nz, ny, nx): E, Ix, Iy, Iz, Qxx, Qyy, Qzz, Qxy, Qxz, Qyz."""
        if edges is None:
            return self._stop_plan("lateral", self.lib.wv_set_lateral, None, None)
        plan = WvLateralPlan()
        n_bins = self._fill_edges(plan, edges, 8, "set_lateral")
        taken = self._fill_box(plan, self._interior_box() if box is None else box, stride, first_step, period)
        plan.threshold = float(threshold)
        self._fill_constants(plan, spacing, sample_rate, ambient_density)
        threshold_map, map_pointer = self._threshold_map(threshold_map, taken, "set_lateral")
        _check(self.lib.wv_set_lateral(self.h, C.byref(plan), map_pointer))
        self.lateral_shape = (10, n_bins, taken[2], taken[1], taken[0])
        return self.lateral_shape

    def lateral_count(self):
        """wv_lateral_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_lateral_count)

    def fetch_lateral(self):
        """wv_fetch_lateral: (dict(onset=uint32[nz, ny, nx], pre=float64[nz, ny, nx], velocity=float64[3, nz, ny, nx],
        bins=float64[10, n_bins, nz, ny, nx]), captures in them).  ARRIVAL_NONE marks a node without an onset.  The plan keeps running."""
        shape = tuple(self.lateral_shape or (0, 0, 0, 0, 0))   # (no plan: the library says so)
        out = dict(onset=np.zeros(shape[2:], np.uint32), pre=np.zeros(shape[2:], np.float64), velocity=np.zeros((3,) + shape[2:], np.float64),
                   bins=np.zeros(shape, np.float64))
        return out, self._fetch(self.lib.wv_fetch_lateral, *out.values())   # (in the order the library takes them)

    # ---- modulation maps accumulated on the device while wv_run goes on ------------------------------
    def set_modulation(self, freqs, bands, box="mesh", stride=1, first_step=0, period=1):
        """wv_set_modulation.  `freqs`: M <= 16 modulation frequencies in CYCLES PER STEP, 0 .. 0.5 (modulation.cycles_per_step turns
        hertz into them); `bands`: float64[K][S][5], K <= 8 cascades of S <= 4 biquad sections (wayverb_amd.decay designs them, for the
        rate of the CAPTURED series: the mesh's rate / period); `box`, `stride`, `first_step`, `period` as for set_snapshots.  At every
        plan step the engine captures the box as a snapshot would, runs every node's capture through each cascade, squares it and adds
        the square to the band's energy and, times the twiddles spectrum_twiddle gives, to a running Fourier sum per modulation
        frequency -- modulation.modulation_fold over the snapshots of the same plan reproduces all of it bit for bit.  Excludes every
        other plan.  set_modulation(None, None) stops and forgets.  Returns the shape (K, M, nz, ny, nx)."""
        if freqs is None:
            return self._stop_plan("modulation", self.lib.wv_set_modulation, None, None, None, 0, 0)
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        sections = self._sections(bands, "set_modulation")
        plan = WvModulationPlan()
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.n_freqs = f.shape[0]
        _check(self.lib.wv_set_modulation(self.h, C.byref(plan), f.ctypes.data_as(C.c_void_p), sections.ctypes.data_as(C.c_void_p), sections.shape[0],
                                          sections.shape[1]))
        self.modulation_shape = (sections.shape[0], f.shape[0], taken[2], taken[1], taken[0])
        return self.modulation_shape

    def modulation_count(self):
        """wv_modulation_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_modulation_count)

    def fetch_modulation(self):
        """wv_fetch_modulation: (energy float64[K, nz, ny, nx], sums complex128[K, M, nz, ny, nx]).  They hold every capture
        modulation_count counts.  The plan keeps running."""
        shape = tuple(self.modulation_shape or (0, 0, 0, 0, 0))   # (no plan: the library says so)
        energy = np.zeros(shape[:1] + shape[2:], dtype=np.float64)
        sums = np.zeros(shape, dtype=np.complex128)
        _check(self.lib.wv_fetch_modulation(self.h, energy.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p), None))
        return energy, sums

    # ---- band-limited arrival maps accumulated on the device while wv_run goes on --------------------
    def set_arrival_bands(self, edges, bands, threshold=0.0, tail=None, lag=0, box="mesh", stride=1, first_step=0, period=1, threshold_map=None,
                          reserved=0):
        """wv_set_arrival_bands: set_arrival with set_decay's filter bank ahead of the square.  `edges`, `threshold`, `threshold_map`,
        `box`, `stride`, `first_step`, `period` as for set_arrival; `bands`: float64[K][S][5] as for set_decay (designed for the rate of
        the CAPTURED series); `tail`: None or (n_tail, tail_first, tail_captures) -- n_tail uniform bins of tail_captures captures
        behind the explicit ones, the first at tail_first captures behind the onset, the last open-ended; `lag`: captures by which
        each band's clock starts late, one integer for all bands or K of them; `reserved` is the plan's reserved word, 0.  Per node the engine keeps the broadband onset, peak and
        peak_capture, and per band the energy ahead of the onset, the bins and the first time moment; arrival.banded_arrival_fold over
        the snapshots reproduces all of it bit for bit.  Excludes every other plan.  set_arrival_bands(None, None) stops and forgets.
        Returns the shape of the bins, (K, n_edges + n_tail, nz, ny, nx)."""
        if edges is None:
            return self._stop_plan("arrival_bands", self.lib.wv_set_arrival_bands, None, None, None, 0, 0)
        sections = self._sections(bands, "set_arrival_bands")
        plan = WvArrivalBandsPlan()
        self._fill_edges(plan, edges, 16, "set_arrival_bands", count="n_edges", what="explicit bins")
        if tail is not None:
            plan.n_tail, plan.tail_first, plan.tail_captures = (int(v) for v in tail)
        lags = [int(lag)] * min(sections.shape[0], 8) if np.isscalar(lag) else [int(v) for v in lag]
        if len(lags) > 8 or (not np.isscalar(lag) and len(lags) != sections.shape[0]):
            raise ValueError("set_arrival_bands: one lag, or one per band")
        for k, v in enumerate(lags):
            plan.lag[k] = v
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.threshold, plan.reserved = float(threshold), int(reserved)
        threshold_map, map_pointer = self._threshold_map(threshold_map, taken, "set_arrival_bands")
        _check(self.lib.wv_set_arrival_bands(self.h, C.byref(plan), map_pointer, sections.ctypes.data_as(C.c_void_p), sections.shape[0], sections.shape[1]))
        self.arrival_bands_shape = (sections.shape[0], plan.n_edges + plan.n_tail, taken[2], taken[1], taken[0])
        return self.arrival_bands_shape

    def arrival_bands_count(self):
        """wv_arrival_bands_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_arrival_bands_count)

    def fetch_arrival_bands(self):
        """wv_fetch_arrival_bands: (dict(onset=uint32[nz, ny, nx], peak=float32, peak_capture=uint32, pre=float64[K, nz, ny, nx],
        moment=float64[K, nz, ny, nx], bins=float64[K, n_bins, nz, ny, nx]), captures in them).  ARRIVAL_NONE marks a node without an
        onset.  The plan keeps running."""
        shape = tuple(self.arrival_bands_shape or (0, 0, 0, 0, 0))   # (no plan: the library says so)
        node, band = shape[2:], shape[:1] + shape[2:]
        out = dict(onset=np.zeros(node, np.uint32), peak=np.zeros(node, np.float32), peak_capture=np.zeros(node, np.uint32),
                   pre=np.zeros(band, np.float64), moment=np.zeros(band, np.float64), bins=np.zeros(shape, np.float64))
        return out, self._fetch(self.lib.wv_fetch_arrival_bands, *out.values())   # (in the order the library takes them)

    # ---- time-binned field spectra accumulated on the device while wv_run goes on ---------------------
    # (None until a plan is set.  A default of the class, not one of _plan_state's attributes: tests/golden/python_front.json holds
    # the attributes of a fresh engine name by name, and was recorded before this plan)
    waterfall_shape = None

    def set_waterfall(self, freqs, n_bins, bin_captures, box="mesh", stride=1, first_step=0, period=1):
        """wv_set_waterfall.  `freqs`: K frequencies in CYCLES PER STEP, 0 .. 0.5 (K <= 64); `n_bins` time bins of `bin_captures` captures
        each, the last open-ended (K * n_bins <= 4096); `box`, `stride`, `first_step`, `period` as for set_snapshots.  At every plan step
        the engine captures the box as a snapshot would and adds it, on the device, to the Fourier sum of the capture's time bin per node
        and frequency: capture j (0, 1, ... since the plan was set) of step n_j goes to bin min(j // bin_captures, n_bins - 1),
        X[b][k] = X[b][k] + p_j exp(-2 pi i f_k n_j) with the twiddles spectrum_twiddle gives at the ABSOLUTE step -- a NumPy loop over
        the snapshots of the same plan reproduces it bit for bit (wayverb_amd.waterfall.waterfall_fold).  |X[b][k]|^2 is the short-time
        spectrum, the backward cumulative sums over b the cumulative spectral decay (wayverb_amd.waterfall).  No window.  Excludes
        every other plan.  set_waterfall(None, None, None) stops and forgets.  Returns the shape (n_bins, K, nz, ny, nx)."""
        if freqs is None:
            return self._stop_plan("waterfall", self.lib.wv_set_waterfall, None, None)
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        plan = WvWaterfallPlan()
        taken = self._fill_box(plan, box, stride, first_step, period)
        plan.n_freqs, plan.n_bins, plan.bin_captures = f.shape[0], int(n_bins), int(bin_captures)
        _check(self.lib.wv_set_waterfall(self.h, C.byref(plan), f.ctypes.data_as(C.c_void_p)))
        self.waterfall_shape = (int(n_bins), f.shape[0], taken[2], taken[1], taken[0])
        return self.waterfall_shape

    def waterfall_count(self):
        """wv_waterfall_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_waterfall_count)

    def fetch_waterfall(self):
        """wv_fetch_waterfall: (complex128[n_bins, K, nz, ny, nx], captures in it).  The plan keeps running."""
        out = np.zeros(tuple(self.waterfall_shape or (0, 0, 0, 0, 0)), dtype=np.complex128)   # (no plan: the library says so)
        return out, self._fetch(self.lib.wv_fetch_waterfall, out)

    # ---- interaural maps accumulated on the device while wv_run goes on -------------------------------
    # (a default of the class, as waterfall_shape is and for its reason)
    interaural_shape = None

    def set_interaural(self, edges, ear_a=(0, 0, 0), ear_b=(0, 0, 0), max_lag=0, threshold=0.0, sections=None, box="mesh", stride=1, first_step=0,
                       period=1, threshold_map=None):
        """wv_set_interaural.  `ear_a`, `ear_b`: offsets in MESH NODES (not box strides) from a taken node to its two ears, every
        component -8 .. 8, both on the mesh for every node taken (interaural.ear_offsets makes them of an axis and a distance in
        metres); equal ears give the autocorrelation form.  `max_lag`: L, 0 .. 16 captures (interaural.max_lag makes it of
        milliseconds).  `edges` (4 at the most), `threshold`, `threshold_map`, `box`, `stride`, `first_step`, `period` as for
        set_arrival.  `sections`: None, or float64[S][5], S <= 4 biquad sections of the ONE band-pass cascade both ears run through
        (decay.butterworth_bandpass designs them, for the rate of the CAPTURED series).  Per node the engine keeps the onset (of the
        louder ear, unfiltered), the two energies ahead of it and, in bins counted from the node's OWN onset, Ea, Eb and the lagged
        products C[-L] .. C[+L] (tau = +l: ear a earlier, ear b later by l captures; a product goes to the bin of the LATER sample);
        interaural.interaural_fold over snapshots of the two ear planes reproduces all of it bit for bit, and interaural.iacf / iacc /
        iacc_lag turn the bins into ISO 3382-1 Annex B's figures in their head-less (spaced omni) form -- not a dummy head.  Excludes
        every other plan.  set_interaural(None) stops and forgets.  Returns the shape of the bins, (n_bins, 2 L + 3, nz, ny, nx): Ea, Eb,
        C[-L] .. C[+L]."""
        if edges is None:
            return self._stop_plan("interaural", self.lib.wv_set_interaural, None, None, None)
        plan = WvInterauralPlan()
        n_bins = self._fill_edges(plan, edges, 4, "set_interaural")
        taken = self._fill_box(plan, box, stride, first_step, period)
        for axis in range(3):
            plan.ear_a[axis], plan.ear_b[axis] = int(ear_a[axis]), int(ear_b[axis])
        plan.max_lag, plan.threshold = int(max_lag), float(threshold)
        coefficients, pointer = None, None
        if sections is not None:
            coefficients = np.ascontiguousarray(sections, dtype=np.float64)
            if coefficients.ndim != 2 or coefficients.shape[1] != 5:
                raise ValueError("set_interaural: sections is float64[S][5], got shape %r" % (coefficients.shape,))
            plan.n_sections, pointer = coefficients.shape[0], coefficients.ctypes.data_as(C.c_void_p)
        threshold_map, map_pointer = self._threshold_map(threshold_map, taken, "set_interaural")
        _check(self.lib.wv_set_interaural(self.h, C.byref(plan), pointer, map_pointer))
        self.interaural_shape = (n_bins, 2 * int(max_lag) + 3, taken[2], taken[1], taken[0])
        return self.interaural_shape

    def interaural_count(self):
        """wv_interaural_count: (captures of completed steps since the plan was set, the step of the last of them)."""
        return self._count(self.lib.wv_interaural_count)

    def fetch_interaural(self):
        """wv_fetch_interaural: (dict(onset=uint32[nz, ny, nx], pre=float64[2, nz, ny, nx], bins=float64[n_bins, 2 L + 3, nz, ny, nx]),
        captures in them).  ARRIVAL_NONE marks a node without an onset.  The plan keeps running."""
        shape = tuple(self.interaural_shape or (0, 0, 0, 0, 0))   # (no plan: the library says so)
        out = dict(onset=np.zeros(shape[2:], np.uint32), pre=np.zeros((2,) + shape[2:], np.float64), bins=np.zeros(shape, np.float64))
        return out, self._fetch(self.lib.wv_fetch_interaural, *out.values())   # (in the order the library takes them)

    def step_count(self):
        s = C.c_uint64()
        _check(self.lib.wv_step_count(self.h, C.byref(s)))
        return s.value

    def enable_kernel_timing(self, on=True):
        _check(self.lib.wv_enable_kernel_timing(self.h, int(on)))

    def kernel_time_ms(self):
        ms = C.c_double()
        n = C.c_uint64()
        _check(self.lib.wv_kernel_time_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_time_detail(self):
        """(mean ms per launch of the dominant kernel, launches, time steps those launches covered)"""
        ms = C.c_double()
        n = C.c_uint64()
        steps = C.c_uint64()
        _check(self.lib.wv_kernel_time_detail(self.h, C.byref(ms), C.byref(n), C.byref(steps)))
        return ms.value, n.value, steps.value

    QUERY_PASSES, QUERY_XWALL_ENTRIES, QUERY_FIELDS, QUERY_MARCH_LIVE_PERMILLE, QUERY_SWEEP_LIVE_PERMILLE, QUERY_MARCH_ROUNDS = 0, 1, 2, 3, 4, 5
    QUERY_HALO_WAIT_NS, QUERY_HALO_WAITS, QUERY_HALO_EXCHANGES, QUERY_HALO_BYTES_SENT, QUERY_EARLY_PASSES = 6, 7, 8, 9, 10
    QUERY_BOUNDARY1_NS, QUERY_BOUNDARY2_NS, QUERY_BOUNDARY_TIMED = 11, 12, 13
    QUERY_WHOLE_STEPS = 14
    QUERY_TRIPLE_PASSES = 15
    QUERY_TRIPLE_MARCH_NS, QUERY_TRIPLE_MARCH_TIMED, QUERY_BOUNDARY3_NS, QUERY_FIXUP3_NS, QUERY_TRIPLE_PARTS_TIMED = 16, 17, 18, 19, 20
    QUERY_SNAPSHOT_NS, QUERY_SNAPSHOT_BYTES, QUERY_SNAPSHOTS_TAKEN = 21, 22, 23
    QUERY_WIDE_GATHERS, QUERY_DIRECTIONAL_LAUNCHES = 24, 25
    QUERY_SPECTRUM_CAPTURES, QUERY_SPECTRUM_FOLDS, QUERY_SPECTRUM_NS = 26, 27, 28
    QUERY_DECAY_CAPTURES, QUERY_DECAY_FOLDS, QUERY_DECAY_NS = 29, 30, 31
    QUERY_INTENSITY_CAPTURES, QUERY_INTENSITY_FOLDS, QUERY_INTENSITY_NS, QUERY_INTENSITY_GATHER_NS, QUERY_INTENSITY_GATHERS = 32, 33, 34, 35, 36
    QUERY_ARRIVAL_CAPTURES, QUERY_ARRIVAL_FOLDS, QUERY_ARRIVAL_NS = 37, 38, 39
    QUERY_LATERAL_CAPTURES, QUERY_LATERAL_FOLDS, QUERY_LATERAL_NS, QUERY_LATERAL_GATHER_NS, QUERY_LATERAL_GATHERS = 40, 41, 42, 43, 44
    QUERY_MODULATION_CAPTURES, QUERY_MODULATION_FOLDS, QUERY_MODULATION_NS = 45, 46, 47
    QUERY_ARRIVAL_BANDS_CAPTURES, QUERY_ARRIVAL_BANDS_FOLDS, QUERY_ARRIVAL_BANDS_NS = 48, 49, 50
    QUERY_WATERFALL_CAPTURES, QUERY_WATERFALL_FOLDS, QUERY_WATERFALL_NS = 51, 52, 53
    QUERY_INTERAURAL_CAPTURES, QUERY_INTERAURAL_FOLDS, QUERY_INTERAURAL_NS = 54, 55, 56

    def query(self, what):
        """wv_query: two-step passes taken / wall nodes on compact copies / fields allocated."""
        self.lib.wv_query.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        v = C.c_uint64()
        _check(self.lib.wv_query(self.h, what, C.byref(v)))
        return v.value

    def synchronize(self):
        _check(self.lib.wv_synchronize(self.h))

    def set_stream_tuning(self, variant=2, rows_per_wave=0, waves_x=0, waves_y=0, knob=0):
        _check(self.lib.wv_set_stream_tuning(self.h, variant, rows_per_wave, waves_x, waves_y, knob))

    # ---- slab communicator ------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        _check(load_library().wv_comm_unique_id(buf))
        return bytes(buf)

    @staticmethod
    def comm_use_library(path):
        """wv_comm_use_library: resolve the RCCL entry points in exactly this shared library (before any communicator)."""
        lib = load_library()
        lib.wv_comm_use_library.argtypes = [C.c_char_p]
        _check(lib.wv_comm_use_library(path.encode() if path else None))

    def comm_init(self, id_bytes, rank, nranks):
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(id_bytes)
        _check(self.lib.wv_comm_init(self.h, buf, rank, nranks))


class LocalSlabGroup:
    """A z-slab chain whose slabs are engines of this process (wv_comm_init_local / wv_run_group):
    `engines[r]` is slab r.  Same step code as the one-rank-per-GPU RCCL chain, other transport."""

    def __init__(self, engines):
        self.engines = list(engines)
        self.lib = load_library()
        self._handles = (C.c_void_p * len(self.engines))(*[e.h for e in self.engines])
        _check(self.lib.wv_comm_init_local(self._handles, len(self.engines)))

    def run_steps(self, n_steps):
        done = C.c_uint64()
        flag = C.c_int32()
        _check(self.lib.wv_run_group(self._handles, len(self.engines), int(n_steps), C.byref(done), C.byref(flag)))
        return done.value, flag.value

    def close(self):
        for e in self.engines:
            if e.h:
                self.lib.wv_comm_destroy(e.h)
        for e in self.engines:
            e.close()


def run(engine, pre, post, keep_going=lambda: True):
    """`waveguide::run<pre, post>` with arbitrary callbacks (waveguide.h:36-126): the generic,
    per-step-synchronised path.  pre(engine, step) -> bool; post(engine, step) -> None; both see
    the `current` buffer through engine.read_value / write_value / read_field / write_field."""
    step = 0
    while pre(engine, step) and keep_going():
        flag = engine.step()
        raise_for_flag(flag)
        post(engine, step)
        engine.swap()
        step += 1
    return step


def run_fast(engine, source_kind, source_node, signal, receivers, keep_going=lambda: True, chunk=1024):
    """`run` with a hard/soft single-node source and node receivers, device resident.
    Returns (steps, out[steps, n_receivers])."""
    n = len(signal)
    engine.set_source(source_kind, source_node, signal)
    engine.set_receivers(receivers)
    first = engine.step_count()
    done_total = 0
    while done_total < n and keep_going():
        done, flag = engine.run_steps(min(chunk, n - done_total))
        done_total += done
        raise_for_flag(flag)
        if done == 0:
            break
    return done_total, engine.fetch_receivers(first, done_total)


def run_fast_slabs(mesh, slabs, source_kind, source_node, signal, receivers, precision="f64", devices=None,
                   keep_going=lambda: True, chunk=1024, tuning=None):
    """`run_fast` on a mesh cut into `slabs` z-slabs that live in THIS process -- on the GPUs listed in `devices`
    (slab r on devices[r % len(devices)]; default: all on the current device) -- joined by the in-process transport
    and stepped together (wv_comm_init_local / wv_run_group: the step code of the one-rank-per-GPU RCCL chain,
    face planes travelling by device-to-device copies).  Returns (steps, out[steps, n_receivers]) exactly as
    run_fast on the whole mesh does, bit for bit."""
    from .slab import SlabLayout, place_source_and_receivers, slab_mesh
    devices = list(devices) if devices else [-1]
    engines, owners = [], []
    try:
        for r in range(slabs):
            L = SlabLayout(mesh.dims, r, slabs)
            eng = Engine(slab_mesh(mesh, L), precision=precision, device=devices[r % len(devices)],
                         ghost_lo=L.ghost_lo, ghost_hi=L.ghost_hi, tuning=tuning)
            engines.append(eng)
            src_local, mine = place_source_and_receivers(L, source_node, receivers)
            if src_local is not None:
                eng.set_source(source_kind, src_local, signal)
            eng.set_receivers([idx for _, idx in mine])
            owners.append([pos for pos, _ in mine])
        group = LocalSlabGroup(engines)
    except Exception:
        for e in engines:
            e.close()
        raise
    try:
        n = len(signal)
        done_total = 0
        while done_total < n and keep_going():
            done, flag = group.run_steps(min(chunk, n - done_total))
            done_total += done
            raise_for_flag(flag)
            if done == 0:
                break
        out = np.zeros((done_total, len(receivers)))
        for eng, cols in zip(engines, owners):
            if cols:
                out[:, cols] = eng.fetch_receivers(0, done_total)
        return done_total, out
    finally:
        group.close()


class _ResidentMesh:
    """What Engine's buffer helpers need to know about a mesh whose nodes never came to the host."""

    def __init__(self, dims, counts):
        self.dims = dims
        self.num_nodes = dims[0] * dims[1] * dims[2]
        self.bidx = [np.broadcast_to(np.uint32(0), (counts[d], d + 1)) for d in range(3)]
        self.nodes = None


class SceneMesh:
    """wv_scene_mesh: the scene -> mesh chain run on the device, results resident in HBM.
    `fetch()` brings (nodes, [b1, b2, b3]) to the host; `engine()` builds an Engine on the
    device-resident nodes without that round trip."""

    def __init__(self, dims, min_corner, spacing, voxel_index, aabb, side, triangles, vertices, device=-1):
        self.lib = load_library()
        L = self.lib
        L.wv_scene_mesh_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_uint32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.wv_scene_mesh_fetch.argtypes = [C.c_void_p] * 5
        L.wv_scene_mesh_create_engine.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(WvOptions),
                                                  C.POINTER(C.c_void_p)]
        L.wv_scene_mesh_destroy.argtypes = [C.c_void_p]
        L.wv_scene_mesh_destroy.restype = None
        self.dims = tuple(int(d) for d in dims)
        nx, ny, nz = self.dims
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        t = np.ascontiguousarray(triangles, dtype=np.uint32)
        vox = np.ascontiguousarray(voxel_index, dtype=np.uint32)
        mc = np.ascontiguousarray(min_corner, dtype=np.float32)
        a0 = np.ascontiguousarray(aabb[0], dtype=np.float32)
        a1 = np.ascontiguousarray(aabb[1], dtype=np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        counts = (C.c_uint64 * 3)()
        h = C.c_void_p()
        _check(L.wv_scene_mesh_create(nx, ny, nz, p(mc), float(spacing), p(vox), vox.shape[0], p(a0), p(a1), int(side),
                                      p(t), t.shape[0], p(v), v.shape[0], int(device), C.byref(h), counts))
        self.h = h
        self.counts = tuple(int(c) for c in counts)
        self.spacing = float(spacing)
        self.min_corner = mc

    def fetch(self, nodes=True):
        nx, ny, nz = self.dims
        n = np.zeros(nx * ny * nz, dtype=M.condensed_node_dtype) if nodes else None
        b = [np.zeros((self.counts[d], d + 1), dtype=np.uint32) for d in range(3)]
        _check(self.lib.wv_scene_mesh_fetch(self.h, n.ctypes.data_as(C.c_void_p) if nodes else None,
                                            *[x.ctypes.data_as(C.c_void_p) for x in b]))
        return n, b

    def engine(self, coefficients, precision="f64", **kw):
        """An Engine on the device-resident nodes.  Its .mesh holds no node array."""
        coeffs = np.ascontiguousarray(coefficients, dtype=M.coefficients_dtype)
        opt = WvOptions()
        self.lib.wv_default_options(C.byref(opt))
        opt.precision = PRECISION_F32 if precision == "f32" else PRECISION_F64
        opt.flag_interval = kw.get("flag_interval", 0)
        opt.stream_variant = kw.get("stream_variant", 2)
        opt.all_tiles = 1 if kw.get("all_tiles", False) else 0
        apply_tuning(opt, kw.get("tuning"))
        handle = C.c_void_p()
        _check(self.lib.wv_scene_mesh_create_engine(self.h, coeffs.ctypes.data_as(C.c_void_p), coeffs.shape[0],
                                                    C.byref(opt), C.byref(handle)))
        return Engine.from_handle(handle, _ResidentMesh(self.dims, self.counts), precision)

    def close(self):
        if getattr(self, "h", None):
            self.lib.wv_scene_mesh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""Transparent sources: ctypes front of wayverb_amd/csrc/compensation_signal.hip.

A soft source fed make_transparent(x) leaves the pressure at its node equal to x: the input minus the mesh's own impulse
response at the excitation node, convolved with the input (src/waveguide/src/make_transparent.cpp:10-30).  That response
comes from the free-field waveguide folded onto 1/48 of space (compressed_rectangular_waveguide,
src/waveguide/compensation_signal/), which runs on the GPU here -- the reference compiles a 512-tap table in at build
time; this module makes it on the device at first use and keeps it for the process."""
import ctypes as C

import numpy as np

from .engine import SOURCE_HARD, SOURCE_SOFT, _check, load_library


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def compressed_waveguide(signal, steps, soft=False, device=-1):
    """run_hard_source / run_soft_source of a compressed_rectangular_waveguide of `steps` steps: node 0 after each of the
    2 * ((steps + 1) // 2) steps, as float32."""
    lib = load_library()
    lib.wv_compressed_waveguide_run.argtypes = [C.c_int32, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p]
    x = np.ascontiguousarray(signal, dtype=np.float32)
    out = np.zeros(2 * ((int(steps) + 1) // 2), dtype=np.float32)
    _check(lib.wv_compressed_waveguide_run(int(device), int(steps), SOURCE_SOFT if soft else SOURCE_HARD, _p(x), x.shape[0],
                                           _p(out)))
    return out


def mesh_impulse_response(taps, device=-1):
    """The table `write_compensation_signal <taps>` prints (compensation_signal/cmd/main.cpp:42-60): the hard source {0, 1},
    first `taps` outputs."""
    return compressed_waveguide([0.0, 1.0], taps, device=device)[:taps]


_responses = {}


def make_transparent(x, taps=512, response=None):
    """waveguide::make_transparent: x minus (right_hanning(taps) * response) convolved with x, len(x) + taps - 1 floats.
    Without a `response` the mesh's own, of `taps` taps, is made on the device once per process."""
    if response is None:
        if taps not in _responses:
            _responses[taps] = mesh_impulse_response(taps)
        response = _responses[taps]
    h = np.ascontiguousarray(response, dtype=np.float32)
    if h.shape[0] != taps:
        raise ValueError("response has %d taps, expected %d" % (h.shape[0], taps))
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(x.shape[0] + taps - 1, dtype=np.float32)
    lib = load_library()
    lib.wv_make_transparent.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    _check(lib.wv_make_transparent(_p(x), x.shape[0], _p(h), taps, _p(out)))
    return out

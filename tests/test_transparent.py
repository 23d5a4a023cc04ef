"""CPU: transparent sources (wayverb_amd/transparent.py, csrc/compensation_signal.hip).  wv_make_transparent against the
restatement of make_transparent.cpp:10-30 in tests/test_transparent_source_kat.py; the generator of the mesh response fails
loudly without a GPU (no CPU fallback), in C, Python and C++; its kernel keeps out of scratch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_transparent_source_kat import make_transparent as restated_make_transparent
from test_transparent_source_kat import mesh_impulse_response as restated_mesh_impulse_response
from test_transparent_source_kat import mesh_impulse_response_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "compensation_signal_test.cpp")
CPP_EXE = os.path.join(ROOT, "tests", "cpp", "compensation_signal_test")


def build_cpp_test(built_library):
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), CPP_SRC,
                           "-o", CPP_EXE, "-L", os.path.join(ROOT, "wayverb_amd"), "-lwayverb_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "wayverb_amd")])
    return CPP_EXE


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def _inputs():
    rng = np.random.default_rng(20)
    return {"ones": np.ones(20, dtype=np.float32),
            "ramp": np.array([1, 2, 3, 4, 5, 4, 3, 2, 1], dtype=np.float32),
            "random420": rng.standard_normal(420).astype(np.float32),
            "random85173": rng.uniform(-1, 1, 85173).astype(np.float32)}


@pytest.fixture(scope="module")
def short_response():
    return restated_mesh_impulse_response(8)


@pytest.mark.parametrize("name", ["ones", "ramp", "random420", "random85173"])
@pytest.mark.parametrize("table", ["golden512", "mesh8"])
def test_make_transparent_matches_the_restatement(built_library, short_response, name, table):
    from wayverb_amd import transparent as T
    x = _inputs()[name]
    h = mesh_impulse_response_table() if table == "golden512" else short_response
    got = T.make_transparent(x, taps=len(h), response=h)
    want = restated_make_transparent(x, h, table_length=len(h))
    assert got.dtype == np.float32 and got.shape == want.shape == (len(x) + len(h) - 1,)
    # one float ulp of the restatement, or (where the value is near zero and numpy's summation order shows) 1e-9 of the input
    ulp = np.spacing(np.abs(want))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all((err <= ulp) | (err <= 1e-9 * np.abs(x).max())), err.max()


def test_make_transparent_of_a_unit_impulse_is_minus_the_windowed_response(built_library):
    from wayverb_amd import transparent as T
    h = mesh_impulse_response_table()
    got = T.make_transparent([1.0], response=h)
    k = np.arange(512)
    window = (0.5 - 0.5 * np.cos(2 * np.pi * (0.5 + k / (2 * 511.0)))).astype(np.float32)
    want = -(window * h)
    want[0] += 1
    assert np.array_equal(got, want.astype(np.float32))      # (+0 where the response is 0: 0 - 0)


def test_make_transparent_refuses_bad_arguments(built_library):
    from wayverb_amd import engine as E
    from wayverb_amd import transparent as T
    with pytest.raises(ValueError):
        T.make_transparent([1.0], taps=4, response=[0.0, 0.0, 1.0])
    with pytest.raises(E.WaveguideError, match="at least 2 taps"):
        T.make_transparent([1.0], taps=1, response=[0.0])
    assert T.make_transparent([], taps=3, response=[0.0, 0.0, 1.0]).tobytes() == np.zeros(2, np.float32).tobytes()


def test_compressed_waveguide_without_a_gpu_fails_loudly(built_library):
    _no_gpu()
    from wayverb_amd import engine as E
    from wayverb_amd import transparent as T
    for call in (lambda: T.compressed_waveguide([0.0, 1.0], 8), lambda: T.compressed_waveguide([1.0], 9, soft=True),
                 lambda: T.mesh_impulse_response(512), lambda: T.make_transparent(np.ones(20, np.float32))):
        with pytest.raises(E.WaveguideError, match="no HIP device"):
            call()
    lib = ctypes.CDLL(built_library)
    out = np.zeros(8, dtype=np.float32)
    x = np.array([0.0, 1.0], dtype=np.float32)
    rc = lib.wv_compressed_waveguide_run(ctypes.c_int32(-1), ctypes.c_uint64(8), ctypes.c_int32(1), x.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.c_uint64(2), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == -4 and not out.any()       # WV_E_NO_DEVICE, nothing computed on the host


def test_compressed_waveguide_refuses_a_bad_source_kind(built_library):
    lib = ctypes.CDLL(built_library)
    lib.wv_last_error.restype = ctypes.c_char_p
    out = np.zeros(8, dtype=np.float32)
    rc = lib.wv_compressed_waveguide_run(ctypes.c_int32(-1), ctypes.c_uint64(8), ctypes.c_int32(0), None, ctypes.c_uint64(0),
                                         out.ctypes.data_as(ctypes.c_void_p))
    assert rc == -1 and b"source_kind" in lib.wv_last_error()


def test_cpp_mirror_compiles_and_reports_the_missing_device(built_library):
    exe = build_cpp_test(built_library)
    _no_gpu()
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "no HIP device" in p.stdout, p.stdout + p.stderr


def test_the_compressed_waveguide_kernel_does_not_spill(built_library):
    from wayverb_amd import build as B
    text = open(B.COMPENSATION_RESOURCES).read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    assert any("compressed_waveguide_kernel" in b.split()[0] for b in blocks)
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split()[0]
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b.split()[0]

"""The cl::Buffer mirror of the C++ headers at a declared cadence (include/wayverb_amd/cl_mirror.h, cl_mirror_cadence()): built against
the OpenCL C++ bindings and the library, run on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cl_mirror_cadence_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "cl_mirror_cadence_test")
OPENCL_INCLUDE = "/opt/rocm/include"     # CL/cl.hpp, the bindings the reference uses (core/cl/include.h)


def _build(built_library):
    if not os.path.exists(os.path.join(OPENCL_INCLUDE, "CL", "cl.hpp")):
        pytest.skip("no OpenCL C++ bindings in this image")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-DCL_TARGET_OPENCL_VERSION=120",
                           "-isystem", OPENCL_INCLUDE, "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                           "-L", os.path.join(ROOT, "wayverb_amd"), "-lwayverb_amd", "-lOpenCL",
                           "-Wl,-rpath," + os.path.join(ROOT, "wayverb_amd")])


def test_cl_mirror_cadence_compiles_against_the_mirror(built_library):
    _build(built_library)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = subprocess.run([EXE], capture_output=True, text=True)
    assert p.returncode in (2, 3), p.stdout + p.stderr       # no OpenCL device found / no HIP device here: said so, not crashed


@pytest.mark.gpu
def test_cl_mirror_at_a_declared_cadence_follows_the_run_without_rollbacks(built_library):
    """tests/cpp/cl_mirror_cadence_test.cpp: `canonical` with cl_mirror_cadence() = 4 and a two-plane range on a 40^3 room, 90 steps.
    At every fourth callback the cl::Buffer's planes equal those of a step-by-step run, in between they keep the last mirrored field,
    the rest of the buffer stays zero; rollbacks == 0, fields_mirrored == 23, and the run took whole batches."""
    _build(built_library)
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    if p.returncode == 3:
        pytest.skip("no OpenCL GPU device on this box: " + p.stdout.strip())
    assert p.returncode == 0 and "CL MIRROR CADENCE OK" in p.stdout, p.stdout + p.stderr

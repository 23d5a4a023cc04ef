"""`canonical_many` of the C++ headers (include/wayverb_amd/waveguide.h, setup.h): built against the library, run on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "receiver_array_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "receiver_array_test")


def _build(built_library):
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                           "-L", os.path.join(ROOT, "wayverb_amd"), "-lwayverb_amd", "-Wl,-rpath," + os.path.join(ROOT, "wayverb_amd")])


def test_receiver_array_test_compiles_against_the_headers(built_library):
    _build(built_library)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = subprocess.run([EXE], capture_output=True, text=True)
    assert p.returncode == 2 and "no HIP device" in p.stdout, p.stdout + p.stderr      # said so, not crashed


@pytest.mark.gpu
def test_canonical_many_gives_every_receiver_the_band_canonical_gives_it(built_library):
    """tests/cpp/receiver_array_test.cpp: four receivers on a 40^3 room, 90 steps, one run; each band bytewise equal to `canonical`
    for that receiver; the progress callback fired 90 times, in order."""
    _build(built_library)
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "RECEIVER ARRAYS OK" in p.stdout, p.stdout + p.stderr

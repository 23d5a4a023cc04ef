"""Lateral maps, the parts that need no GPU: the planning header (wayverb_amd/csrc/lateral_plan.h) against hand-derived cases, the new
entry points and wv_lateral_plan's layout, the fold kernel's resource usage as the build reported it, and the Python layer's
arguments.  (The kernel's text on the host is tests/test_lateral_host.py's; what wv_set_lateral does with a plan is
tests/test_gpu_lateral.py's.)"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from wayverb_amd import lateral as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")

NEW = ("wv_set_lateral", "wv_lateral_count", "wv_fetch_lateral")


def test_lateral_planning_header_against_hand_derived_cases():
    """tests/cpp/lateral_plan_test.cpp: what a plan is refused for and in which order, the reference's sentence on every face of the
    mesh; the places and sizes of the state block, their alignment for odd B and their overflow checks; the traffic model.  (That
    the other plans' setters refuse, with which words, is tests/test_gpu_lateral.py's, on the engine itself.)"""
    src = os.path.join(ROOT, "tests", "cpp", "lateral_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "lateral_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "LATERAL PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    # the plan's header is host code: no HIP in it; the fold uses neither LDS nor atomics
    header = open(os.path.join(CSRC, "lateral_plan.h")).read().split("#pragma once")[1]
    assert "hip" not in header.lower()
    kernel = open(os.path.join(CSRC, "lateral_kernels.hip.h")).read().split("#pragma once")[1]
    assert "__shared__" not in kernel and "atomic" not in kernel


def test_lateral_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_lateral", "lateral_count", "fetch_lateral"):
        assert callable(getattr(E.Engine, method))
    for fn in ("lateral_fold", "direct_direction", "lateral_axis", "figure_of_eight_energy", "lateral_fraction", "energy_density", "diffuseness",
               "edges_from_ms"):
        assert callable(getattr(L, fn))
    assert (E.Engine.QUERY_LATERAL_CAPTURES, E.Engine.QUERY_LATERAL_FOLDS, E.Engine.QUERY_LATERAL_NS, E.Engine.QUERY_LATERAL_GATHER_NS,
            E.Engine.QUERY_LATERAL_GATHERS) == (40, 41, 42, 43, 44)
    assert L.NONE == E.ARRIVAL_NONE and len(L.PLANES) == 10 and L.MAX_BINS == 8


def test_lateral_plan_struct_has_the_documented_size_and_offsets():
    """wv_lateral_plan as a C compiler lays the header's declaration out: the box and the cadence where wv_decay_plan has them, n_bins
    at 56, the threshold at 60, eight edges from 64, the three doubles from 96 -- 120 bytes -- and the ctypes mirror agrees; the query
    ids follow 39 and nothing before them is renumbered."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_bins", "threshold", "edges", "spacing", "sample_rate",
              "ambient_density"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_lateral_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_lateral_plan, %s));' % f for f in fields) + \
        'printf(" %zu %d %d %d %d %d %d %d", sizeof(((wv_lateral_plan*)0)->edges), WV_QUERY_LATERAL_CAPTURES, WV_QUERY_LATERAL_FOLDS, ' \
        'WV_QUERY_LATERAL_NS, WV_QUERY_LATERAL_GATHER_NS, WV_QUERY_LATERAL_GATHERS, WV_QUERY_ARRIVAL_NS, WV_QUERY_INTENSITY_GATHERS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 64, 96, 104, 112]
    assert got == [120] + offsets + [32, 40, 41, 42, 43, 44, 39, 36]
    assert [ctypes.sizeof(E.WvLateralPlan)] + [getattr(E.WvLateralPlan, f).offset for f in fields] == [120] + offsets


def test_the_fold_kernel_needs_no_scratch_and_spills_nothing(built_library):
    """The compiler's resource metadata for lateral_fold_kernel, written beside the library by wayverb_amd.build: ScratchSize 0 (no
    array is indexed by a lane's value), no VGPR and no SGPR spill, no LDS, at most the 64 VGPRs that keep eight waves per SIMD.
    profiles/r14/lateral_kernel_resources.txt records what a build for gfx950 reported."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "lateral_fold_kernel" in b.split()[0]]
    assert len(blocks) == 1
    for what in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill", r"LDS Size \[bytes/block\]"):
        assert int(re.search(what + r": (\d+)", blocks[0]).group(1)) == 0, blocks[0]
    assert int(re.search(r"VGPRs: (\d+)", blocks[0]).group(1)) <= 64, blocks[0]
    assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blocks[0]).group(1)) >= 8, blocks[0]
    recorded = open(os.path.join(ROOT, "profiles", "r14", "lateral_kernel_resources.txt")).read()
    assert recorded.count("Function Name:") == 1 and "ScratchSize [bytes/lane]: 0" in recorded
    assert "VGPRs Spill: 0" in recorded and "SGPRs Spill: 0" in recorded and "LDS Size [bytes/block]: 0" in recorded


def test_python_arguments_to_plan():
    """Engine.set_lateral turns (origin, extent, stride) into nodes taken per axis as set_intensity does (no box: the mesh's
    interior), the edge list into n_bins and the table, the map into float32 of the box's shape; nine edges and a map of another
    shape are refused before the library is asked."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_lateral(self, handle, plan, threshold_map):
            self.plan = plan._obj if plan is not None else None
            self.map = threshold_map
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    assert eng.set_lateral((0, 40, 640), 1e-3, spacing=0.05, sample_rate=8000.0, ambient_density=1.2) == (10, 3, 26, 18, 22)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.n_bins) == (1, 1, 1, 22, 18, 26, 1, 1, 1, 3)
    assert list(p.edges)[:4] == [0, 40, 640, 0] and p.threshold == np.float32(1e-3) and eng.lib.map is None
    assert (p.spacing, p.sample_rate, p.ambient_density) == (0.05, 8000.0, 1.2)
    shape = eng.set_lateral([0], 0.0, box=((1, 1, 2), (21, 18, 24)), stride=(1, 2, 3), first_step=5, period=7, threshold_map=np.ones((8, 9, 21)),
                            spacing=1, sample_rate=2, ambient_density=3)
    p = eng.lib.plan
    assert shape == (10, 1, 8, 9, 21) == eng.lateral_shape and eng.lib.map is not None
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.n_bins) == (1, 1, 2, 21, 9, 8, 1, 2, 3, 5, 7, 1)
    with pytest.raises(ValueError):
        eng.set_lateral(range(9), 0.0, spacing=1, sample_rate=1, ambient_density=1)
    with pytest.raises(ValueError):
        eng.set_lateral((0, 1), 0.0, threshold_map=np.ones((2, 2, 2)), spacing=1, sample_rate=1, ambient_density=1)
    assert eng.set_lateral(None) is None and eng.lib.plan is None and eng.lateral_shape is None
    eng.h = None


def test_canonical_fills_in_the_plan():
    """simulation.lateral_plan_arguments: a plane in metres becomes that plane less its rim; the edges are edges_ms at the rate of the
    captured series, which is also the rate the integrator is given; a plane on a face of the mesh, no threshold, both plane and box,
    an unknown key, every=0, edges that do not begin with 0 and nine of them are refused."""
    from wayverb_amd import simulation as W

    class Mesh:
        dims, spacing, min_corner = (24, 20, 28), 0.05, (0.0, -0.5, 1.0)

    class Env:
        ambient_density = 1.2

    plan = W.lateral_plan_arguments(dict(plane=1.55, every=2, threshold=1e-3), Mesh, 8000.0, Env)
    assert plan == dict(edges=[0, 20, 320], threshold=1e-3, threshold_map=None, box=((1, 1, 11), (22, 18, 1)), stride=1, first_step=0, period=2,
                        spacing=0.05, sample_rate=4000.0, ambient_density=1.2)
    plan = W.lateral_plan_arguments(dict(box=((1, 1, 1), (4, 4, 4)), threshold=0.0, edges_ms=(0, 10)), Mesh, 8000.0, Env)
    assert (plan["edges"], plan["period"], plan["box"], plan["sample_rate"]) == ([0, 80], 1, ((1, 1, 1), (4, 4, 4)), 8000.0)
    for bad in (dict(plane=1.0, threshold=1.0), dict(plane=2.35, threshold=1.0), dict(threshold=1.0), dict(plane=1.5),
                dict(plane=1.5, box=((1, 1, 1), (2, 2, 2)), threshold=1.0), dict(plane=1.5, threshold=1.0, window=3),
                dict(plane=1.5, threshold=1.0, every=0), dict(plane=1.5, threshold=1.0, edges_ms=(0, 50, 50.01)),
                dict(plane=1.5, threshold=1.0, edges_ms=(5, 80)), dict(plane=1.5, threshold=1.0, edges_ms=tuple(range(0, 90, 10)))):
        with pytest.raises(ValueError):
            W.lateral_plan_arguments(bad, Mesh, 8000.0, Env)

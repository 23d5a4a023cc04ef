"""Arrival-aligned energy maps, the parts that need no GPU: the planning header (wayverb_amd/csrc/arrival_plan.h) against hand-derived
cases, the new entry points and wv_arrival_plan's layout, the fold kernel's resource usage as the build reported it, and the Python
layer's arguments.  (The kernel's text on the host is tests/test_arrival_host.py's; what wv_set_arrival does with a plan is
tests/test_gpu_arrival.py's.)"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from wayverb_amd import arrival as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")

NEW = ("wv_set_arrival", "wv_arrival_count", "wv_fetch_arrival")


def test_arrival_planning_header_against_hand_derived_cases():
    """tests/cpp/arrival_plan_test.cpp: which edge tables and thresholds are refused; the bin of rel, with rel equal to each edge, one
    below it and 2^32 - 2; the places and sizes of the state block with their overflow checks; the traffic model."""
    src = os.path.join(ROOT, "tests", "cpp", "arrival_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "arrival_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ARRIVAL PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    # the plan's header is host code: no HIP in it; the engine file keeps no stage bookkeeping of its own; one launch site
    assert "hip" not in open(os.path.join(CSRC, "arrival_plan.h")).read().split("#pragma once")[1].lower()
    text = open(os.path.join(CSRC, "engine_arrival.hip.h")).read()
    for word in ("spectrum_good_captures", "steps.push_back", "hipEventElapsedTime", "plan_batch_end(", "begin_run("):
        assert word not in text, word
    shared = open(os.path.join(CSRC, "engine_staged.hip.h")).read()   # (the life cycle's one copy, on capture_stage.h's bookkeeping)
    assert ".st." in shared and "spectrum_good_captures" not in shared and "steps.push_back" not in shared
    launches = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip")) and
                re.search(r"hipLaunchKernelGGL\(\(?wv::arrival_fold_kernel\b", open(os.path.join(CSRC, name)).read())]
    assert launches == ["engine_arrival.hip.h"]
    # every other plan's setter refuses while an arrival plan is active, in the wording of the existing refusals: each plan's sentence
    # stands once in all of the sources, in the one function every setter's file calls
    sources = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip", ".cpp"))}
    for sentence in ("a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)", "a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)",
                     "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)", "a decay plan is active (wv_set_decay(e, NULL) stops it)",
                     "an intensity plan is active (wv_set_intensity(e, NULL) stops it)", "an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it)",
                     "a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it)"):
        assert sum(text.count(sentence + "; the plans exclude each other") for text in sources.values()) == 1, sentence
    assert "two plans exclude" not in "".join(sources.values())
    for name in ("engine_snapshot.hip.h", "engine_spectrum.hip.h", "engine_decay.hip.h", "engine_intensity.hip.h", "engine_arrival.hip.h", "engine_lateral.hip.h"):
        # (engine_decay.hip.h keeps the one refusal that is its own: a banded plan asked for under a plain one)
        assert sources[name].count("plan_refused(") == 1 and sources[name].count("plan is active (") == (name == "engine_decay.hip.h"), name


def test_arrival_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_arrival", "arrival_count", "fetch_arrival"):
        assert callable(getattr(E.Engine, method))
    for fn in ("arrival_fold", "edges_from_ms", "arrival_time", "clarity", "definition", "centre_time", "direct_level_db"):
        assert callable(getattr(A, fn))
    assert (E.Engine.QUERY_ARRIVAL_CAPTURES, E.Engine.QUERY_ARRIVAL_FOLDS, E.Engine.QUERY_ARRIVAL_NS) == (37, 38, 39)
    assert E.ARRIVAL_NONE == A.NONE == 0xFFFFFFFF


def test_arrival_plan_struct_has_the_documented_size_and_offsets():
    """wv_arrival_plan as a C compiler lays the header's declaration out: the box and the cadence where wv_decay_plan has them, n_bins
    at 56, the threshold at 60, sixteen edges from 64 -- 128 bytes -- and the ctypes mirror agrees; the query ids follow 36."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_bins", "threshold", "edges"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_arrival_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_arrival_plan, %s));' % f for f in fields) + \
        'printf(" %zu %d %d %d", sizeof(((wv_arrival_plan*)0)->edges), WV_QUERY_ARRIVAL_CAPTURES, WV_QUERY_ARRIVAL_FOLDS, WV_QUERY_ARRIVAL_NS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 64]
    assert got == [128] + offsets + [64, 37, 38, 39]
    assert [ctypes.sizeof(E.WvArrivalPlan)] + [getattr(E.WvArrivalPlan, f).offset for f in fields] == [128] + offsets


def test_the_fold_kernel_needs_no_scratch_and_spills_nothing(built_library):
    """The compiler's resource metadata for arrival_fold_kernel, written beside the library by wayverb_amd.build: ScratchSize 0 (no
    array is indexed by a lane's value), no VGPR and no SGPR spill, no LDS, at most the 64 VGPRs that keep eight waves per SIMD.
    profiles/r13/arrival_kernel_resources.txt records what a build for gfx950 reported."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "arrival_fold_kernel" in b.split()[0]]
    assert len(blocks) == 1
    for what in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill", r"LDS Size \[bytes/block\]"):
        assert int(re.search(what + r": (\d+)", blocks[0]).group(1)) == 0, blocks[0]
    assert int(re.search(r"VGPRs: (\d+)", blocks[0]).group(1)) <= 64, blocks[0]
    assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blocks[0]).group(1)) >= 8, blocks[0]
    recorded = open(os.path.join(ROOT, "profiles", "r13", "arrival_kernel_resources.txt")).read()
    assert recorded.count("Function Name:") == 1 and "ScratchSize [bytes/lane]: 0" in recorded
    assert "VGPRs Spill: 0" in recorded and "SGPRs Spill: 0" in recorded


def test_python_arguments_to_plan():
    """Engine.set_arrival turns (origin, extent, stride) into nodes taken per axis as set_snapshots does, the edge list into n_bins and
    the table, the map into float32 of the box's shape; 17 edges and a map of another shape are refused before the library is asked."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_arrival(self, handle, plan, threshold_map):
            self.plan = plan._obj if plan is not None else None
            self.map = threshold_map
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    assert eng.set_arrival((0, 400, 640), 1e-3) == (3, 28, 20, 24)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.n_bins) == (0, 0, 0, 24, 20, 28, 1, 1, 1, 3)
    assert list(p.edges)[:4] == [0, 400, 640, 0] and p.threshold == np.float32(1e-3) and eng.lib.map is None
    shape = eng.set_arrival([0], 0.0, box=((1, 1, 2), (21, 18, 24)), stride=(1, 2, 3), first_step=5, period=7, threshold_map=np.ones((8, 9, 21)))
    p = eng.lib.plan
    assert shape == (1, 8, 9, 21) == eng.arrival_shape and eng.lib.map is not None
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.n_bins) == (1, 1, 2, 21, 9, 8, 1, 2, 3, 5, 7, 1)
    with pytest.raises(ValueError):
        eng.set_arrival(range(17), 0.0)
    with pytest.raises(ValueError):
        eng.set_arrival((0, 1), 0.0, threshold_map=np.ones((2, 2, 2)))
    assert eng.set_arrival(None) is None and eng.lib.plan is None and eng.arrival_shape is None
    eng.h = None


def test_canonical_fills_in_the_plan():
    """simulation.arrival_plan_arguments: a plane in metres becomes that whole plane; the edges are early_ms at the rate of the captured
    series; a plane outside the mesh, no threshold, both plane and box, an unknown key and every=0 are refused."""
    from wayverb_amd import simulation as W

    class Mesh:
        dims, spacing, min_corner = (24, 20, 28), 0.05, (0.0, -0.5, 1.0)

    plan = W.arrival_plan_arguments(dict(plane=1.55, every=2, threshold=1e-3), Mesh, 8000.0)
    assert plan == dict(edges=[0, 200, 320], threshold=1e-3, threshold_map=None, box=((0, 0, 11), (None, None, 1)), stride=1, first_step=0, period=2)
    plan = W.arrival_plan_arguments(dict(box=((1, 1, 1), (4, 4, 4)), threshold=0.0, early_ms=(10,)), Mesh, 8000.0)
    assert (plan["edges"], plan["period"], plan["box"]) == ([0, 80], 1, ((1, 1, 1), (4, 4, 4)))
    for bad in (dict(plane=0.9, threshold=1.0), dict(plane=2.45, threshold=1.0), dict(threshold=1.0), dict(plane=1.5),
                dict(plane=1.5, box=((1, 1, 1), (2, 2, 2)), threshold=1.0), dict(plane=1.5, threshold=1.0, window=3),
                dict(plane=1.5, threshold=1.0, every=0), dict(plane=1.5, threshold=1.0, early_ms=(50, 50.01))):
        with pytest.raises(ValueError):
            W.arrival_plan_arguments(bad, Mesh, 8000.0)

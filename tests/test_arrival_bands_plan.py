"""Band-limited arrival maps, the parts that need no GPU: the planning header (wayverb_amd/csrc/arrival_bands_plan.h) against hand-derived
cases, the new entry points and wv_arrival_bands_plan's layout, the fold kernel's resource usage as the build reported it, where the
plan touches the engine's sources, and the Python layer's arguments.  (The kernel's text on the host is
tests/test_arrival_bands_host.py's; what wv_set_arrival_bands does with a plan is tests/test_gpu_arrival_bands.py's.)"""
import ctypes
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from wayverb_amd import arrival as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")
NEW = ("wv_set_arrival_bands", "wv_arrival_bands_count", "wv_fetch_arrival_bands")
SENTENCE = "a banded arrival plan is active (wv_set_arrival_bands(e, NULL, NULL, NULL, 0, 0) stops it); the plans exclude each other"
OLD_SENTENCES = ("a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)", "a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)",
                 "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)", "a decay plan is active (wv_set_decay(e, NULL) stops it)",
                 "an intensity plan is active (wv_set_intensity(e, NULL) stops it)", "an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it)",
                 "a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it)",
                 "a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it)")


def test_planning_header_against_hand_derived_cases():
    """tests/cpp/arrival_bands_plan_test.cpp: which tails are refused; rel under a lag, a lag larger than d included; bin(rel) at every
    edge, one below it, tail_first and tail_first - 1, the tail's last boundary and 2^32 - 2; the table of the bins' first rels and the
    walk by it; places and sizes of both blocks with their overflow answers; the traffic model.  The header is host code: no HIP."""
    src = os.path.join(ROOT, "tests", "cpp", "arrival_bands_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "arrival_bands_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ARRIVAL BANDS PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    header = open(os.path.join(CSRC, "arrival_bands_plan.h")).read()
    assert "hip" not in header.split("#pragma once")[1].lower()
    assert sorted(re.findall(r"#include [<\"]([^>\"]+)[>\"]", header)) == ["arrival_plan.h", "cstdint"]


def test_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_arrival_bands", "arrival_bands_count", "fetch_arrival_bands"):
        assert callable(getattr(E.Engine, method))
    for fn in ("banded_arrival_fold", "band_edges", "lag_captures", "band_clarity", "band_definition", "band_centre_time", "band_decay_maps"):
        assert callable(getattr(A, fn))
    assert (E.Engine.QUERY_ARRIVAL_BANDS_CAPTURES, E.Engine.QUERY_ARRIVAL_BANDS_FOLDS, E.Engine.QUERY_ARRIVAL_BANDS_NS) == (48, 49, 50)


def test_plan_struct_has_the_documented_size_and_offsets():
    """wv_arrival_bands_plan as a C compiler lays the header's declaration out: the box and the cadence where every plan has them,
    n_edges at 56, the threshold at 60, sixteen edges from 64, the tail's three words from 128, eight lags from 140, reserved at 172
    -- 176 bytes, as the header's comment says -- and the ctypes mirror agrees; the query ids follow the modulation plan's 47."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_edges", "threshold", "edges", "n_tail",
              "tail_first", "tail_captures", "lag", "reserved"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_arrival_bands_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_arrival_bands_plan, %s));' % f for f in fields) + \
        'printf(" %zu %zu %d %d %d", sizeof(((wv_arrival_bands_plan*)0)->edges), sizeof(((wv_arrival_bands_plan*)0)->lag), ' \
        'WV_QUERY_ARRIVAL_BANDS_CAPTURES, WV_QUERY_ARRIVAL_BANDS_FOLDS, WV_QUERY_ARRIVAL_BANDS_NS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 64, 128, 132, 136, 140, 172]
    assert got == [176] + offsets + [64, 32, 48, 49, 50]
    assert [ctypes.sizeof(E.WvArrivalBandsPlan)] + [getattr(E.WvArrivalBandsPlan, f).offset for f in fields] == [176] + offsets
    comment = open(os.path.join(ROOT, "include", "wayverb_amd.h")).read()
    assert "The struct is 176 bytes" in comment and "lag at 140, reserved at 172" in comment


def test_the_fold_kernel_needs_neither_scratch_nor_lds(built_library):
    """The compiler's account of arrival_bands_fold_kernel's four instances (1 .. 4 sections), written beside the library by
    wayverb_amd.build: no scratch, no VGPR or SGPR spill, no LDS, at most the 128 VGPRs that keep four waves per SIMD -- the bar the
    banded decay fold and the modulation fold are held to.  profiles/r19/arrival_bands_kernel_resources.txt records what a build for
    gfx950 reported.  (The names of the arrival fold and the banded decay fold are no substrings of this kernel's.)"""
    from wayverb_amd import build as B
    all_blocks = re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:]
    blocks = [b for b in all_blocks if "arrival_bands_fold_kernel" in b.split()[0]]
    assert len(blocks) == 4
    assert len([b for b in all_blocks if "arrival_fold_kernel" in b.split()[0]]) == 1
    assert len([b for b in all_blocks if "decay_bands_fold_kernel" in b.split()[0]]) == 4
    for b in blocks:
        for what in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill", r"LDS Size \[bytes/block\]"):
            assert int(re.search(what + r": (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 128, b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 4, b
    recorded = open(os.path.join(ROOT, "profiles", "r19", "arrival_bands_kernel_resources.txt")).read()
    assert recorded.count("Function Name:") == 4 and recorded.count("ScratchSize [bytes/lane]: 0") == 4
    assert recorded.count("VGPRs Spill: 0") == 4 and recorded.count("SGPRs Spill: 0") == 4 and recorded.count("LDS Size [bytes/block]: 0") == 4


def test_the_plan_touches_no_other_plans_file():
    """DESIGN.md 4.15's list for a seventh staged plan: its own three files, one launch site of its kernel, one case in each of the two
    switches and one refusal row in engine_staged.hip.h; the other plans' files do not name it; its sentence stands once in all of
    the sources and holds none of the eight existing sentences."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip", ".cpp"))}
    launches = [name for name, t in text.items() if "wv::arrival_bands_fold_kernel<" in t]
    assert launches == ["engine_arrival_bands.hip.h"] and text["engine_arrival_bands.hip.h"].count("hipLaunchKernelGGL((wv::arrival_bands_fold_kernel") == 1
    for name in ("engine_spectrum.hip.h", "engine_decay.hip.h", "engine_intensity.hip.h", "engine_arrival.hip.h", "engine_lateral.hip.h",
                 "engine_modulation.hip.h", "engine_snapshot.hip.h", "engine_io.hip.h", "engine_setup.hip.h", "capture_stage.h", "decay_plan.h",
                 "spectrum_plan.h", "arrival_plan.h", "modulation_plan.h", "lateral_plan.h", "intensity_plan.h", "snapshot_plan.h", "arrival_kernels.hip.h",
                 "decay_bands_kernels.hip.h", "modulation_kernels.hip.h", "fold_parts.hip.h"):
        assert "arrival_bands" not in text[name].lower() and "arrivalbands" not in text[name].lower() and "banded arrival" not in text[name], name
    own = text["engine_arrival_bands.hip.h"]
    for word in ("spectrum_good_captures", "steps.push_back", "hipEventElapsedTime", "plan_batch_end(", "begin_run(", "plan is active ("):
        assert word not in own, word
    assert own.count("plan_refused(") == 1
    for word in ("__shared__", "atomic", " / ", " % "):      # (the fold's one division is arrival_bands_plan.h's, ahead of the capture loop)
        assert word not in text["arrival_bands_kernels.hip.h"].split("#pragma once")[1].split("namespace wv {")[1], word
    staged = text["engine_staged.hip.h"]
    assert staged.count("ArrivalBands&>(p)") == 2 and staged.count("kArrivalBandsRow") == 1 and "kArrivalBandsStage == kSpectrumStage" in staged
    assert sum(t.count(SENTENCE) for t in text.values()) == 1 and SENTENCE in staged
    for old in OLD_SENTENCES:
        assert old not in SENTENCE
        assert sum(t.count(old + "; the plans exclude each other") for t in text.values()) == 1, old
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "arrival_bands_refusals.json")))
    assert all(text_.endswith(SENTENCE) for _, text_ in golden["while_active"].values()) and len(golden["while_active"]) == len(golden["under"]) == 8
    assert all(any(text_.endswith(old + "; the plans exclude each other") for old in OLD_SENTENCES) for _, text_ in golden["under"].values())


def test_python_arguments_to_plan():
    """Engine.set_arrival_bands turns (origin, extent, stride) into nodes taken per axis as set_snapshots does, the edge list into
    n_edges and the table, the tail and the lags into their words, the map into float32 of the box's shape; 17 edges, a 2-D bands
    array, a map of another shape and a lag list of another length are refused before the library is asked."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_arrival_bands(self, handle, plan, threshold_map, sections, n_bands, n_sections):
            self.plan = plan._obj if plan is not None else None
            self.map, self.counts = threshold_map, (n_bands, n_sections)
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    bands = np.zeros((3, 4, 5))
    assert eng.set_arrival_bands((0, 400, 640), bands, 1e-3) == (3, 3, 28, 20, 24) and eng.lib.counts == (3, 4)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.n_edges, p.n_tail, p.reserved) == (0, 0, 0, 24, 20, 28, 1, 1, 1, 3, 0, 0)
    assert list(p.edges)[:4] == [0, 400, 640, 0] and p.threshold == np.float32(1e-3) and eng.lib.map is None and list(p.lag) == [0] * 8
    shape = eng.set_arrival_bands([0], bands[:2, :1], 0.0, tail=(100, 8, 8), lag=(3, 17), box=((1, 1, 2), (21, 18, 24)), stride=(1, 2, 3),
                                  first_step=5, period=7, threshold_map=np.ones((8, 9, 21)))
    p = eng.lib.plan
    assert shape == (2, 101, 8, 9, 21) == eng.arrival_bands_shape and eng.lib.map is not None and eng.lib.counts == (2, 1)
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.n_edges) == (1, 1, 2, 21, 9, 8, 1, 2, 3, 5, 7, 1)
    assert (p.n_tail, p.tail_first, p.tail_captures) == (100, 8, 8) and list(p.lag) == [3, 17, 0, 0, 0, 0, 0, 0]
    eng.set_arrival_bands([0], bands, lag=4)
    assert list(eng.lib.plan.lag) == [4, 4, 4, 0, 0, 0, 0, 0]
    for bad in (dict(edges=range(17), bands=bands), dict(edges=(0, 1), bands=np.zeros((3, 5))), dict(edges=(0, 1), bands=bands, lag=(1, 2)),
                dict(edges=(0, 1), bands=bands, threshold_map=np.ones((2, 2, 2)))):
        with pytest.raises(ValueError):
            eng.set_arrival_bands(bad.pop("edges"), bad.pop("bands"), **bad)
    assert eng.set_arrival_bands(None, None) is None and eng.lib.plan is None and eng.arrival_bands_shape is None
    eng.h = None


def test_band_edges_and_the_time_axis():
    """50 and 80 ms at 8 kHz, every second step: edges 0, 200, 320; a tail of 10 ms bins (40 captures) out to 500 ms (2000 captures)
    begins one bin behind the last edge, at 360, and has ceil((2000 - 360) / 40) = 41 bins; the bins' first captures are the time axis
    of the decay curve."""
    edges, tail = A.band_edges((50, 80), 500, 10, 2, 8000.0)
    assert edges == [0, 200, 320] and tail == (41, 360, 40)
    first = A.bin_first_rels(edges, tail)
    assert first[:5] == [0, 200, 320, 360, 400] and len(first) == 44 and first[-1] == 360 + 40 * 40
    assert A.band_edges((50, 80), None, 10, 2, 8000.0) == ([0, 200, 320], None)
    assert A.band_edges((50, 80), 80, 10, 2, 8000.0) == ([0, 200, 320], None)      # nothing behind the early edges
    assert A.band_edges((50,), 60, 0.01, 1, 1000.0) == ([0, 50], (9, 51, 1))         # a tail bin is a capture at the least
    with pytest.raises(ValueError):
        A.bin_first_rels((0, 5), (3, 5, 2))                                          # the tail must begin behind the last edge


def test_canonical_routes_an_arrival_dict_with_bands(built_library):
    """simulation.arrival_plan_arguments answers for every dict it took before exactly as before and still refuses the new keys;
    arrival_bands_plan_arguments takes them: Butterworth sections at the rate of the captured series, the tail, the lags."""
    from wayverb_amd import decay as D
    from wayverb_amd import simulation as W

    class Mesh:
        dims, spacing, min_corner = (24, 20, 28), 0.05, (0.0, -0.5, 1.0)

    plain = dict(plane=1.55, every=2, threshold=1e-3)
    assert W.arrival_plan_arguments(plain, Mesh, 8000.0) == dict(edges=[0, 200, 320], threshold=1e-3, threshold_map=None, box=((0, 0, 11), (None, None, 1)),
                                                                 stride=1, first_step=0, period=2)
    for key, value in (("bands", [(100, 200)]), ("tail_ms", 500), ("tail_bin_ms", 10), ("lag", 0)):
        with pytest.raises(ValueError):
            W.arrival_plan_arguments(dict(plain, **{key: value}), Mesh, 8000.0)
    octaves = D.octave_band_edges([250.0, 500.0])
    plan = W.arrival_bands_plan_arguments(dict(plain, bands=octaves, tail_ms=500, tail_bin_ms=10), Mesh, 8000.0)
    assert sorted(plan) == ["bands", "box", "edges", "first_step", "lag", "period", "stride", "tail", "threshold", "threshold_map"]
    assert plan["edges"] == [0, 200, 320] and plan["tail"] == (41, 360, 40) and plan["period"] == 2 and plan["box"] == ((0, 0, 11), (None, None, 1))
    assert plan["bands"].shape == (2, 4, 5) and plan["bands"].tobytes() == np.stack([D.butterworth_bandpass(lo, hi, 4000.0) for lo, hi in octaves]).tobytes()
    assert plan["lag"] == [A.lag_captures(plan["bands"][k], c, 4000.0) for k, c in enumerate((250.0, 500.0))] and plan["lag"][0] > plan["lag"][1] > 0
    assert W.arrival_bands_plan_arguments(dict(plain, bands=octaves, lag=0), Mesh, 8000.0)["lag"] == [0, 0]
    for bad in (dict(plain, bands=[]), dict(plain, bands=[(200, 100)]), dict(plain, bands=octaves, lag="late"), dict(plain, bands=octaves, window=3),
                dict(bands=octaves, plane=1.55)):
        with pytest.raises(ValueError):
            W.arrival_bands_plan_arguments(bad, Mesh, 8000.0)

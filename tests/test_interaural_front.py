"""The Python front of the interaural plan, without a GPU: simulation.interaural_plan_arguments (valid dicts, every fault alone and
every ordered pair of two, the rounding of the ears and the warnings), what canonical hands on to the engine (a recording stand-in, as
tests/python_front_cases.py builds one), the refusal of slabs, where the plan stands in the tables, that test_python_front.py's fixture
is still met, and that no other plan's file names the new one."""
import json
import os
import re

import numpy as np

import python_front_cases as cases
from wayverb_amd import engine as E
from wayverb_amd import interaural as IA
from wayverb_amd import simulation as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")
MESH, Z, BOX = cases.MESH, cases.Z, cases.BOX      # dims (8, 9, 10), spacing 0.05, min corner z = 0.3; plane 4; a box
RATE = 8000.0
BASE = dict(threshold=1e-3, plane=Z)
KEYS_SENTENCE = ("interaural=dict(plane=<z in metres> or box=..., threshold=, every=, edges_ms=, ear_axis=, ear_distance=, ears=, max_lag_ms=, band_hz=, "
                 "threshold_map=, stride=, first_step=)")

FAULTS = dict(cases.PLANE_FAULTS, **cases.ONSET_FAULTS, **{
    "edges-not-from-0": cases.put(edges_ms=(5, 80)), "five-edges": cases.put(edges_ms=(0, 1, 2, 3, 4)), "no-edges": cases.put(edges_ms=()),
    "ears-and-axis": cases.put(ears=((0, -1, 0), (0, 1, 0)), ear_axis=(0, 1, 0)), "ears-and-distance": cases.put(ears=((0, -1, 0), (0, 1, 0)), ear_distance=0.2),
    "one-ear": cases.put(ears=((0, -1, 0),)), "ear-9-nodes": cases.put(ears=((0, -9, 0), (0, 1, 0))), "zero-axis": cases.put(ear_axis=(0, 0, 0)),
    "negative-distance": cases.put(ear_distance=-0.1), "distance-past-8-nodes": cases.put(ear_distance=1.0),
    "lag-negative": cases.put(max_lag_ms=-1.0), "lag-nan": cases.put(max_lag_ms=float("nan")),
    "band-reversed": cases.put(band_hz=(500.0, 100.0)), "band-of-one": cases.put(band_hz=(100.0,)), "band-from-0": cases.put(band_hz=(0.0, 100.0))})


def expected(plan):
    """The sentence a dict is refused with, by the order the function's docstring gives: keys and cadence first, then edges_ms, the ears,
    max_lag_ms, band_hz, the plane last; None for a valid dict."""
    if set(plan) - {"plane", "box"} - set(W.INTERAURAL_KEYS) or ("plane" in plan) == ("box" in plan) or "threshold" not in plan:
        return KEYS_SENTENCE
    if int(plan.get("every", 1)) < 1:
        return "interaural: every must be >= 1"
    edges = list(plan.get("edges_ms", (0, 80)))
    if not edges or edges[0] != 0 or len(edges) > 4:
        return "interaural: edges_ms begins with 0 and has 4 entries at the most"
    if plan.get("ears") is not None:
        if "ear_axis" in plan or "ear_distance" in plan:
            return "interaural: the ears are ears=((x, y, z), (x, y, z)) in mesh nodes, or ear_axis= and ear_distance= in metres"
        if len(plan["ears"]) != 2 or any(len(ear) != 3 or max(abs(v) for v in ear) > 8 for ear in plan["ears"]):
            return "interaural: ears holds two offsets (x, y, z) in mesh nodes, every component -8 .. 8"
    else:
        distance, axis = plan.get("ear_distance", 0.17), plan.get("ear_axis", (0, 1, 0))
        if not any(axis) or distance < 0:
            return "interaural: ear_axis is a non-zero vector and ear_distance >= 0 metres"
        if distance / MESH.spacing > 16.5:
            return "interaural: ear_distance=%g m is more than 8 mesh nodes (spacing %g m) from the seat" % (distance, MESH.spacing)
    if not plan.get("max_lag_ms", 1.0) >= 0:
        return "interaural: max_lag_ms must be >= 0"
    band = plan.get("band_hz")
    if band is not None and (len(band) != 2 or not 0 < band[0] < band[1]):
        return "interaural: band_hz is (lo_hz, hi_hz) with 0 < lo < hi, or None"
    if "plane" in plan and not 0 <= int(round((plan["plane"] - MESH.min_corner[2]) / MESH.spacing)) <= MESH.dims[2] - 1:
        return "interaural: plane z=%g m is outside the mesh" % plan["plane"]
    return None


def says(plan, rate=RATE):
    got = cases.answer(lambda: W.interaural_plan_arguments(dict(plan), MESH, rate))
    return got.get("says") if got.get("raises") == "ValueError" else got


def test_valid_dicts_become_the_arguments_of_set_interaural():
    got = W.interaural_plan_arguments(dict(BASE), MESH, RATE)
    assert sorted(got) == ["box", "ear_a", "ear_b", "edges", "first_step", "max_lag", "period", "sections", "stride", "threshold", "threshold_map"]
    assert got["edges"] == [0, 640] and (got["ear_a"], got["ear_b"]) == ((0, -1, 0), (0, 2, 0))            # 0.17 m at 0.05 m: 3 nodes along y
    assert (got["max_lag"], got["threshold"], got["sections"], got["period"], got["stride"], got["first_step"]) == (8, 1e-3, None, 1, 1, 0)
    assert got["box"] == ((0, 0, 4), (None, None, 1)) and got["threshold_map"] is None
    # lags and edges at the rate of the CAPTURED series
    for rate, every, ms, want in ((8000.0, 1, 1.0, 8), (8000.0, 2, 1.0, 4), (12000.0, 1, 1.0, 12), (12000.0, 3, 0.5, 2), (16000.0, 1, 1.0, 16), (8000.0, 1, 0.0, 0)):
        got = W.interaural_plan_arguments(dict(BASE, every=every, max_lag_ms=ms), MESH, rate)
        assert (got["max_lag"], got["period"], got["edges"]) == (want, every, [0, int(round(0.08 * rate / every))]), (rate, every, ms)
    got = W.interaural_plan_arguments(dict(threshold=0.5, box=BOX, ears=((-8, 0, 1), (8, 0, -1)), edges_ms=(0, 5, 80, 200), band_hz=(100.0, 400.0), every=2,
                                           stride=(1, 2, 1), first_step=7, threshold_map=cases.THRESHOLD_MAP), MESH, RATE)
    assert (got["ear_a"], got["ear_b"], got["edges"], got["box"], got["stride"], got["first_step"]) == ((-8, 0, 1), (8, 0, -1), [0, 20, 320, 800], BOX, (1, 2, 1), 7)
    assert got["sections"].shape == (4, 5) and got["sections"].tobytes() == IA.butterworth_bandpass(100.0, 400.0, RATE / 2).tobytes()
    assert got["threshold_map"] is cases.THRESHOLD_MAP
    # other axes; both ears on the seat
    assert W.interaural_plan_arguments(dict(BASE, ear_axis=(1, 0, 0), ear_distance=0.2), MESH, RATE)["ear_b"] == (2, 0, 0)
    got = W.interaural_plan_arguments(dict(BASE, ear_distance=0.0), MESH, RATE)
    assert got["ear_a"] == got["ear_b"] == (0, 0, 0)
    assert expected(BASE) is None


def test_the_warnings():
    """The ears more than a quarter off the distance asked for; more than 16 captures of lag."""
    got = cases.answer(lambda: W.interaural_plan_arguments(dict(BASE, ear_distance=0.07), MESH, RATE))              # 1.4 nodes -> 1: 0.05 m, 29 % off
    assert [w for w in got["warnings"]] == ["interaural: the ears are 0.05 m apart on this mesh (spacing 0.05 m), more than a quarter off the 0.07 m asked for"]
    assert "warnings" not in cases.answer(lambda: W.interaural_plan_arguments(dict(BASE, ear_distance=0.17), MESH, RATE))   # 0.15 m: 12 % off
    got = cases.answer(lambda: W.interaural_plan_arguments(dict(BASE, max_lag_ms=3.0), MESH, RATE))
    assert [w for w in got["warnings"]] == ["interaural: max_lag_ms=3 needs 24 captures at every=1, the engine holds 16: the lags end at 2 ms"]
    assert W.interaural_plan_arguments(dict(BASE, max_lag_ms=3.0, every=2), MESH, RATE)["max_lag"] == 12


def test_every_fault_alone_and_every_ordered_pair_of_faults():
    names = list(FAULTS)
    seen = set()
    for first in names:
        for second in names:
            plan = dict(BASE)
            for name in ([first] if first == second else [first, second]):
                FAULTS[name](plan)
            want = expected(plan)
            got = says(plan)
            if want is None:      # (two faults that undo each other)
                assert isinstance(got, dict) and "returns" in got, (first, second, got)
            else:
                assert got == want, (first, second, got, want)
                seen.add("the distance" if "more than 8 mesh nodes" in want else "the plane" if "plane z=" in want else want)
    assert len(names) == 22 and expected(BASE) is None
    for name in names:      # each fault alone IS refused
        plan = dict(BASE)
        FAULTS[name](plan)
        assert expected(plan) is not None, name
    assert len(seen) == 10      # keys, every, edges, ears and axis, the ears, the axis, the distance, the lag, the band, the plane


def test_plan_call_and_canonical_hand_the_arguments_on():
    vm, source, receiver = cases.box_scene(W)
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    plan = dict(threshold=1e-4, plane=5 * vm.mesh.spacing, every=2, ears=((0, -1, 0), (0, 1, 0)), max_lag_ms=0.5, edges_ms=(0, 2))
    name, positional, keywords = W.plan_call("interaural", plan, vm.mesh, rate, env, 0.01)
    assert (name, positional) == ("interaural", ()) and keywords == W.interaural_plan_arguments(plan, vm.mesh, rate)
    log = []

    def run_fast(eng, kind, index, signal, receivers, keep_going=None):
        log.append(["run_fast"])
        return signal.shape[0], np.zeros((signal.shape[0], 7))

    with cases.stand_ins(W.E, Engine=lambda *a, **k: cases.RecordingEngine(log, *a, **k), run_fast=run_fast):
        bands, taken = W.canonical(vm, source, receiver, env, 100.0, 0.6, 9.5 / rate, precision="f32", interaural=plan)
    assert taken == "what fetch_interaural returned" and len(bands) == 1
    assert [c[0] for c in log] == ["Engine", "set_interaural", "run_fast", "fetch_interaural", "close"]
    assert log[1] == ["set_interaural", [], cases.canon(keywords)]
    seen = {}

    def canonical(vm_, source_, receiver_, environment, cutoff, usable_portion, simulation_time, precision, device, **given):
        seen.update(given)
        return ["bands"], "what was taken"

    with cases.stand_ins(W, compute_voxels_and_mesh=lambda *a, **k: vm, canonical=canonical), cases.stand_ins(W.P, postprocess=lambda *a, **k: "audio"):
        got = W.impulse_response(None, None, None, source, receiver, interaural=plan)
    assert seen == dict(interaural=plan) and len(got) == 4 and got[3] == "what was taken"


def test_slabs_are_refused_and_every_earlier_keyword_answers_first():
    def slabbed(**plans):
        return cases.answer(lambda: W.canonical(None, None, None, None, 100.0, 0.6, 0.01, slabs=2, **plans))
    assert slabbed(interaural={}) == {"raises": "ValueError", "says": "interaural maps are accumulated on one domain only (slabs=1)"}
    for keyword in cases.PLAN_KEYWORDS + ("waterfall",):
        assert slabbed(**{keyword: {}, "interaural": {}}) == slabbed(**{keyword: {}}) != slabbed(interaural={})


def test_where_the_plan_stands_in_the_tables():
    """The new plan is the last of every table that may grow.  tests/test_waterfall_plan.py and tests/test_waterfall_front.py pin
    E.PLAN_NAMES, E._PLAN_CALLS, W.PLANS and W.SLABS_REFUSALS with the waterfall plan as their LAST entry (and the latter two entry by
    entry), so in the two of the engine's the new plan stands just ahead of it, and in the front it is the last of ALL_PLANS and
    ALL_SLABS_REFUSALS, which hold the pinned tables unchanged at their head and are what canonical and plan_call look in."""
    assert E.PLAN_NAMES[-2:] == ("interaural", "waterfall") and list(E._PLAN_CALLS)[-2:] == ["interaural", "waterfall"]
    assert W.ALL_PLANS[:len(W.PLANS)] == W.PLANS and [k for k, _ in W.ALL_PLANS[len(W.PLANS):]] == ["interaural"]
    assert list(W.ALL_SLABS_REFUSALS)[:len(W.SLABS_REFUSALS)] == list(W.SLABS_REFUSALS) and list(W.ALL_SLABS_REFUSALS)[-1] == "interaural"
    for name in ("wv_set_interaural", "wv_interaural_count", "wv_fetch_interaural"):
        assert name in E.EXPORTS
    for method in ("set_interaural", "interaural_count", "fetch_interaural"):
        assert callable(getattr(E.Engine, method)) and getattr(E.Engine, method).__doc__
    assert C_sizeof() == 112 and (E.Engine.QUERY_INTERAURAL_CAPTURES, E.Engine.QUERY_INTERAURAL_FOLDS, E.Engine.QUERY_INTERAURAL_NS) == (54, 55, 56)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    assert "WV_QUERY_INTERAURAL_CAPTURES = 54, WV_QUERY_INTERAURAL_FOLDS = 55, WV_QUERY_INTERAURAL_NS = 56" in header


def C_sizeof():
    import ctypes
    plan = E.WvInterauralPlan
    assert (plan.first_step.offset, plan.period.offset, plan.ear_a.offset, plan.ear_b.offset, plan.max_lag.offset, plan.n_bins.offset, plan.threshold.offset,
            plan.edges.offset, plan.n_sections.offset) == (40, 48, 56, 68, 80, 84, 88, 92, 108)
    return ctypes.sizeof(plan)


def test_the_python_front_fixture_is_still_met():
    """tests/golden/python_front.json, recorded before this plan: a fresh engine's plan attributes are the names it holds -- the new
    shape is a default of the class -- and every recorded answer of the argument functions is still given (tests/test_python_front.py
    asserts all of it; this is the part the new plan could have moved)."""
    fixture = cases.unpack(json.load(open(os.path.join(ROOT, "tests", "golden", "python_front.json"))))
    eng = cases.stand_in_engine(E)
    assert "interaural_shape" not in vars(eng) and eng.interaural_shape is None and E.Engine.interaural_shape is None
    recorded = [group for group in fixture if "plan state" in group]
    assert recorded, sorted(fixture)
    for name in E.PLAN_NAMES:
        assert getattr(eng, name + "_shape") is None


def test_the_other_plans_files_do_not_name_the_new_one():
    """The plan's own files, and of the shared ones exactly those DESIGN.md 4.15 lists (and engine_snapshot.hip.h, where the third kind
    of capture is launched beside the other two)."""
    own = {"interaural_plan.h", "interaural_kernels.hip.h", "engine_interaural.hip.h"}
    shared = {"engine.hip.h", "engine_staged.hip.h", "engine_batch.hip.h", "engine_slab.hip.h", "engine_base.h", "engine.hip", "engine_snapshot.hip.h"}
    naming = {f for f in os.listdir(CSRC) if re.search(r"interaural|ear_gather", open(os.path.join(CSRC, f), errors="replace").read(), flags=re.I)
              and f.endswith((".h", ".hip", ".cpp"))}
    assert naming == own | shared, sorted(naming ^ (own | shared))
    from wayverb_amd import build as B
    assert own <= set(B.HEADERS)      # (a change of any of them makes the library stale)
    kernels = open(os.path.join(CSRC, "interaural_kernels.hip.h")).read().split("#pragma once")[1]
    assert "__shared__" not in kernels and "atomic" not in kernels
    staged = open(os.path.join(CSRC, "engine_staged.hip.h")).read()
    assert staged.count("launch_ear_gather(") == 1 and staged.count("launch_intensity_gather(") == 1 and staged.count("launch_snapshot_gather(") == 1


def test_the_resource_report_shows_no_scratch_and_no_lds():
    """profiles/r23/interaural_kernel_resources.txt, the compiler's report for gfx950: every instance of both kernels."""
    text = open(os.path.join(ROOT, "profiles", "r23", "interaural_kernel_resources.txt")).read()
    rows = re.findall(r"^(interaural_fold_kernel<\d+, \d+>|ear_gather_kernel<\w+>)\s+VGPRs\s+(\d+)\s+AGPRs\s+(\d+)\s+scratch\s+(\d+)\s+LDS\s+(\d+)", text, flags=re.M)
    assert len(rows) == 10 and {r[0] for r in rows} >= {"interaural_fold_kernel<4, 16>", "interaural_fold_kernel<0, 0>", "ear_gather_kernel<float>", "ear_gather_kernel<double>"}
    for name, vgprs, agprs, scratch, lds in rows:
        assert int(scratch) == 0 and int(lds) == 0 and int(vgprs) + int(agprs) <= 512, name

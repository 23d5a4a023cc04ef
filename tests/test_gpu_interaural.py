"""Interaural maps: per node of a box the energies and lagged products of the field at two nodes an ear-distance apart, binned from the
node's own onset, accumulated on the device while wv_run keeps going (wv_set_interaural; csrc/interaural_kernels.hip.h,
engine_interaural.hip.h).  The reference of every comparison is a second, identical engine with a SNAPSHOT plan of the whole mesh at
the same cadence, from whose snapshots the two ear planes are cut and go through interaural.interaural_fold -- the definition.
Equality is BYTEWISE, and every comparison also asserts that it is not one of zeros.  Small meshes, forms forced, a few dozen steps."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import interaural_twin as T
import plan_argument_faults as F
import plan_twin as P
from helpers import set_tuning
from plan_cases import (ALL_FORMS, FILE_COUNTS, FILE_FORMS, box_scene, capture_counts, changes_nothing, check, default_tuning_afterwards, ear_level,
                        ear_map, ears_on_the_mesh, levels, make_engine, plan_on, reference_snapshots)
from test_gpu_plan_refusals import BANDS, SET, STOP, refusal
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import interaural as IA
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECTIONS = D.butterworth_bandpass(500.0, 2000.0, 8000.0)                # four sections; [:1] is a cascade of one
EDGES = {1: [0], 4: [0, 3, 8, 20]}
SEAT = dict(box=((3, 2, 4), (10, 9, 7)), ear_a=(0, -2, 0), ear_b=(0, 2, 0))      # B = 630 on the 24 x 20 x 28 room


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def ear_planes(snaps, dims, box, stride, ear):
    """The plane of one ear cut from snapshots of the whole mesh float32[n, nz, ny, nx]: every taken node's, `ear` mesh nodes away."""
    origin, extent = box
    stride = (stride,) * 3 if np.isscalar(stride) else tuple(stride)
    cut = []
    for axis in range(3):
        ext = dims[axis] - origin[axis] if extent[axis] is None else extent[axis]
        first = origin[axis] + ear[axis]
        assert first >= 0 and first + ext - 1 - (ext - 1) % stride[axis] < dims[axis]
        cut.append(slice(first, first + ext, stride[axis]))
    return np.ascontiguousarray(snaps[:, cut[2], cut[1], cut[0]])


def reference(case_name, tag, form, n_steps, period, box, ear_a, ear_b, stride=1, first_step=0):
    # (one launch per step is a form of single steps that the snapshot tests' table does not list: its reference is theirs)
    snaps, steps = reference_snapshots(case_name, tag, "single" if form == "whole" else form, dict(box="mesh", period=period, first_step=first_step), n_steps)
    dims = cases.CASES[case_name]()["mesh"].dims
    return ear_planes(snaps, dims, box, stride, ear_a), ear_planes(snaps, dims, box, stride, ear_b), steps


THRESHOLDS = dict(zero=dict(threshold=0.0), scalar=dict(threshold=ear_level), map=dict(threshold=0.0, threshold_map=ear_map))


def check_seats(case_name, tag, form, n_steps, period, box, ear_a, ear_b, L, edges, sections, threshold="scalar", stride=1, query=None):
    """The shared check of an interaural plan whose threshold is made of the input (plan_cases.levels), and what this kind adds: both
    ears hear something at the end, and a map leaves a node that never reaches its threshold."""
    plan = plan_on(case_name, "interaural", box=box, stride=stride, period=period, edges=list(edges), ear_a=tuple(ear_a), ear_b=tuple(ear_b), max_lag=L,
                   sections=sections, **THRESHOLDS[threshold])
    got, want, plan, snaps, _ = check("interaural", case_name, tag, form, plan, n_steps, query)
    a, b = ears_on_the_mesh(plan, snaps)
    assert np.abs(a[-1]).max() > 0 and np.abs(b[-1]).max() > 0
    if threshold == "map" and a[0].size > 8:
        assert (got["onset"] == IA.NONE).any() and (got["onset"] != IA.NONE).any()       # a node that never reaches its threshold
    return got, want


def same(got, want, what=""):
    for key in ("onset", "pre", "bins"):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (what, key)
        assert got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), (what, key)


GRID = [(L, n_bins, S) for L in (0, 1, 5, 16) for n_bins in (1, 4) for S in (0, 1, 4)]


@pytest.mark.parametrize("L,n_bins,S", GRID, ids=["L%d-bins%d-S%d" % g for g in GRID])
def test_lags_bins_and_sections_against_the_definition(L, n_bins, S):
    """Every lag class, one and four bins, no filter, one section and four; 33 captures (two full stages and one for the fetch: the
    history carried across folds, bin edges inside and between folds); fp32 and fp64 and the three kinds of threshold in turn."""
    k = GRID.index((L, n_bins, S))
    check_seats("random", ("f32", "f64")[k % 2], "pair", 32, 1, SEAT["box"], SEAT["ear_a"], SEAT["ear_b"], L, EDGES[n_bins], SECTIONS[:S] if S else None,
          ("zero", "scalar", "map")[k % 3])


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("threshold", ["zero", "scalar", "map"])
def test_thresholds_in_both_precisions(tag, threshold):
    check_seats("random", tag, "triple", 32, 1, SEAT["box"], SEAT["ear_a"], SEAT["ear_b"], 5, EDGES[4], SECTIONS[:2], threshold)


PLACES = {
    "plane-ears-8-along-x": dict(box=((8, 0, 14), (8, None, 1)), ear_a=(-8, 0, 0), ear_b=(8, 0, 0)),
    "strided-box-every-ear-at-its-limit": dict(box=((8, 8, 9), (8, 4, 10)), stride=(2, 1, 3), ear_a=(-8, -8, -8), ear_b=(8, 8, 8)),
    "one-node-negative-and-mixed-ears": dict(box=((5, 6, 7), (1, 1, 1)), ear_a=(-3, 2, -1), ear_b=(1, -2, 0)),
    "odd-B-567": dict(box=((3, 2, 4), (9, 9, 7)), ear_a=(1, 0, -2), ear_b=(-1, 0, 2)),
    "ears-on-the-mesh-faces": dict(box=((0, 2, 0), (None, 16, None)), stride=(3, 5, 9), ear_a=(0, -2, 0), ear_b=(0, 2, 0)),
    "equal-ears": dict(box=((3, 2, 4), (10, 9, 7)), ear_a=(2, 1, -1), ear_b=(2, 1, -1)),
}


@pytest.mark.parametrize("name", sorted(PLACES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_strides_and_ear_offsets_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; 21 captures."""
    place = PLACES[name]
    got, _ = check_seats("random", tag, "triple", 20, 1, place["box"], place["ear_a"], place["ear_b"], 5, EDGES[4], SECTIONS[:1], "map", place.get("stride", 1))
    if name == "equal-ears":                 # the autocorrelation form: symmetric in the lag, and the energies are C[0]
        bins = got["bins"]
        assert bins[:, 0].tobytes() == bins[:, 1].tobytes() == bins[:, 2 + 5].tobytes()
        for l in range(1, 6):
            assert bins[:, 2 + 5 + l].tobytes() == bins[:, 2 + 5 - l].tobytes()


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_equal_ears_on_the_node_no_lag_no_filter_is_the_arrival_plan(tag):
    """ear_a == ear_b == 0, L = 0, no sections: Ea (and Eb, and C[0]), pre[0] and onset are the arrival plan's E, pre and onset of the
    same box, edges and threshold -- code that was there before this plan -- bit for bit."""
    a, _, _ = reference("random", tag, "pair", 32, 1, SEAT["box"], (0, 0, 0), (0, 0, 0))
    scalar, tmap = levels(a, a)
    for thr, m in ((scalar, None), (0.0, tmap)):
        set_tuning(**ALL_FORMS["pair"])
        engines = [make_engine(cases.CASES["random"](), tag) for _ in range(2)]
        try:
            engines[0].set_interaural(EDGES[4], (0, 0, 0), (0, 0, 0), 0, thr, None, box=SEAT["box"], threshold_map=m)
            engines[1].set_arrival(EDGES[4], thr, box=SEAT["box"], threshold_map=m)
            for e in engines:
                assert e.run_steps(32) == (32, 0)
            got, count = engines[0].fetch_interaural()
            arrival, arrival_count = engines[1].fetch_arrival()
        finally:
            for e in engines:
                e.close()
        assert count == arrival_count == 33
        assert got["onset"].tobytes() == arrival["onset"].tobytes() and got["pre"][0].tobytes() == got["pre"][1].tobytes() == arrival["pre"].tobytes()
        for plane in range(3):
            assert np.ascontiguousarray(got["bins"][:, plane]).tobytes() == arrival["bins"].tobytes(), plane
        assert np.abs(arrival["bins"]).max() > 0 and (arrival["onset"] != IA.NONE).any()


def test_the_early_iacf_peaks_at_the_travel_time_between_the_ears():
    """A 48^3 fp32 box, a smooth pulse from a hard source at the centre, seats on the x axis through it.  With the ears two nodes apart
    ON that axis the early IACF peaks at the lag the wave takes from one ear to the other: 2 sqrt 3 = 3.46 captures at the mesh's speed
    of 1 / sqrt 3 nodes per step, so round(2 sqrt 3) = 3 within one capture -- positive, ear a being the nearer one.  With the ear axis
    PERPENDICULAR to the source's direction both ears hear the same: the peak is at lag 0."""
    set_tuning()
    mesh = M.box_mesh(48, 48, 48)
    t = np.arange(72, dtype=np.float64)              # (a run ends with its source signal)
    sig = np.exp(-0.5 * ((t - 12.0) / 3.0) ** 2)
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(24, 24, 24), signal=sig, recv=[mesh.compute_index(30, 24, 24)])
    seats = dict(box=((30, 24, 24), (8, 1, 1)))        # x = 30 .. 37, six to thirteen nodes from the source
    lags = {}
    for name, ear_a, ear_b in (("along", (-1, 0, 0), (1, 0, 0)), ("across", (0, -1, 0), (0, 1, 0))):
        eng = make_engine(case, "f32")
        try:
            eng.set_interaural([0, 40], ear_a, ear_b, 8, 1e-4, None, **seats)
            assert eng.run_steps(70) == (70, 0)
            got, count = eng.fetch_interaural()
        finally:
            eng.close()
        assert count == 71 and (got["onset"] != IA.NONE).all()
        lags[name] = IA.iacc_lag(got["bins"], 0, interpolate=False).reshape(-1)
        peak = IA.iacc(got["bins"], 0, interpolate=False).reshape(-1)
        print(name, "lags", lags[name].tolist(), "iacc", peak.tolist())
        assert (peak > 0.5).all()
    want = int(round(2.0 * np.sqrt(3.0)))
    assert want == 3 and (np.abs(lags["along"] - want) <= 1).all()
    assert (lags["across"] == 0).all()


# ---- the stepping forms --------------------------------------------------------------------------------------------------------------------

FORM_CASES = [("single", 1), ("single", 5), ("whole", 1), ("whole", 3), ("graph", 16), ("graph", 1), ("pair", 2), ("pair", 3), ("triple", 3), ("triple", 4), ("triple", 7)]


@pytest.mark.parametrize("form,period", FORM_CASES, ids=["%s-every%d" % c for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_same_bytes(form, period, tag):
    """Single steps, one launch per step, graph replay, two- and three-step passes, periods that do and do not divide 2 and 3: the
    bytes are those of the definition fed from a snapshot run in the SAME form (one launch per step: in single steps, the form it is a
    variant of) -- and those of single steps."""
    n_steps = 64 if form == "graph" and period == 16 else 30
    query = {"pair": E.Engine.QUERY_PASSES, "triple": E.Engine.QUERY_TRIPLE_PASSES}.get(form)
    got, _ = check_seats("random", tag, form, n_steps, period, SEAT["box"], SEAT["ear_a"], SEAT["ear_b"], 5, EDGES[4], SECTIONS[:1], "zero", query=query)
    a, b, steps = reference("random", tag, "single", n_steps, period, SEAT["box"], SEAT["ear_a"], SEAT["ear_b"])
    same(got, IA.interaural_fold(a, b, 0.0, EDGES[4], 5, SECTIONS[:1]), (form, period, tag))


# ---- refusals: the 12 x 10 x 9 fp32 box mesh of tests/plan_argument_faults.py, no stepping ------------------------------------------

INVALID = -1


def one_section(entry=None, value=None, n=1):
    s = np.zeros((n, 5))
    s[:, 0] = 1.0
    if entry is not None:
        s.reshape(-1)[entry] = value
    return s


IA_BASE = dict(F.BOX, n_bins=3, threshold=1e-3, edges=[0, 4, 9], map=None, ear_a=[-1, 0, 0], ear_b=[1, 0, 0], max_lag=3, n_sections=1, sections=one_section())
IA_FAULTS = dict(F.SHARED, **F.ONSET, **{
    "n_bins 0": F.put(n_bins=0), "n_bins 5": F.put(n_bins=5), "max_lag 17": F.put(max_lag=17), "ear 9": F.put(ear_b=[1, 0, 9]), "ear -9": F.put(ear_a=[-1, -9, 0]),
    "n_sections 5": F.put(n_sections=5, sections=one_section(n=5)), "coef inf": F.put(sections=one_section(3, F.INF)), "coef NaN": F.put(sections=one_section(0, F.NAN)),
    "sections NULL": F.put(sections=None), "ear off -x": F.put(x0=0), "ear off +x": F.put(x0=8), "ear off +z": F.put(ear_b=[1, 0, 7])})


def expected_refusal(a):
    """[code, sentence] by the order the contract sets for wv_set_interaural's checks, restated; None for a plan that is taken."""
    def says(text):
        return [INVALID, text if text == "null argument" else "wv_set_interaural: " + text]
    if not 1 <= a["n_bins"] <= 4:
        return says("n_bins must be 1 .. 4")
    edges = a["edges"][:a["n_bins"]]
    if edges[0] != 0 or any(y <= x for x, y in zip(edges, edges[1:])):
        return says("edges[0] must be 0 and the edges strictly increasing")
    if not (a["threshold"] >= 0 and np.isfinite(a["threshold"])):
        return says("the threshold must be >= 0 and finite")
    if not 0 <= a["max_lag"] <= 16:
        return says("max_lag must be 0 .. 16")
    if any(not -8 <= v <= 8 for v in list(a["ear_a"]) + list(a["ear_b"])):
        return says("every component of an ear offset must be -8 .. 8")
    if not 0 <= a["n_sections"] <= 4:
        return says("n_sections must be 0 .. 4")
    if a["n_sections"] and a["sections"] is None:
        return says("null argument")
    if a["n_sections"] and not np.isfinite(a["sections"][:a["n_sections"]]).all():
        return says("every coefficient must be finite")
    if min(a["sx"], a["sy"], a["sz"]) < 1:
        return says("strides must be >= 1")
    if a["period"] < 1:
        return says("period must be >= 1")
    axes = list(zip((a["x0"], a["y0"], a["z0"]), (a["nx"], a["ny"], a["nz"]), (a["sx"], a["sy"], a["sz"]), F.MESH))
    for o, n, s, d in axes:
        if n < 1 or o < 0 or o + (n - 1) * s >= d:
            return says("the box leaves the mesh")
    for ear in (a["ear_a"], a["ear_b"]):
        for (o, n, s, d), e in zip(axes, ear):
            if o + e < 0 or o + (n - 1) * s + e >= d:
                return says("an ear leaves the mesh")
    if a["map"] is not None and not (np.isfinite(a["map"]) & (a["map"] >= 0)).all():
        return says("every entry of the threshold map must be >= 0 and finite")
    return None


def call_setter(eng, args):
    plan = E.WvInterauralPlan()
    for name, _ in plan._fields_:
        if name in ("edges", "ear_a", "ear_b"):
            for k, v in enumerate(args[name]):
                getattr(plan, name)[k] = v
        elif name in args:
            setattr(plan, name, args[name])
    sections = None if args["sections"] is None else np.ascontiguousarray(args["sections"], dtype=np.float64)
    tmap = None if args["map"] is None else np.ascontiguousarray(args["map"], dtype=np.float32)
    rc = eng.lib.wv_set_interaural(eng.h, C.byref(plan), F.pointer(sections), F.pointer(tmap))
    return None if rc == 0 else [rc, eng.lib.wv_last_error().decode()]


@pytest.fixture(scope="module")
def fault_engine(built_library):
    eng = F.make_engine()
    yield eng
    eng.close()


SET_INTERAURAL = lambda e: e.set_interaural((0, 4, 9), (-1, 0, 0), (1, 0, 0), 3, 1e-3, one_section(), box=((1, 1, 1), (4, 3, 2)))       # noqa: E731


def test_every_argument_fault_and_every_ordered_pair_with_code_and_sentence(fault_engine):
    """Every single fault and every ordered pair of two (the second wins where both touch one argument): the code and the WHOLE
    sentence, by the precedence the checks have; the engine is untouched by every refused call, and an earlier plan's state is."""
    eng = fault_engine
    assert SET_INTERAURAL(eng) == (3, 9, 2, 3, 4)
    assert eng.run_steps(3) == (3, 0)
    kept, kept_count = eng.fetch_interaural()
    before = F.state(eng)
    said = set()
    names = list(IA_FAULTS)
    for first in names:
        for second in names:
            args = dict(IA_BASE)
            for name in ([first] if first == second else [first, second]):
                IA_FAULTS[name](args)
            want = expected_refusal(args)
            got = call_setter(eng, args)
            assert got == want, (first, second, got, want)
            if want is None:            # (two faults that undo each other: x0 = 0 with the ear moved by another fault ...) the plan was taken
                call_setter(eng, IA_BASE)
                raise AssertionError("no two of these faults undo each other: %s, %s" % (first, second))
            said.add(want[1])
            assert F.state(eng) == before, (first, second)
        again, count = eng.fetch_interaural()
        assert count == kept_count == 4, first
        same(again, kept, first)
    assert np.abs(kept["bins"]).max() + np.abs(kept["pre"]).max() > 0 and len(names) == 32 and expected_refusal(dict(IA_BASE)) is None
    for name in names:
        args = dict(IA_BASE)
        IA_FAULTS[name](args)
        assert expected_refusal(args) is not None, name
    assert len(said) == 13       # every sentence the setter has for an argument was said
    eng.set_interaural(None)


TEN = dict(SET, modulation=lambda e: e.set_modulation([0.0, 0.125], BANDS, box=((1, 1, 1), (4, 3, 2))),
           arrival_bands=lambda e: e.set_arrival_bands((0, 4), BANDS, 1e-3, box=((1, 1, 1), (4, 3, 2))),
           waterfall=lambda e: e.set_waterfall([0.0, 0.125], 3, 2, box=((1, 1, 1), (4, 3, 2))))
TEN_STOP = dict(STOP, modulation=lambda e: e.set_modulation(None, None), arrival_bands=lambda e: e.set_arrival_bands(None, None),
                waterfall=lambda e: e.set_waterfall(None, None, None))
ACTIVE = {
    "snapshots": ("wv_set_snapshots", "a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)"),
    "spectrum": ("wv_set_spectrum", "a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)"),
    "decay": ("wv_set_decay", "a decay plan is active (wv_set_decay(e, NULL) stops it)"),
    "decay_bands": ("wv_set_decay_bands", "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)"),
    "intensity": ("wv_set_intensity", "an intensity plan is active (wv_set_intensity(e, NULL) stops it)"),
    "arrival": ("wv_set_arrival", "an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it)"),
    "lateral": ("wv_set_lateral", "a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it)"),
    "modulation": ("wv_set_modulation", "a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it)"),
    "arrival_bands": ("wv_set_arrival_bands", "a banded arrival plan is active (wv_set_arrival_bands(e, NULL, NULL, NULL, 0, 0) stops it)"),
    "waterfall": ("wv_set_waterfall", "a waterfall plan is active (wv_set_waterfall(e, NULL, NULL) stops it)"),
}
TAIL = "; the plans exclude each other"


def test_the_plan_excludes_each_of_the_ten_others_in_both_directions(fault_engine):
    """Under an interaural plan every existing setter says the new row's sentence; under each existing plan the new setter says that
    plan's row.  WV_E_STATE throughout, and the refused call changes nothing: the active plan is still the one its count answers for."""
    eng = fault_engine
    assert sorted(TEN) == sorted(ACTIVE) and TAIL == P.TAIL
    SET_INTERAURAL(eng)
    for kind, setter in TEN.items():
        assert refusal(setter, eng) == [-6, ACTIVE[kind][0] + ": an interaural plan is active (wv_set_interaural(e, NULL, NULL, NULL) stops it)" + TAIL], kind
        assert eng.interaural_count() == (0, 0)
    eng.set_interaural(None)
    for kind, setter in TEN.items():
        setter(eng)
        assert refusal(SET_INTERAURAL, eng) == [-6, "wv_set_interaural: " + ACTIVE[kind][1] + TAIL], kind
        assert refusal(lambda e: e.interaural_count(), eng) == [-6, "wv_interaural_count: no interaural plan is set"]
        TEN_STOP[kind](eng)
        SET_INTERAURAL(eng)      # with the plan stopped the setter that was refused goes through
        eng.set_interaural(None)
    eng.checkpoint()
    SET_INTERAURAL(eng)
    code, text = refusal(lambda e: e.rollback(), eng)
    assert code == -6 and "interaural plan was set after the checkpoint" in text and "its state has" in text
    eng.set_interaural(None)
    eng.rollback()
    eng.drop_checkpoint()


def test_a_slab_of_a_chain_and_a_group_refuse():
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    set_plan = lambda e: e.set_interaural([0], (-1, 0, 0), (1, 0, 0), 2, box=((1, 0, 0), (4, 4, 1)))       # noqa: E731
    assert refusal(set_plan, slab) == [-6, "wv_set_interaural: not on a slab of a chain (one domain only)"]
    slab.close()
    eng = E.Engine(mesh, precision="f32")
    group = E.LocalSlabGroup([eng])
    set_plan(eng)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_run_group accumulates no interaural maps: .*\(wv_set_interaural\(e, NULL, NULL, NULL\) stops the plan\)"):
        group.run_steps(4)
    eng.set_interaural(None)
    assert group.run_steps(4) == (4, 0)
    group.close()


# ---- the family's scripts, replayed -----------------------------------------------------------------------------------------------------

MODES = {"default": {}, "three-step-passes": dict(pair=1, triple=1), "single-steps": dict(pair=0)}
_script = {}


@pytest.fixture(scope="module", autouse=True)
def interaural_family():
    with T.registered():
        yield


@pytest.mark.parametrize("seed", range(T.SEEDS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_random_plan_sequence(oracle, interaural_family, seed, mode):
    """The eight scripts tests/test_interaural_twin.py holds to what the comparison needs, through plan_twin.replay: after every call
    both fields, at every fetch, handover, stop and the end every output of the plan, bytewise."""
    if seed not in _script:
        _script[seed] = P.build_script(oracle, T.FAMILY, seed)
    script = _script[seed]
    set_tuning(**MODES[mode])
    eng = E.Engine(script["mesh"], precision=script["tag"], all_tiles=False)
    try:
        P.replay(eng, script)
    finally:
        eng.close()


# ---- the Python front and the tools -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("captures", FILE_COUNTS["interaural"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("interaural", captures)


@pytest.mark.parametrize("form", FILE_FORMS["interaural"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("interaural", tag, form)


def test_canonical_returns_the_maps_beside_the_receiver_output():
    """simulation.canonical(..., interaural=...): the records are those of a run without a plan, the maps are the definition's over
    canonical's own snapshots of the same plane and cadence; a second plan beside it is refused with the engine's message."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=dict(box=((0, 0, 12), (None, None, 1)), period=2))
    plan = dict(box=((0, 2, 12), (None, 20, 1)), every=2, threshold=1e-6, edges_ms=(0.0, 8e3 / rate), ears=((0, -2, 0), (0, 2, 0)), max_lag_ms=6e3 / rate)
    bands, (maps, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", interaural=plan)
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 21 and maps["bins"].shape == (2, 9, 1, 20, 24)          # edges [0, 4], L = 3
    want = IA.interaural_fold(np.ascontiguousarray(fields[:, :, 0:20]), np.ascontiguousarray(fields[:, :, 4:24]), 1e-6, [0, 4], 3)
    same(maps, want, "canonical")
    assert np.abs(maps["bins"]).max() > 0 and IA.iacc(maps["bins"]).shape == (1, 20, 24)
    with pytest.raises(E.WaveguideError, match="error -6: wv_set_interaural: a decay plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, decay=dict(n_bins=2, bin_captures=2), interaural=plan)
    with pytest.raises(ValueError, match="interaural maps are accumulated on one domain only"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, interaural=plan)


def test_the_tool_writes_the_iacc_maps_of_one_plane(tmp_path):
    """tools/interaural_map.py on a 24^3 room: IACC_E / IACC_L / IACC_A, their lags and the bins of one plane less the ears' rim."""
    out = tmp_path / "interaural.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "interaural_map.py"), "--room", "24", "--seconds", "0.05", "--precision", "f32",
                        "--plane", "z=1.5", "--early-ms", "10", "--band", "40,160", "--out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        bins, onset, a, b, L = f["bins"], f["onset"], f["ear_a"], f["ear_b"], int(f["max_lag"])
        maps = {k: f[k] for k in ("iacc_e", "iacc_l", "iacc_a", "lag_e_ms", "lag_l_ms", "lag_a_ms")}
        rate, edges, captures = float(f["sample_rate"]), f["edges"], int(f["captures"])
    ny = 24 - int(max(0, -a[1], -b[1])) - int(max(0, a[1], b[1]))
    assert "wrote" in p.stdout and bins.shape == (2, 2 * L + 3, ny, 24) and onset.shape == (ny, 24) and 1 <= L <= 16
    assert list(edges) == [0, int(round(0.010 * rate))] and captures == int(np.ceil(rate * 0.05)) + 1
    assert all(m.shape == (ny, 24) for m in maps.values()) and np.abs(bins).max() > 0
    heard = np.isfinite(maps["iacc_a"])
    assert heard.any() and (maps["iacc_a"][heard] > 0).all() and (maps["iacc_a"][heard] <= 1.0 + 1e-3).all()
    assert (np.abs(maps["lag_a_ms"][heard]) <= (L + 0.5) * 1e3 / rate).all()


def test_the_rate_tool_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/interaural_rate.py --side 64 --steps 48: every row is there and the maps of the snapshot-and-twin way equal the plan's
    bytewise in all eight cases."""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "interaural_rate.py"), "--side", "64", "--steps", "48",
                        "--repeats", "1", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 8, p.stdout
    report = json.load(open(str(out)))
    assert len(report["cases"]) == 8 and all(c["bytewise_equal"] and c["not_zeros"] for c in report["cases"].values())
    assert all(set(c["steps_per_second"]) == {"no plan", "snapshots + numpy", "interaural plan"} for c in report["cases"].values())

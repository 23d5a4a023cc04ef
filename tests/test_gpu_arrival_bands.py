"""Band-limited arrival maps: per octave band, energy binned from each node's own broadband onset less the band's lag, explicit bins and a
uniform tail, accumulated on the device while wv_run keeps going (wv_set_arrival_bands; csrc/arrival_bands_kernels.hip.h,
engine_arrival_bands.hip.h).  The reference of every comparison is a second, identical engine with a SNAPSHOT plan of the same box and
cadence, whose snapshots arrival.banded_arrival_fold -- the definition in NumPy -- folds in capture order; the two cross-plan
identities are held against wv_set_arrival and wv_set_decay_bands on the device.  Equality is BYTEWISE on all six outputs; the filter
states show in every capture that follows.  Small meshes, forms forced, a few dozen steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import set_tuning
from test_arrival_bands_host import IDENTITY, random_sections
from test_gpu_decay import BOXES, reference_snapshots
from test_gpu_plan_refusals import CONSTANTS, refusal
from test_gpu_plan_refusals import SET as SET7
from test_gpu_plan_refusals import STOP as STOP7
from test_gpu_snapshots import FORMS, make_engine
from wayverb_amd import arrival as A
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "arrival_bands_refusals.json")
EDGES = (0, 1, 5, 16, 17)
TAIL_W3 = (4, 19, 3)          # begins inside the second fold for an onset at capture 0; its last bin is open-ended from rel 28 on
PLANE = dict(box=((0, 0, 15), (None, None, 1)))      # of the 32^3 impulse room


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


def threshold_of(snaps):
    """The median, over the box's nodes, of the snapshots' per-node max |p|, so that lanes of one wave sit in different bins; where
    that is 0 (an impulse seen at an even period: more than half of the nodes never move) the lower quartile of the non-zero maxima."""
    highest = np.abs(snaps).max(axis=0)
    median = np.float32(np.median(highest))
    return median if median > 0 or not (highest > 0).any() else np.float32(np.quantile(highest[highest > 0], 0.25))


def bands_engine(case_name, tag, form, plan, edges, sections, threshold, **more):
    set_tuning(**FORMS[form])
    eng = make_engine(cases.CASES[case_name](), tag)
    shape = eng.set_arrival_bands(edges, sections, threshold, **dict(more, **plan))
    return eng, shape


def same(got, want):
    for key in A.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), "%s differs at %d places" % (key, (got[key] != want[key]).sum())


def check(case_name, tag, form, plan, edges, sections, n_steps, tail=None, lag=0, threshold=None, map_factors=None, query=None, spread=True):
    snaps, steps = reference_snapshots(case_name, tag, form, plan, n_steps)
    thr = threshold_of(snaps) if threshold is None else np.float32(threshold)
    threshold_map = None if map_factors is None else (thr * map_factors(snaps.shape[1:])).astype(np.float32)
    want = A.banded_arrival_fold(snaps, thr if threshold_map is None else threshold_map, edges, sections, tail=tail, lag=lag)
    if spread:      # what the reference alone must show before a comparison means anything
        heard = want["onset"] != A.NONE
        assert heard.any() and (~heard).any() and len(set(want["onset"][heard].tolist())) >= 3
        assert (want["bins"].reshape(want["bins"].shape[:2] + (-1,)).max(axis=2) > 0).sum(axis=1).min() >= 2
    eng, shape = bands_engine(case_name, tag, form, plan, edges, sections, 0.0 if threshold_map is not None else thr, tail=tail, lag=lag,
                              threshold_map=threshold_map)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert eng.arrival_bands_count() == (len(steps), int(steps[-1]))
        got, captures = eng.fetch_arrival_bands()
        if query is not None:
            assert eng.query(query) > 0
        assert eng.query(E.Engine.QUERY_ARRIVAL_BANDS_CAPTURES) == len(steps)
        folds = eng.query(E.Engine.QUERY_ARRIVAL_BANDS_FOLDS)
    finally:
        eng.close()
    assert captures == len(steps) and shape == want["bins"].shape and folds <= -(-len(steps) // 16) + 1
    same(got, want)
    return got, want, snaps


FORM_QUERIES = {"single": None, "graph": None, "pair": E.Engine.QUERY_PASSES, "triple": E.Engine.QUERY_TRIPLE_PASSES}


@pytest.mark.parametrize("period", [1, 2, 3, 7])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_fold_of_the_snapshots(form, period, tag):
    """Single steps, graph replay, two- and three-step passes at periods 1, 2, 3 and 7, fp32 and fp64: one plane of the 32^3 impulse
    room, 30 steps (64 under graph replay), two bands of two sections with lags 0 and 2, bins from 0, 1 and 3 captures behind each
    node's onset and a tail of two-capture bins from 4."""
    n_steps = 64 if form == "graph" else 30
    query = FORM_QUERIES[form] if (form == "pair" and period >= 2) or (form == "triple" and period >= 3) else None
    check("impulse_flat", tag, form, dict(PLANE, period=period), (0, 1, 3), random_sections(2, 2, 3), n_steps, tail=(3, 4, 2), lag=(0, 2), query=query)


def _random_factors(shape):
    return 10.0 ** np.random.default_rng(42).uniform(-1, 1, shape)


# (box, K, S, lags, a per-node map?): B = 1 (< 64), 240, 567 (three workgroups, a ragged tail), 630, 720 and 1890 with strides; every
# template instance; one band and eight; lags 0, 2 and 20 -- the lagged stretch of a node that hears its onset at capture 0 .. 12
# crosses the fold boundary at 16 -- and a different lag per band
SHAPES = [("one-node", 1, 1, 2, False), ("sub-box-16-byte-rows", 2, 2, (0, 20), True), ("sub-box-567-odd", 8, 2, (0, 1, 2, 3, 5, 8, 13, 20), True),
          ("sub-box-630", 3, 4, (20, 2, 0), False), ("every-face-stride-3", 1, 4, 0, True), ("strides-1-2-3", 2, 3, (2, 20), False)]


@pytest.mark.parametrize("name,K,S,lag,with_map", SHAPES, ids=["%s-K%dS%d" % s[:3] for s in SHAPES])
def test_boxes_bands_and_sections_on_a_room_with_walls(name, K, S, lag, with_map):
    """tests/golden/cases.py "random": 24 x 20 x 28, six wall filters, a soft source, noise in the field from the start; every step
    captured, 33 captures (16 + 16 + 1), edges (0, 1, 5, 16, 17) and a tail of three-capture bins from 19 whose last bin goes
    open-ended at 28.  The threshold is the median of the per-node max |p|, or a per-node map of 0.1 .. 10 times it."""
    got, want, _ = check("random", "f64", "triple", dict(BOXES[name], period=1), EDGES, random_sections(K, S, 10 * K + S), 32, tail=TAIL_W3, lag=lag,
                         map_factors=_random_factors if with_map else None, spread=name != "one-node")
    if name != "one-node":
        assert (want["bins"][:, -1].reshape(K, -1).max(axis=1) > 0).any()       # the open-ended bin took something


@pytest.mark.parametrize("tail", [None, (3, 20, 7), (20, 18, 1)], ids=["no-tail", "tail-inside-a-fold", "a-bin-per-capture"])
def test_tails(tail):
    check("random", "f32", "pair", dict(BOXES["sub-box-567-odd"], period=1), EDGES, random_sections(2, 3, 9), 32, tail=tail, lag=(0, 2))


def test_a_node_without_an_onset_keeps_everything_in_pre():
    """A threshold above every |p|: no onset, no bin, no moment; pre holds every band's whole energy and the peak is still found."""
    got, want, snaps = check("random", "f64", "single", dict(BOXES["sub-box-630"], period=1), EDGES, random_sections(2, 1, 4), 20, tail=TAIL_W3,
                             threshold=1e30, spread=False)
    assert (got["onset"] == A.NONE).all() and not got["bins"].any() and not got["moment"].any() and (got["pre"] > 0).all()
    assert got["peak"].tobytes() == np.abs(snaps).max(axis=0).tobytes()


def test_identity_sections_reproduce_the_arrival_plan_on_the_device():
    """One band, lag 0, no tail, the section (1, 0, 0, 0, 0): all six outputs are wv_set_arrival's, bytewise."""
    plan = dict(BOXES["sub-box-567-odd"], period=1)
    snaps, _ = reference_snapshots("random", "f64", "pair", plan, 32)
    thr = threshold_of(snaps)
    got, want, _ = check("random", "f64", "pair", plan, EDGES, IDENTITY, 32)
    set_tuning(**FORMS["pair"])
    eng = make_engine(cases.CASES["random"](), "f64")
    try:
        eng.set_arrival(EDGES, thr, **plan)
        assert eng.run_steps(32) == (32, 0)
        plain, captures = eng.fetch_arrival()
    finally:
        eng.close()
    assert captures == 33
    for key in ("onset", "peak", "peak_capture"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    for key in ("pre", "moment", "bins"):
        assert got[key][0].tobytes() == plain[key].tobytes() and np.abs(plain[key]).max() > 0, key


@pytest.mark.parametrize("w,n_bins", [(1, 16), (5, 7), (16, 3), (40, 2)])
def test_threshold_zero_reproduces_the_banded_decay_plan_on_the_device(w, n_bins):
    """Threshold 0, one edge, tail_first = tail_captures = W, n_tail = n - 1: the bins are wv_set_decay_bands' with bin_captures = W and
    n_bins = n, bytewise -- the merged fold and the new one on the same captures, with the reference's Butterworth octave bands."""
    plan = dict(BOXES["sub-box-567-odd"], period=1)
    sections = np.array([D.butterworth_bandpass(lo, hi, 8000.0) for lo, hi in D.octave_band_edges([250.0, 500.0, 1000.0])])
    got, want, _ = check("random", "f64", "pair", plan, (0,), sections, 32, tail=(n_bins - 1, w, w), threshold=0.0, spread=False)
    set_tuning(**FORMS["pair"])
    eng = make_engine(cases.CASES["random"](), "f64")
    try:
        eng.set_decay(n_bins, w, bands=sections, **plan)
        assert eng.run_steps(32) == (32, 0)
        bins, captures = eng.fetch_decay()
    finally:
        eng.close()
    assert captures == 33 and got["bins"].tobytes() == bins.tobytes() and bins.max() > 0
    assert (got["onset"] == 0).all() and not got["pre"].any()


def test_fetching_mid_run_and_at_the_end():
    """A fetch after 14 captures folds t = 14 < 16; the states it leaves carry the next 17 captures."""
    plan = dict(BOXES["sub-box-630"], period=1)
    sections = random_sections(3, 4, 2)
    args = dict(tail=TAIL_W3, lag=(0, 2, 20))
    snaps, steps = reference_snapshots("random", "f64", "pair", plan, 30)
    thr = threshold_of(snaps)
    eng, _ = bands_engine("random", "f64", "pair", plan, EDGES, sections, thr, **args)
    try:
        assert eng.run_steps(13) == (13, 0)
        mid, mid_count = eng.fetch_arrival_bands()
        again, again_count = eng.fetch_arrival_bands()
        assert eng.run_steps(17) == (17, 0)
        end, end_count = eng.fetch_arrival_bands()
    finally:
        eng.close()
    assert (mid_count, again_count, end_count) == (14, 14, 31)
    same(mid, A.banded_arrival_fold(snaps[:14], thr, EDGES, sections, **args))
    same(again, mid)
    want = A.banded_arrival_fold(snaps, thr, EDGES, sections, **args)
    same(end, want)
    assert ((want["onset"] >= 14) & (want["onset"] != A.NONE)).any() and (want["onset"] < 14).any()      # onsets on both sides of the fetch


@pytest.mark.parametrize("form", ["single", "triple"])
def test_checkpoint_run_rollback_rerun_gives_the_same_state_twice(form):
    """The impulse room's plane: the wavefront is crossing it at the checkpoint, so some onsets lie before it and some behind.  The
    checkpoint holds sums AND filter states: the re-run's captures are filtered from the state capture 10 left."""
    plan = dict(PLANE, period=1)
    edges, sections, args = (0, 2, 6), random_sections(2, 3, 8), dict(tail=(3, 8, 2), lag=(0, 2))
    snaps, steps = reference_snapshots("impulse_flat", "f64", form, plan, 27)
    thr = threshold_of(snaps)
    want = A.banded_arrival_fold(snaps, thr, edges, sections, **args)
    heard = want["onset"] != A.NONE
    assert (want["onset"][heard] <= 10).any() and (want["onset"][heard] > 10).any()
    golden = json.load(open(GOLDEN))
    eng, _ = bands_engine("impulse_flat", "f64", form, plan, edges, sections, thr, **args)
    try:
        assert eng.run_steps(10) == (10, 0)            # captures of 0 .. 10
        eng.checkpoint()
        assert eng.run_steps(17) == (17, 0)
        first, first_count = eng.fetch_arrival_bands()
        eng.rollback()
        assert eng.step_count() == 10 and eng.arrival_bands_count() == (11, 10)
        kept, kept_count = eng.fetch_arrival_bands()
        assert eng.run_steps(17) == (17, 0)
        second, second_count = eng.fetch_arrival_bands()
        assert eng.arrival_bands_count() == (28, 27)
        eng.set_arrival_bands(edges, sections, thr, **dict(args, **plan))      # a plan set after the checkpoint has no state to go back to
        assert refusal(lambda e: e.rollback(), eng) == golden["rollback"]
    finally:
        eng.close()
    assert (first_count, kept_count, second_count) == (28, 11, 28)
    same(kept, A.banded_arrival_fold(snaps[:11], thr, edges, sections, **args))
    same(first, want)
    same(second, want)


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("bad_step", [12, 13, 14])
def test_a_run_that_stops_on_a_flag_holds_nothing_of_a_later_step(form, bad_step):
    """inf in the source signal at step f, a capture every 4 steps: sums and onsets hold the captures of 0, 4, 8, 12 and nothing of 16,
    whose field (inf / nan) the batch had already produced when the flag was read.  Neither do the filter states: both engines get
    clean fields and run on, and the continued run's outputs are the twin's continued from the state capture 12 left -- finite."""
    set_tuning(**FORMS[form])
    mesh = M.box_mesh(12, 12, 12)
    sig = np.zeros(40)
    sig[0] = 1.0
    sig[bad_step] = np.inf
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=sig,
                recv=[mesh.compute_index(7, 6, 6)])
    plan = dict(box=((0, 0, 6), (None, None, 1)), period=4)
    sections, args = random_sections(2, 3, 12), dict(tail=(2, 2, 2), lag=(0, 1))
    engines = [make_engine(case, "f64", plan), make_engine(case, "f64")]
    try:
        engines[1].set_arrival_bands((0, 1), sections, 1e-3, **dict(args, **plan))
        memories = [engines[0].read_boundary_data(d) for d in (1, 2, 3)]
        for eng in engines:
            done, flag = eng.run_steps(40)
            assert done == bad_step and flag & M.ERR_INF
        snaps, steps = engines[0].fetch_snapshots()
        assert list(steps) == [0, 4, 8, 12] and engines[1].arrival_bands_count() == (4, 12)
        got, count = engines[1].fetch_arrival_bands()
        want, state = A.banded_arrival_fold(snaps, np.float32(1e-3), (0, 1), sections, return_state=True, **args)
        assert count == 4 and np.isfinite(got["bins"]).all() and np.isfinite(got["peak"]).all() and (want["onset"] != A.NONE).any()
        same(got, want)
        rng = np.random.default_rng(7)
        fields = [rng.uniform(-1, 1, mesh.num_nodes) * (mesh.nodes["boundary_type"] & M.ID_INSIDE != 0) for _ in range(2)]
        sig = np.zeros(16)
        sig[1] = 0.5
        for eng in engines:
            eng.write_field(fields[0], E.BUF_PREVIOUS)
            eng.write_field(fields[1], E.BUF_CURRENT)
            for d, clean in zip((1, 2, 3), memories):
                eng.write_boundary_data(d, clean)
            eng.set_source(E.SOURCE_HARD, mesh.compute_index(6, 6, 6), sig)
            assert eng.run_steps(8) == (8, 0)
        snaps, steps = engines[0].fetch_snapshots()
        assert list(steps) == [0, 4, 8, 12, 16, 20] and engines[1].arrival_bands_count() == (6, 20)
        got, count = engines[1].fetch_arrival_bands()
    finally:
        for eng in engines:
            eng.close()
    continued = A.banded_arrival_fold(snaps[4:], np.float32(1e-3), (0, 1), sections, state=state, first_capture=4, **args)
    assert np.isfinite(got["bins"]).all() and np.isfinite(got["moment"]).all() and (continued["bins"][:, -1] > 0).any()
    same(got, continued)


def test_generic_steps_in_between_capture_nothing():
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    plan = dict(box=((0, 0, 0), (None, None, 2)), period=3)
    sections, args = random_sections(2, 2, 5), dict(tail=(2, 2, 1), lag=(0, 1))
    engines = [make_engine(case, "f32"), make_engine(case, "f32")]
    golden = json.load(open(GOLDEN))
    try:
        for e in engines:
            assert e.run_steps(9) == (9, 0)
        engines[0].set_arrival_bands((0, 1), sections, 0.2, **dict(args, **plan))       # steps 0, 3, 6 lie before the plan
        engines[1].set_snapshots(**plan)
        assert engines[0].arrival_bands_count() == (0, 0)
        for e in engines:
            assert e.run_steps(4) == (4, 0)               # 9 (at the start of this run), 12
            for _ in range(3):                            # 13 -> 16 by generic steps: 15 is passed
                assert e.step() == 0
                e.swap()
        assert engines[0].arrival_bands_count() == (2, 12)
        for e in engines:
            assert e.run_steps(2) == (2, 0)               # 18
        got, count = engines[0].fetch_arrival_bands()
        snaps, steps = engines[1].fetch_snapshots()
        assert list(steps) == [9, 12, 18] and count == 3
        want = A.banded_arrival_fold(snaps, np.float32(0.2), (0, 1), sections, **args)
        same(got, want)
        assert (want["onset"] != A.NONE).any() and (want["onset"] == A.NONE).any()
        engines[0].set_arrival_bands(None, None)          # stops, forgets and frees ...
        assert refusal(lambda e: e.arrival_bands_count(), engines[0]) == golden["no_plan"]["arrival_bands_count"]
        assert refusal(lambda e: e.fetch_arrival_bands(), engines[0]) == golden["no_plan"]["fetch_arrival_bands"]
        engines[0].set_decay(2, 2, **plan)                # ... and a decay plan takes its place
        assert engines[0].run_steps(3) == (3, 0) and engines[0].decay_count() == (2, 21)
    finally:
        for e in engines:
            e.close()


# ---- refusals: code and text against tests/golden/arrival_bands_refusals.json, written by hand from the contract ----------------

BOX = ((1, 1, 1), (4, 3, 2))
BANDS = np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]], [[0.5, 0.25, 0.0, -0.1, 0.0]]])
SET8 = dict(SET7, modulation=lambda e: e.set_modulation([0.0, 0.125], BANDS, box=BOX))
STOP8 = dict(STOP7, modulation=lambda e: e.set_modulation(None, None))


def set_bands(e, **faults):
    """A good plan on the 12 x 10 x 9 mesh with the named faults put in."""
    tail = [3, 6, 2]
    for index, key in enumerate(("n_tail", "tail_first", "tail_captures")):
        if key in faults:
            tail[index] = faults.pop(key)
    args = dict(edges=(0, 4), bands=BANDS, threshold=1e-3, tail=tuple(tail), lag=3, box=BOX)
    args.update(faults)
    return e.set_arrival_bands(args.pop("edges"), args.pop("bands"), **args)


def bad_map(stride_fault):
    m = np.full((2, 0 if stride_fault else 3, 4), 1e-3, np.float32)      # (a zero stride takes no node along its axis)
    m[..., 1] = -1e-3
    return m


FAULTS = {"stride": dict(stride=(1, 0, 1)), "period": dict(period=0), "box": dict(box=((9, 1, 1), (4, 3, 2))),
          "bands": dict(bands=np.repeat(BANDS[:1], 9, axis=0)), "coefficient": dict(bands=BANDS * np.array([1, 1, 1, np.nan, 1])),
          "n_edges": dict(edges=()), "edges": dict(edges=(0, 5, 5)), "threshold": dict(threshold=-1.0), "map": None,
          "n_tail": dict(n_tail=4095), "tail_first": dict(tail_first=4), "tail_captures": dict(tail_captures=0), "reserved": dict(reserved=1)}


def faults_of(*names):
    merged = {}
    for name in names:
        merged.update(FAULTS[name] or dict(threshold_map=bad_map("stride" in names)))
    return merged


def test_every_refusal_in_code_text_and_order():
    """Every single fault answers its sentence, and of two faults the one the contract asks first: the shared checks, then bands,
    sections and coefficients, then edges, threshold and map, then the tail and the reserved word.  ("edges" with "n_edges" is one
    fault, and so is "coefficient" with "bands": each pair sets one argument.)  An earlier plan survives every refused call."""
    golden = json.load(open(GOLDEN))
    names = [name for name, _ in golden["arguments"]]
    assert names == list(FAULTS) and all(code == -1 for _, (code, _) in golden["arguments"])
    says = dict(golden["arguments"])
    eng = E.Engine(M.box_mesh(12, 10, 9), precision="f32")
    try:
        set_bands(eng)
        assert eng.run_steps(3) == (3, 0)
        before, count = eng.fetch_arrival_bands()
        for i, first in enumerate(names):
            assert refusal(lambda e: set_bands(e, **faults_of(first)), eng) == says[first], first
            for second in names[i + 1:]:
                if {first, second} in ({"bands", "coefficient"}, {"n_edges", "edges"}):
                    continue
                assert refusal(lambda e: set_bands(e, **faults_of(first, second)), eng) == says[first], (first, second)
        for bad in ((1, 2), (0, 5, 4)):
            assert refusal(lambda e: set_bands(e, edges=bad), eng) == says["edges"]
        for bad in (np.inf, np.nan):
            assert refusal(lambda e: set_bands(e, threshold=bad), eng) == says["threshold"]
        assert refusal(lambda e: set_bands(e, bands=np.zeros((1, 5, 5))), eng) == says["bands"]
        assert refusal(lambda e: set_bands(e, n_tail=4096), eng) == says["n_tail"]
        with pytest.raises(ValueError):
            set_bands(eng, edges=tuple(range(17)))
        set_bands(eng, n_tail=0, tail_first=0, tail_captures=0)      # without a tail neither is looked at ...
        set_bands(eng)                                               # ... (and the plan is back, from capture 0)
        assert eng.arrival_bands_count() == (0, 0)
    finally:
        eng.close()
    assert count == 4 and before["bins"].shape == (2, 5, 2, 3, 4)


def test_the_plans_exclude_each_other_both_ways():
    """The new setter under each of the eight existing plans, in their sentences; each of the eight setters under the new plan, in its
    one sentence; the refused call leaves the active plan capturing, and once it is stopped the refused setter goes through."""
    golden = json.load(open(GOLDEN))
    assert sorted(golden["under"]) == sorted(golden["while_active"]) == sorted(SET8) and len(SET8) == 8
    eng = E.Engine(M.box_mesh(12, 10, 9), precision="f32")
    try:
        for kind in sorted(SET8):
            SET8[kind](eng)
            assert refusal(set_bands, eng) == golden["under"][kind], kind
            assert eng.run_steps(2) == (2, 0)
            STOP8[kind](eng)
        set_bands(eng)
        assert eng.run_steps(2) == (2, 0)
        before, count = eng.fetch_arrival_bands()
        for kind in sorted(SET8):
            assert refusal(SET8[kind], eng) == golden["while_active"][kind], kind
        after, after_count = eng.fetch_arrival_bands()
        assert after_count == count == 3
        same(after, before)
        assert eng.run_steps(2) == (2, 0) and eng.arrival_bands_count()[0] == 5
        eng.set_arrival_bands(None, None)
        for kind in sorted(SET8):
            SET8[kind](eng)
            STOP8[kind](eng)
    finally:
        eng.close()
    # a slab of a chain; a group takes no engine with a plan
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    try:
        assert refusal(lambda e: e.set_arrival_bands((0, 2), BANDS, 0.1, box=((0, 0, 0), (4, 4, 1))), slab) == golden["slab"]
    finally:
        slab.close()
    eng = E.Engine(mesh, precision="f32")
    group = E.LocalSlabGroup([eng])
    try:
        eng.set_arrival_bands((0, 2), BANDS, 0.1, box=((0, 0, 0), (4, 4, 1)))
        assert refusal(lambda g: g.run_steps(4), group) == golden["group"]
        eng.set_arrival_bands(None, None)
        assert group.run_steps(4) == (4, 0)
    finally:
        group.close()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise."""
    set_tuning(**FORMS[form])
    case = cases.CASES["random"]()
    out = []
    for plan in (None, dict(box="mesh", stride=(1, 2, 1), period=7, first_step=3)):
        eng = make_engine(case, tag)
        try:
            if plan:
                eng.set_arrival_bands((0, 2, 4), random_sections(3, 4, 1), 0.3, tail=(2, 5, 1), lag=(0, 1, 2), **plan)
            assert eng.run_steps(case["steps"]) == (case["steps"], 0)
            out.append([eng.fetch_receivers(0, case["steps"]), eng.read_field(E.BUF_CURRENT), eng.read_field(E.BUF_PREVIOUS)] +
                       [eng.read_boundary_data(d) for d in (1, 2, 3)])
            if plan:
                assert eng.arrival_bands_count() == (9, 59)   # steps 3, 10, ..., 59
        finally:
            eng.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert np.abs(out[0][0]).max() > 0


def test_kernel_timing_accounts_for_the_fold_kernels():
    eng, _ = bands_engine("impulse_flat", "f64", "single", dict(box="mesh", period=1), (0, 4, 8), random_sections(2, 4, 1), 1e-6, tail=(4, 12, 4))
    try:
        eng.enable_kernel_timing(True)
        assert eng.run_steps(40) == (40, 0)
        eng.fetch_arrival_bands()
        assert eng.query(E.Engine.QUERY_ARRIVAL_BANDS_FOLDS) == 3 and eng.query(E.Engine.QUERY_ARRIVAL_BANDS_NS) > 0
    finally:
        eng.close()


def test_canonical_returns_the_band_maps_beside_the_receiver_output():
    """simulation.canonical(..., arrival=dict(bands=...)): the records are those of a run without a plan, the state is the
    engine-level one, folded from canonical's own snapshots of the same plane and cadence with the sections, edges, tail and lags
    arrival_bands_plan_arguments names."""
    from test_gpu_decay import _box_scene
    set_tuning()
    W, vm, source, receiver = _box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    plane_z = 12 * vm.mesh.spacing
    spec = dict(plane=plane_z, every=2, threshold=1e-4, early_ms=(6e3 / rate, 10e3 / rate), bands=[(rate / 40, rate / 20), (rate / 20, rate / 10)],
                tail_ms=30e3 / rate, tail_bin_ms=4e3 / rate, lag="group-delay")
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                         snapshots=dict(box=((0, 0, 12), (None, None, 1)), period=2))
    bands, (out, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", arrival=spec)
    args = W.arrival_bands_plan_arguments(spec, vm.mesh, rate)
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert args["edges"] == [0, 3, 5] and args["tail"] == (4, 7, 2) and len(args["lag"]) == 2 and max(args["lag"]) > 0
    assert captures == 21 and out["bins"].shape == (2, 7, 1, 24, 24)
    want = A.banded_arrival_fold(fields, np.float32(1e-4), args["edges"], args["bands"], tail=args["tail"], lag=args["lag"])
    same(out, want)
    assert (want["onset"] != A.NONE).any() and len(set(want["onset"].ravel().tolist())) >= 3
    zero = W.arrival_bands_plan_arguments(dict(spec, lag=0), vm.mesh, rate)
    assert zero["lag"] == [0, 0]


def test_the_tool_writes_per_band_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --clarity-map --clarity-bands 31.5,63 --clarity-tail-ms 200 on its built-in hall, a short run."""
    out = tmp_path / "arrival.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.1",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--clarity-map", "--arrival-plane", "z=1.5",
                        "--arrival-threshold", "1e-5", "--arrival-out", str(out), "--clarity-bands", "31.5,63", "--clarity-tail-ms", "200"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        got = {k: f[k] for k in f.files}
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    n_bins = len(got["edges"]) + int(got["tail"][0])
    assert got["bins"].shape == (2, n_bins, dims[1], dims[0]) and int(got["tail"][0]) >= 1 and int(got["captures"]) == steps + 1
    assert got["onset"].shape == (dims[1], dims[0]) and got["c80_db"].shape == got["ts_s"].shape == got["t20_s"].shape == (2, dims[1], dims[0])
    assert list(got["bands_hz"]) == [31.5, 63.0] and got["lag"].shape == (2,)
    heard = got["onset"] != A.NONE
    assert heard.any() and (got["bins"][:, 0][:, heard] > 0).all() and (got["ts_s"][:, heard] >= 0).all()


def test_the_rate_tool_runs_and_its_outputs_equal_the_definition(tmp_path):
    """tools/arrival_bands_rate.py on a 48 x 48 x 16 room, 48 steps per repeat, two repeats: every row is there, the plan's outputs equal
    arrival.banded_arrival_fold over the snapshots bytewise, and the figures land in the JSON file."""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "arrival_bands_rate.py"), "--dims", "48,48,16",
                        "--steps", "48", "--bands", "1,4", "--repeats", "2", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 2 and "ARRIVAL BANDS RATE OK" in p.stdout, p.stdout
    report = json.load(open(str(out)))
    for bands in (1, 4):
        rows = report["f64"]["%d bands" % bands]
        assert rows["bytewise_equal"] is True and rows["captures"] == 48
        assert sorted(rows["rows"]) == ["arrival", "arrival_bands", "decay_bands", "none"]
        assert rows["rows"]["arrival_bands"]["folds"] >= 1 and rows["rows"]["arrival_bands"]["mean_fold_ms"] > 0

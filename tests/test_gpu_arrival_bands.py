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
from test_arrival_bands_host import IDENTITY
from plan_cases import (BOXES, FILE_FORMS, FORMS, FORM_QUERIES, box_scene, changes_nothing, check, default_tuning_afterwards,
                        make_engine, plan_on, random_sections, reference_snapshots, scaled_map)
from plan_cases import median_or_lower_quartile as threshold_of
from test_gpu_plan_refusals import refusal
from test_gpu_plan_refusals import SET as SET7
from test_gpu_plan_refusals import STOP as STOP7
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
    default_tuning_afterwards()


def bands_plan(case, cadence, edges, sections, tail=None, lag=0, threshold=threshold_of, map_factors=None):
    """`threshold`: a number, or a callable(snaps, plan) of the reference's snapshots; `map_factors`: a per-node map of that many times it."""
    lag = [int(lag)] * sections.shape[0] if np.isscalar(lag) else list(lag)
    onset = dict(threshold=threshold) if map_factors is None else dict(threshold=0.0, threshold_map=scaled_map(threshold, map_factors))
    return plan_on(case, "arrival_bands", edges=list(edges), bands=sections, tail=tail, lag=lag, **onset, **cadence)


def same(got, want):
    for key in A.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), "%s differs at %d places" % (key, (got[key] != want[key]).sum())


@pytest.mark.parametrize("period", [1, 2, 3, 7])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_fold_of_the_snapshots(form, period, tag):
    """Single steps, graph replay, two- and three-step passes at periods 1, 2, 3 and 7, fp32 and fp64: one plane of the 32^3 impulse
    room, 30 steps (64 under graph replay), two bands of two sections with lags 0 and 2, bins from 0, 1 and 3 captures behind each
    node's onset and a tail of two-capture bins from 4."""
    n_steps = 64 if form == "graph" else 30
    query = FORM_QUERIES[form] if (form == "pair" and period >= 2) or (form == "triple" and period >= 3) else None
    plan = bands_plan("impulse_flat", dict(PLANE, period=period), (0, 1, 3), random_sections(2, 2, 3), tail=(3, 4, 2), lag=(0, 2))
    check("arrival_bands", "impulse_flat", tag, form, plan, n_steps, query)


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
    plan = bands_plan("random", dict(BOXES[name], period=1), EDGES, random_sections(K, S, 10 * K + S), tail=TAIL_W3, lag=lag,
                      map_factors=_random_factors if with_map else None)
    want = check("arrival_bands", "random", "f64", "triple", plan, 32, **(dict(condition=None) if name == "one-node" else {}))[1]
    if name != "one-node":
        assert (want["bins"][:, -1].reshape(K, -1).max(axis=1) > 0).any()       # the open-ended bin took something


@pytest.mark.parametrize("tail", [None, (3, 20, 7), (20, 18, 1)], ids=["no-tail", "tail-inside-a-fold", "a-bin-per-capture"])
def test_tails(tail):
    check("arrival_bands", "random", "f32", "pair", bands_plan("random", dict(BOXES["sub-box-567-odd"], period=1), EDGES, random_sections(2, 3, 9), tail=tail, lag=(0, 2)), 32)


def test_a_node_without_an_onset_keeps_everything_in_pre():
    """A threshold above every |p|: no onset, no bin, no moment; pre holds every band's whole energy and the peak is still found."""
    plan = bands_plan("random", dict(BOXES["sub-box-630"], period=1), EDGES, random_sections(2, 1, 4), tail=TAIL_W3, threshold=float(np.float32(1e30)))
    got, _, _, snaps, _ = check("arrival_bands", "random", "f64", "single", plan, 20, condition=None)
    assert (got["onset"] == A.NONE).all() and not got["bins"].any() and not got["moment"].any() and (got["pre"] > 0).all()
    assert got["peak"].tobytes() == np.abs(snaps).max(axis=0).tobytes()


def test_identity_sections_reproduce_the_arrival_plan_on_the_device():
    """One band, lag 0, no tail, the section (1, 0, 0, 0, 0): all six outputs are wv_set_arrival's, bytewise."""
    plan = dict(BOXES["sub-box-567-odd"], period=1)
    snaps, _ = reference_snapshots("random", "f64", "pair", plan, 32)
    thr = threshold_of(snaps)
    got = check("arrival_bands", "random", "f64", "pair", bands_plan("random", plan, EDGES, IDENTITY), 32)[0]
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
    got = check("arrival_bands", "random", "f64", "pair", bands_plan("random", plan, (0,), sections, tail=(n_bins - 1, w, w), threshold=0.0), 32, condition=None)[0]
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


@pytest.mark.parametrize("form", FILE_FORMS["arrival_bands"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("arrival_bands", tag, form)


def test_canonical_returns_the_band_maps_beside_the_receiver_output():
    """simulation.canonical(..., arrival=dict(bands=...)): the records are those of a run without a plan, the state is the
    engine-level one, folded from canonical's own snapshots of the same plane and cadence with the sections, edges, tail and lags
    arrival_bands_plan_arguments names."""
    set_tuning()
    W, vm, source, receiver = box_scene()
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

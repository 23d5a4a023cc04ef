"""Lateral maps: p^2, p v and v v^T binned from each node's own onset, accumulated on the device while wv_run keeps going
(wv_set_lateral; csrc/lateral_kernels.hip.h, engine_lateral.hip.h).  The reference of every comparison is a second, identical
engine with a SNAPSHOT plan of the box's hull at the same cadence, whose snapshots lateral.lateral_fold -- the definition in NumPy --
folds in capture order.  Equality is BYTEWISE on onset, pre, the velocities and all ten bin planes.  Small meshes, forms forced, a
few dozen steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import set_tuning
from plan_cases import HULL_BOXES as BOXES
from plan_cases import (FILE_COUNTS, FILE_FORMS, FORMS, FORM_QUERIES, box_of, box_scene, capture_counts, changes_nothing, check, constants, default_tuning_afterwards, filled_bins,
                        hull_of, make_engine, plan_engine, plan_on, quantile_threshold, quarters, reference_snapshots, scaled_map)
from wayverb_amd import arrival as A
from wayverb_amd import engine as E
from wayverb_amd import lateral as L
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def quantile(q):
    return lambda snaps, plan: quantile_threshold(snaps, plan, q)


def lateral_plan(case, cadence, edges, threshold, map_factors=None):
    """`threshold`: a number, or a callable(snaps, plan) of the reference's hull snapshots; `map_factors`: a per-node map of that many times it."""
    if map_factors is not None:
        return plan_on(case, "lateral", edges=list(edges), threshold=0.0, threshold_map=scaled_map(threshold, map_factors), **cadence)
    return plan_on(case, "lateral", edges=list(edges), threshold=threshold, **cadence)


def fold(snaps, plan, threshold, edges, **more):
    """The definition over hull snapshots of `plan`'s box, with the constants the engine is given."""
    c = constants(plan)
    return L.lateral_fold(snaps, hull_of(plan)[1], threshold, edges, c["spacing"], c["sample_rate"], c["ambient_density"], **more)


def same(got, want):
    for key in L.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if got[key].tobytes() != want[key].tobytes():
            planes = [L.PLANES[a] for a in range(10) if got[key][a].tobytes() != want[key][a].tobytes()] if key == "bins" else ""
            raise AssertionError("%s differs at %d entries %s" % (key, (got[key] != want[key]).sum(), planes))


PLANE = dict(box=((1, 1, 15), (30, 30, 1)))


@pytest.mark.parametrize("period", range(1, 8))
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_fold_of_the_hull_snapshots(form, period, tag):
    """Single steps, graph replay, two- and three-step passes at periods 1 .. 7: the plane next to the source of the 32^3 impulse
    room less its rim, 30 steps (64 under graph replay), bins that begin 0, 1 and 3 captures behind each node's own onset.

    The threshold is a quantile of the NON-ZERO per-node maxima of |p| (the plain median is exactly 0 at even periods: the
    checkerboard, see test_gpu_arrival.py).  On the CPU restatement of both precisions, at 30 and at 64 steps:
      - odd periods, the MEDIAN (q = 0.5): 408 .. 456 of the 900 nodes hear an onset and all four conditions of not_trivial hold.  (The
        lower quartile does not serve: at period 5 over 64 steps in f64 it leaves 224 nodes without an onset, one short of a quarter.)
      - even periods, the LOWER QUARTILE (q = 0.25): 336 .. 344 nodes hear an onset (the median leaves 224 at period 4, one short of a
        quarter), and the first three conditions and two bins of E hold.  The fourth cannot hold with ANY threshold: captures an even
        number of steps apart see one colour of the checkerboard move, so a node that ever holds a pressure has six neighbours that
        hold exactly 0 in every capture, its two differences along an axis are equal, g = 0 and v stays 0 -- every Q and I plane is
        zero wherever a threshold above 0 finds an onset, and a threshold of 0 leaves no node without one.  That is asserted as it
        is, and the even periods are compared a second time with a threshold of 0, where every node has its onset at capture 0 and
        the silent colour -- whose neighbours move -- fills two bins of the Q planes and more."""
    n_steps = 64 if form == "graph" else 30
    # (a pass form shows in its counter only where the period leaves room for a pass of that length)
    query = FORM_QUERIES[form] if (form == "pair" and period >= 2) or (form == "triple" and period >= 3) else None
    plan = dict(PLANE, period=period)
    if period % 2 == 1:
        check("lateral", "impulse_flat", tag, form, lateral_plan("impulse_flat", plan, (0, 1, 3), quantile(0.5)), n_steps, query)
        return
    got, want, full, snaps, _ = check("lateral", "impulse_flat", tag, form, lateral_plan("impulse_flat", plan, (0, 1, 3), quantile(0.25)), n_steps, query,
                                      condition=quarters)
    highest = np.abs(box_of(snaps, full)).max(axis=0)
    assert (highest == 0).sum() >= highest.size / 2          # the silent colour: the plain median would be 0, or next to it
    heard = want["onset"] != L.NONE
    assert (want["bins"][1:, :, heard] == 0).all() and (want["velocity"][:, heard] == 0).all() and np.abs(want["velocity"][:, ~heard]).max() > 0
    want = check("lateral", "impulse_flat", tag, form, lateral_plan("impulse_flat", plan, (0, 1, 3), 0.0), n_steps, condition=None)[1]
    assert (want["onset"] == 0).all() and filled_bins(want["bins"][0]) >= 2 and max(filled_bins(want["bins"][a]) for a in range(4, 10)) >= 2


def _random_factors(shape):
    return 10.0 ** np.random.default_rng(42).uniform(-1, 1, shape)


@pytest.mark.parametrize("with_map", [False, True], ids=["scalar", "map"])
@pytest.mark.parametrize("name", sorted(BOXES))
def test_boxes_and_strides_on_a_room_with_walls(name, with_map):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source, noise in the field from the start;
    every step captured, 33 captures (16 + 16 + 1), edges (0, 1, 5, 16, 17): an edge inside a fold, one on a fold's first slot and
    one behind it.  Once with the scalar median of the per-node maxima as the threshold, once with a per-node map of 0.1 .. 10 times
    that median.  (One node has no quarter of nodes to show: the box of one node is compared as it is.)"""
    plan = dict(BOXES[name], period=1)
    check("lateral", "random", "f64", "triple", lateral_plan("random", plan, (0, 1, 5, 16, 17), quantile(0.5), _random_factors if with_map else None), 32,
          **(dict(condition=None) if name == "one-node" else {}))


@pytest.mark.parametrize("w,n_bins", [(1, 8), (5, 7), (16, 3), (40, 2)])
def test_threshold_zero_and_even_edges_equal_the_intensity_plan(w, n_bins):
    """Every onset is capture 0: E and I are an intensity plan's bins of the same box, cadence and bin_captures, and the velocities
    its velocities, bytewise -- the merged fold and the new one on the same captures."""
    plan = dict(BOXES["sub-box-567-odd"], period=1)
    got = check("lateral", "random", "f64", "pair", lateral_plan("random", plan, [k * w for k in range(n_bins)], 0.0), 32, condition=None)[0]
    set_tuning(**FORMS["pair"])
    eng = make_engine(cases.CASES["random"](), "f64")
    eng.set_intensity(n_bins, w, **plan, **constants(plan))
    try:
        assert eng.run_steps(32) == (32, 0)
        bins, captures = eng.fetch_intensity()
        velocity = eng.fetch_intensity_velocity()
    finally:
        eng.close()
    assert captures == 33 and all(np.abs(bins[a]).max() > 0 for a in range(4))
    assert got["bins"][1:4].tobytes() == bins[:3].tobytes() and got["bins"][0].tobytes() == bins[3].tobytes()
    assert got["velocity"].tobytes() == velocity.tobytes()
    assert (got["onset"] == 0).all() and got["pre"].tobytes() == np.zeros(got["pre"].shape).tobytes()


@pytest.mark.parametrize("name", ["sub-box-630", "strides-1-2-3"])
def test_onset_pre_and_energy_equal_the_arrival_plan(name):
    """A thresholded run against an arrival plan of the same box, cadence, threshold and edges: onset, pre and the E plane are its
    onset, pre and bins, bytewise."""
    plan = dict(BOXES[name], period=1)
    edges = (0, 1, 5, 16, 17)
    got, _, full, _, _ = check("lateral", "random", "f64", "pair", lateral_plan("random", plan, edges, quantile(0.5)), 32)
    set_tuning(**FORMS["pair"])
    eng = make_engine(cases.CASES["random"](), "f64")
    eng.set_arrival(edges, full["threshold"], **plan)
    try:
        assert eng.run_steps(32) == (32, 0)
        arrival, captures = eng.fetch_arrival()
    finally:
        eng.close()
    assert captures == 33 and (arrival["onset"] == A.NONE).any() and len(set(arrival["onset"].ravel().tolist())) > 3
    assert got["onset"].tobytes() == arrival["onset"].tobytes() and got["pre"].tobytes() == arrival["pre"].tobytes()
    assert got["bins"][0].tobytes() == arrival["bins"].tobytes()


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_the_receiver_path_carries_the_same_velocities(tag):
    """Four nodes whose 7-point hull does not hold the source node, period 1, first_step 0: the velocities the directional receivers
    carry after n steps equal the plan's after the captures of steps 0 .. n - 1, bytewise -- with a threshold no node reaches, so the
    integrator is seen to run ahead of the onset."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    mesh = case["mesh"]
    sx, sy, sz = mesh.compute_locator(case["source_node"])
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    picks = [(x, y, z) for (x, y, z) in ((3, 2, 4), (12, 10, 10), (7, 6, 5), (4, 10, 9)) if abs(x - sx) + abs(y - sy) + abs(z - sz) > 1]
    assert len(picks) == 4, "the case's source moved next to a picked node"
    n = 24
    c = constants(plan)
    recv = make_engine(case, tag)
    try:
        recv.set_directional_receivers([mesh.compute_index(*p) for p in picks], c["spacing"], c["sample_rate"], c["ambient_density"])
        assert recv.run_steps(n) == (n, 0)                      # records of steps 0 .. n - 1
        recv_v = recv.fetch_directional_velocity(4)
    finally:
        recv.close()
    for threshold in (1e30, 0.0):
        eng = plan_engine(case, tag, "pair", lateral_plan(case, plan, (0, 4), threshold))
        try:
            assert eng.run_steps(n - 1) == (n - 1, 0)           # captures of steps 0 .. n - 1
            assert eng.lateral_count() == (n, n - 1)
            got, _ = eng.fetch_lateral()
        finally:
            eng.close()
        assert (got["onset"] == (L.NONE if threshold else 0)).all()
        for r, (x, y, z) in enumerate(picks):
            assert recv_v[r].tobytes() == got["velocity"][:, z - 4, y - 2, x - 3].tobytes()
    assert np.abs(recv_v).min() > 0


def test_refusals_leave_an_earlier_plan_intact_and_all_six_plans_exclude_each_other():
    """Bad n_bins, edges, thresholds, strides, period, constants and boxes: WV_E_INVALID_ARGUMENT, a node on a face of the mesh with
    the reference's sentence; each of the five other plans while a lateral plan is active and a lateral plan while each of them is:
    WV_E_STATE with the plan to stop in the message; a slab: WV_E_STATE.  After the refusals the earlier plan's results are what they
    were and it goes on capturing."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(BOXES["sub-box-630"], period=1)
    c = constants(plan)
    edges = (0, 1, 5)
    snaps, _ = reference_snapshots("random", "f64", "single", hull_of(plan)[0], 32)
    thr = quantile_threshold(snaps, plan_on("random", "lateral", **plan), 0.5)
    snapshot_plan = dict(box=plan["box"], period=1)
    intensity = dict(box=((1, 1, 1), (4, 4, 4)), **c)
    bands = np.array([[[1.0, 0, 0, 0, 0]]])
    eng = make_engine(case, "f64")
    try:
        eng.set_lateral(edges, thr, **plan, **c)
        assert eng.run_steps(5) == (5, 0)
        before, before_count = eng.fetch_lateral()
        for bad in ((), tuple(range(9)), (1, 2), (0, 5, 5), (0, 5, 4)):
            with pytest.raises((E.WaveguideError, ValueError), match="error -1: .*(n_bins|edges)|8 bins"):
                eng.set_lateral(bad, thr, **plan, **c)
        for bad in (-1.0, np.inf, np.nan):
            with pytest.raises(E.WaveguideError, match="error -1: .*threshold"):
                eng.set_lateral(edges, bad, **plan, **c)
        bad_map = np.full((7, 9, 10), thr, np.float32)
        bad_map[3, 4, 5] = -thr
        with pytest.raises(E.WaveguideError, match="error -1: .*threshold map"):
            eng.set_lateral(edges, thr, threshold_map=bad_map, **plan, **c)
        for bad_box in (((1, 1, 1), (24, 18, 26)), ((-1, 1, 1), (4, 4, 4)), ((1, 1, 28), (1, 1, 1))):
            with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
                eng.set_lateral(edges, thr, box=bad_box, **c)
        for edge_box in (((0, 1, 1), (4, 4, 4)), ((1, 0, 1), (4, 4, 4)), ((1, 1, 0), (4, 4, 4)), ((1, 1, 1), (23, 4, 4)), ((1, 1, 1), (4, 19, 4)),
                         ((1, 1, 1), (4, 4, 27))):
            with pytest.raises(E.WaveguideError, match="error -1: Can't place directional_receiver at this node as it is adjacent to a boundary."):
                eng.set_lateral(edges, thr, box=edge_box, **c)
        with pytest.raises(E.WaveguideError, match="error -1: .*stride"):
            eng.set_lateral(edges, thr, stride=(1, 0, 1), **c)
        with pytest.raises(E.WaveguideError, match="error -1: .*period"):
            eng.set_lateral(edges, thr, period=0, **c)
        for bad in (dict(c, spacing=0.0), dict(c, sample_rate=-1.0), dict(c, ambient_density=float("inf")), dict(c, spacing=float("nan"))):
            with pytest.raises(E.WaveguideError, match="error -1: .*positive and finite"):
                eng.set_lateral(edges, thr, **plan, **bad)
        stop = r"error -6: .*a lateral plan is active \(wv_set_lateral\(e, NULL, NULL\)"
        for set_other in (lambda: eng.set_snapshots(**snapshot_plan), lambda: eng.set_spectrum([0.1], **snapshot_plan),
                          lambda: eng.set_decay(4, 2, **snapshot_plan), lambda: eng.set_decay(4, 2, bands=bands, **snapshot_plan),
                          lambda: eng.set_intensity(2, 2, **intensity), lambda: eng.set_arrival(edges, thr, **snapshot_plan)):
            with pytest.raises(E.WaveguideError, match=stop):
                set_other()
        after, after_count = eng.fetch_lateral()
        assert after_count == before_count == 6
        same(after, before)
        same(after, fold(snaps[:6], plan, thr, edges))
        assert eng.run_steps(3) == (3, 0) and eng.lateral_count() == (9, 8)
        same(eng.fetch_lateral()[0], fold(snaps[:9], plan, thr, edges))
    finally:
        eng.close()
    # the other way round: each of the five other plans refuses a lateral plan, and goes on
    others = [(r"a snapshot plan is active \(wv_set_snapshots\(e, NULL\)", lambda e: e.set_snapshots(**snapshot_plan), lambda e: e.snapshot_count()[0] == 5),
              (r"a spectrum plan is active \(wv_set_spectrum\(e, NULL, NULL\)", lambda e: e.set_spectrum([0.0], **snapshot_plan), lambda e: e.spectrum_count() == (5, 4)),
              (r"a decay plan is active \(wv_set_decay\(e, NULL\)", lambda e: e.set_decay(4, 2, **snapshot_plan), lambda e: e.decay_count() == (5, 4)),
              (r"a banded decay plan is active \(wv_set_decay_bands\(e, NULL, NULL, 0, 0\)", lambda e: e.set_decay(4, 2, bands=bands, **snapshot_plan),
               lambda e: e.decay_count() == (5, 4)),
              (r"an intensity plan is active \(wv_set_intensity\(e, NULL\)", lambda e: e.set_intensity(2, 2, **intensity), lambda e: e.intensity_count() == (5, 4)),
              (r"an arrival plan is active \(wv_set_arrival\(e, NULL, NULL\)", lambda e: e.set_arrival(edges, thr, **snapshot_plan),
               lambda e: e.arrival_count() == (5, 4))]
    for stop, set_other, went_on in others:
        eng = make_engine(case, "f64")
        try:
            set_other(eng)
            assert eng.run_steps(2) == (2, 0)
            with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_lateral: " + stop):
                eng.set_lateral(edges, thr, **plan, **c)
            with pytest.raises(E.WaveguideError, match="error -6: .*no lateral plan"):
                eng.fetch_lateral()
            assert eng.run_steps(2) == (2, 0) and went_on(eng)
        finally:
            eng.close()
    # a slab of a chain; a group takes no engine with a plan
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    try:
        with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
            slab.set_lateral((0, 2), 0.1, box=((1, 1, 1), (4, 4, 1)), **c)
    finally:
        slab.close()
    eng = E.Engine(mesh, precision="f32")
    group = E.LocalSlabGroup([eng])
    try:
        eng.set_lateral((0, 2), 0.1, box=((1, 1, 1), (4, 4, 1)), **c)
        with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no lateral maps"):
            group.run_steps(4)
        eng.set_lateral(None)
        assert group.run_steps(4) == (4, 0)
    finally:
        group.close()


@pytest.mark.parametrize("captures", FILE_COUNTS["lateral"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("lateral", captures)


@pytest.mark.parametrize("form", FILE_FORMS["lateral"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("lateral", tag, form)


def test_canonical_returns_the_maps_beside_the_receiver_output():
    """simulation.canonical(..., lateral=dict(plane=, every=, threshold=, edges_ms=)): the records are those of a run without a plan,
    the state is the definition's over canonical's own snapshots of the plane's hull at the same cadence, with the mesh's spacing,
    sample_rate / every and the environment's density filled in; a second plan beside it is refused with the engine's message."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    plan = dict(box=((1, 1, 11), (22, 22, 1)), period=3)    # (an odd period: see the stepping forms' docstring)
    hplan, box_in_hull = hull_of(plan)
    edges_ms = (0, 9e3 / rate, 15e3 / rate)                 # 9 and 15 steps: 3 and 5 captures at every=3
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=hplan)
    bands, (out, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                         lateral=dict(plane=11 * vm.mesh.spacing, every=3, threshold=1e-4, edges_ms=edges_ms))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 14 == len(steps) and out["bins"].shape == (10, 3, 1, 22, 22)
    want = L.lateral_fold(fields, box_in_hull, np.float32(1e-4), (0, 3, 5), vm.mesh.spacing, rate / 3, env.ambient_density)
    same(out, want)
    assert (want["onset"] != L.NONE).any() and len(set(want["onset"].ravel().tolist())) >= 3
    assert all(np.abs(want["bins"][a]).max() > 0 for a in range(10))
    with pytest.raises(E.WaveguideError, match="error -6: .*snapshot plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, snapshots=dict(period=8), lateral=dict(plane=0.5, threshold=1e-4))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, lateral=dict(plane=0.5, threshold=1e-4))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, lateral=dict(plane=0.0, threshold=1e-4))     # the floor: no node below it


def test_the_tool_writes_the_lateral_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --lateral-map --lateral-plane z=... --lateral-out FILE.npz on its built-in hall, a short run."""
    out = tmp_path / "lateral.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.1",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--lateral-map", "--lateral-plane", "z=1.5",
                        "--lateral-threshold", "1e-5", "--lateral-out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        got = {k: f[k] for k in f.files}
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    rate = float(got["sample_rate"])
    plane = (dims[1] - 2, dims[0] - 2)
    assert got["bins"].shape == (10, 3) + plane and got["velocity"].shape == got["direct_direction"].shape == got["lateral_axis"].shape == (3,) + plane
    assert got["onset"].shape == got["lf"].shape == got["diffuseness"].shape == plane
    assert list(got["edges"]) == L.edges_from_ms((5, 80), 1, rate) and int(got["captures"]) == steps + 1
    heard = got["onset"] != L.NONE
    known = np.isfinite(got["lf"])
    assert heard.any() and known.any() and not known[~heard].any() and (got["lf"][known] >= 0).all()
    facing = np.isfinite(got["direct_direction"][0])
    assert facing.any() and np.allclose((got["direct_direction"][:, facing] ** 2).sum(axis=0), 1.0)
    sideways = np.isfinite(got["lateral_axis"][0])
    assert sideways.any() and np.allclose((got["lateral_axis"][:, sideways] ** 2).sum(axis=0), 1.0)
    assert np.abs((got["lateral_axis"] * got["direct_direction"])[:, sideways].sum(axis=0)).max() < 1e-12 and (got["lateral_axis"][2][sideways] == 0).all()
    assert all(np.abs(got["bins"][a]).max() > 0 for a in range(10)) and np.isfinite(got["diffuseness"][heard]).any()


def test_the_rate_tool_runs_and_its_outputs_equal_the_definition(tmp_path):
    """tools/lateral_rate.py on a 48 x 48 x 16 room, 48 steps per repeat, two repeats: every row is there, the lateral plan's outputs
    equal lateral.lateral_fold over the hull snapshots bytewise, the model of the steady row is the hand-derived one, and the figures land
    in the JSON file."""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "lateral_rate.py"), "--dims", "48,48,16",
                        "--steps", "48", "--periods", "1,8", "--repeats", "2", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and "bytewise equal" in p.stdout and "LATERAL RATE OK" in p.stdout, p.stdout
    report = json.load(open(str(out)))
    assert report["f64"]["bytewise_equal"] is True
    # the steady row's model over the intensity plan's, by hand: 48 captures are three folds of 16; the first finds every onset (at
    # capture 0: `pre` there and back and the onset's store, 16 t + 72) and passes through bins 0 and 1: 256 + 72 + 320 = 648 B per
    # node; the others stay in the last bin: 256 + 52 + 160 = 468; against 256 + 48 + 64 = 368 each.  6 captures are one fold, the
    # onset in it, one bin: 96 + 72 + 160 = 328 against 96 + 48 + 64 = 208
    for period, captures, steady_model in ((1, 48, (648 + 468 + 468) / 3 / 368), (8, 6, 328 / 208)):
        rows = report["f64"]["every %d" % period]
        assert sorted(rows["rows"]) == ["intensity", "lateral", "lateral steady", "none"] and rows["captures"] == captures
        for name in ("lateral", "lateral steady"):
            row = rows["rows"][name]
            assert row["folds"] >= 1 and row["mean_fold_ms"] > 0 and row["gathers"] == captures and row["fetch_seconds_median"] > 0
            assert row["fetch_bytes"] == 46 * 46 * (36 + 80 * 3)
        assert rows["rows"]["lateral steady"]["nodes_with_an_onset_at_the_end"] == 46 * 46
        assert rows["rows"]["lateral"]["nodes_with_an_onset_at_the_end"] <= 46 * 46
        assert abs(rows["over_intensity"]["lateral steady"]["per_fold_model"] - steady_model) < 1e-12

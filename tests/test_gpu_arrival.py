"""Arrival-aligned energy maps: onset, peak and energy binned from each node's own arrival, accumulated on the device while wv_run keeps
going (wv_set_arrival; csrc/arrival_kernels.hip.h, engine_arrival.hip.h).  The reference of every comparison is a second, identical
engine with a SNAPSHOT plan of the same box and cadence, whose snapshots arrival.arrival_fold -- the definition in NumPy -- folds in
capture order.  Equality is BYTEWISE on all six outputs.  Small meshes, forms forced, a few dozen steps."""
import numpy as np
import pytest

import cases
from helpers import set_tuning
from plan_cases import (BOXES, FILE_FORMS, FORMS, FORM_QUERIES, box_scene, changes_nothing, check, default_tuning_afterwards, make_engine,
                        median_threshold, plan_engine, plan_on, reference_snapshots, scaled_map)
from wayverb_amd import arrival as A
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def arrival_plan(case, cadence, edges, threshold=median_threshold, map_factors=None):
    """`threshold`: a number, or a callable(snaps, plan) of the reference's snapshots; `map_factors`: a per-node map of that many times it."""
    if map_factors is not None:
        return plan_on(case, "arrival", edges=list(edges), threshold=0.0, threshold_map=scaled_map(threshold, map_factors), **cadence)
    return plan_on(case, "arrival", edges=list(edges), threshold=threshold, **cadence)


def same(got, want):
    for key in A.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), "%s differs at %d nodes" % (key, (got[key] != want[key]).sum())


@pytest.mark.parametrize("period", range(1, 8))
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_fold_of_the_snapshots(form, period, tag):
    """Single steps, graph replay, two- and three-step passes at periods 1 .. 7: one plane of the 32^3 impulse room, 30 steps (64 under
    graph replay).  The threshold is the median of the reference snapshots' per-node max |p|, so about half of the nodes hear an
    onset and the wavefront puts them into different captures; the bins begin 0, 1 and 3 captures behind each node's own onset.

    At an EVEN period that median is exactly 0, whatever computes the field: an impulse on the rectilinear mesh alternates between the
    two colours of the checkerboard, so captures an even number of steps apart never see one colour move, and with the shell of
    outside nodes more than half of the plane's nodes hold 0 throughout.  A threshold of 0 is legal and is compared as it is (every
    onset is capture 0), but it cannot show a quarter of the nodes without an onset.  Those periods are therefore compared a second
    time with the lower quartile of the NON-ZERO per-node maxima as the threshold (340 of 1024 nodes hear an onset on the CPU
    restatement), where all four conditions are asserted as at the odd periods."""
    n_steps = 64 if form == "graph" else 30
    # (a pass form shows in its counter only where the period leaves room for a pass of that length)
    query = FORM_QUERIES[form] if (form == "pair" and period >= 2) or (form == "triple" and period >= 3) else None
    plan = dict(box=((0, 0, 15), (None, None, 1)), period=period)
    got, want, _, snaps, _ = check("arrival", "impulse_flat", tag, form, arrival_plan("impulse_flat", plan, (0, 1, 3)), n_steps, query,
                                   **({} if period % 2 == 1 else dict(condition=None)))
    if period % 2 == 1:
        assert median_threshold(snaps) > 0
    else:
        assert median_threshold(snaps) == 0 and (want["onset"] == 0).all() and (want["bins"].reshape(3, -1).max(axis=1) > 0).sum() >= 2

        def lower_quartile(snaps, plan):
            highest = np.abs(snaps).max(axis=0)
            return np.float32(np.quantile(highest[highest > 0], 0.25))
        check("arrival", "impulse_flat", tag, form, arrival_plan("impulse_flat", plan, (0, 1, 3), lower_quartile), n_steps)


def _random_factors(shape):
    return 10.0 ** np.random.default_rng(42).uniform(-1, 1, shape)


@pytest.mark.parametrize("with_map", [False, True], ids=["scalar", "map"])
@pytest.mark.parametrize("name", sorted(BOXES))
def test_boxes_and_strides_on_a_room_with_walls(name, with_map):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source, noise in the field from the start;
    every step captured, 33 captures (16 + 16 + 1), edges (0, 1, 5, 16, 17): an edge inside a fold, one on a fold's first slot and
    one behind it.  Once with the scalar median threshold, once with a per-node map of 0.1 .. 10 times that median.  (One node has no
    quarter of nodes to show: the box of one node is compared as it is.)"""
    plan = arrival_plan("random", dict(BOXES[name], period=1), (0, 1, 5, 16, 17), map_factors=_random_factors if with_map else None)
    check("arrival", "random", "f64", "triple", plan, 32, **(dict(condition=None) if name == "one-node" else {}))


@pytest.mark.parametrize("w,n_bins", [(1, 16), (5, 7), (16, 3), (40, 2)])
def test_threshold_zero_and_even_edges_equal_the_decay_plan(w, n_bins):
    """Every onset is capture 0: the bins are a plain decay plan's of the same box and cadence, bytewise -- the merged fold and the new
    one on the same captures."""
    plan = dict(BOXES["sub-box-567-odd"], period=1)
    edges = [k * w for k in range(n_bins)]
    got = check("arrival", "random", "f64", "pair", arrival_plan("random", plan, edges, 0.0), 32, condition=None)[0]
    set_tuning(**FORMS["pair"])
    eng = make_engine(cases.CASES["random"](), "f64")
    eng.set_decay(n_bins, w, **plan)
    try:
        assert eng.run_steps(32) == (32, 0)
        bins, captures = eng.fetch_decay()
    finally:
        eng.close()
    assert captures == 33 and got["bins"].tobytes() == bins.tobytes() and bins.max() > 0
    assert (got["onset"] == 0).all() and got["pre"].tobytes() == np.zeros(got["pre"].shape).tobytes()


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_no_onset_is_earlier_than_the_stencil_can_carry_it(tag):
    """The 32^3 impulse room, the whole mesh, threshold 1e-30, 20 steps: the stencil moves information one node per step, so the step
    of a node's onset is at least its Manhattan distance from the source node plus the step of the source's first non-zero sample
    (0), and nodes farther away than the run is long have no onset and a peak of exactly 0.  The bound is tight: a hard source's
    sample of step 0 is in its six neighbours after one step, so some node attains it to within one step."""
    n_steps = 20
    case = cases.CASES["impulse_flat"]()
    first_sample = int(np.flatnonzero(case["signal"])[0])
    eng = plan_engine("impulse_flat", tag, "triple", arrival_plan("impulse_flat", dict(box="mesh", period=1), (0, 8), 1e-30))
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        got, captures = eng.fetch_arrival()
    finally:
        eng.close()
    assert captures == n_steps + 1
    z, y, x = np.meshgrid(*(np.arange(32),) * 3, indexing="ij")
    distance = np.abs(x - 16) + np.abs(y - 16) + np.abs(z - 16)
    heard = got["onset"] != A.NONE
    onset_step = got["onset"].astype(np.int64)          # first_step 0, period 1
    assert heard.sum() > 1000
    assert (onset_step[heard] >= distance[heard] + first_sample).all()
    assert (onset_step[heard] - distance[heard] - first_sample).min() <= 1
    far = distance > n_steps
    assert far.sum() > 1000 and not heard[far].any() and (got["peak"][far] == 0).all() and (got["peak_capture"][far] == A.NONE).all()
    assert (got["pre"][~heard] == 0).all() and (got["peak"][heard] > 0).all()


def test_refusals_leave_an_earlier_plan_intact():
    """Bad n_bins, edges, thresholds, strides, period and boxes: WV_E_INVALID_ARGUMENT; each of the four other plans while an arrival
    plan is active and an arrival plan while each of them is: WV_E_STATE with the plan to stop in the message; a slab: WV_E_STATE.
    After the refusals the earlier plan's results are what they were and it goes on capturing."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(BOXES["sub-box-630"], period=1)
    edges = (0, 1, 5)
    snaps, _ = reference_snapshots("random", "f64", "single", plan, 32)
    thr = median_threshold(snaps)
    intensity = dict(box=((1, 1, 1), (4, 4, 4)), spacing=0.05, sample_rate=8000.0, ambient_density=1.2)
    eng = make_engine(case, "f64")
    try:
        eng.set_arrival(edges, thr, **plan)
        assert eng.run_steps(5) == (5, 0)
        before, before_count = eng.fetch_arrival()
        for bad in ((), tuple(range(17)), (1, 2), (0, 5, 5), (0, 5, 4)):
            with pytest.raises((E.WaveguideError, ValueError), match="error -1: .*(n_bins|edges)|16 bins"):
                eng.set_arrival(bad, thr, **plan)
        for bad in (-1.0, np.inf, np.nan):
            with pytest.raises(E.WaveguideError, match="error -1: .*threshold"):
                eng.set_arrival(edges, bad, **plan)
        bad_map = np.full((7, 9, 10), thr, np.float32)
        bad_map[3, 4, 5] = -thr
        with pytest.raises(E.WaveguideError, match="error -1: .*threshold map"):
            eng.set_arrival(edges, thr, threshold_map=bad_map, **plan)
        for bad_box in (((0, 0, 0), (25, 20, 28)), ((-1, 0, 0), (4, 4, 4)), ((0, 0, 28), (1, 1, 1))):
            with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
                eng.set_arrival(edges, thr, box=bad_box)
        with pytest.raises(E.WaveguideError, match="error -1: .*stride"):
            eng.set_arrival(edges, thr, box="mesh", stride=(1, 0, 1))
        with pytest.raises(E.WaveguideError, match="error -1: .*period"):
            eng.set_arrival(edges, thr, box="mesh", period=0)
        stop = r"error -6: .*an arrival plan is active \(wv_set_arrival\(e, NULL, NULL\)"
        with pytest.raises(E.WaveguideError, match=stop):
            eng.set_snapshots(**plan)
        with pytest.raises(E.WaveguideError, match=stop):
            eng.set_spectrum([0.1], **plan)
        with pytest.raises(E.WaveguideError, match=stop):
            eng.set_decay(4, 2, **plan)
        with pytest.raises(E.WaveguideError, match=stop):
            eng.set_decay(4, 2, bands=np.array([[[1.0, 0, 0, 0, 0]]]), **plan)
        with pytest.raises(E.WaveguideError, match=stop):
            eng.set_intensity(2, 2, **intensity)
        after, after_count = eng.fetch_arrival()
        assert after_count == before_count == 6
        same(after, before)
        same(after, A.arrival_fold(snaps[:6], thr, edges))
        assert eng.run_steps(3) == (3, 0) and eng.arrival_count() == (9, 8)
        same(eng.fetch_arrival()[0], A.arrival_fold(snaps[:9], thr, edges))
    finally:
        eng.close()
    # the other way round: each of the four other plans refuses an arrival plan, and goes on
    others = [("snapshot", lambda e: e.set_snapshots(**plan), lambda e: e.snapshot_count()[0] == 5),
              ("spectrum", lambda e: e.set_spectrum([0.0], **plan), lambda e: e.spectrum_count() == (5, 4)),
              ("decay", lambda e: e.set_decay(4, 2, **plan), lambda e: e.decay_count() == (5, 4)),
              ("intensity", lambda e: e.set_intensity(2, 2, **intensity), lambda e: e.intensity_count() == (5, 4))]
    for name, set_other, went_on in others:
        eng = make_engine(case, "f64")
        try:
            set_other(eng)
            assert eng.run_steps(2) == (2, 0)
            with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_arrival: an? (banded )?%s plan is active \(wv_set_" % name):
                eng.set_arrival(edges, thr, **plan)
            assert eng.run_steps(2) == (2, 0) and went_on(eng)
        finally:
            eng.close()
    # a slab of a chain; no plan; a group takes no engine with a plan
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    try:
        with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
            slab.set_arrival((0, 2), 0.1, box=((0, 0, 0), (4, 4, 1)))
    finally:
        slab.close()
    eng = E.Engine(mesh, precision="f32")
    group = E.LocalSlabGroup([eng])
    try:
        eng.set_arrival((0, 2), 0.1, box=((0, 0, 0), (4, 4, 1)))
        with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no arrival maps"):
            group.run_steps(4)
        eng.set_arrival(None)
        assert group.run_steps(4) == (4, 0)
    finally:
        group.close()


@pytest.mark.parametrize("form", FILE_FORMS["arrival"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("arrival", tag, form)


def test_canonical_returns_the_maps_beside_the_receiver_output():
    """simulation.canonical(..., arrival=...): the records are those of a run without a plan, the state is the engine-level one
    (folded from canonical's own snapshots of the same plane and cadence)."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    plane_z = 12 * vm.mesh.spacing
    early_ms = (6e3 / rate, 10e3 / rate)         # 6 and 10 steps: 3 and 5 captures at every=2
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                         snapshots=dict(box=((0, 0, 12), (None, None, 1)), period=2))
    bands, (out, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                         arrival=dict(plane=plane_z, every=2, threshold=1e-4, early_ms=early_ms))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 21 and out["bins"].shape == (3, 1, 24, 24)
    want = A.arrival_fold(fields, np.float32(1e-4), (0, 3, 5))
    same(out, want)
    assert (want["onset"] != A.NONE).any() and len(set(want["onset"].ravel().tolist())) >= 3
    with pytest.raises(E.WaveguideError, match="error -6: .*snapshot plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, snapshots=dict(period=8), arrival=dict(plane=plane_z, threshold=1e-4))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, arrival=dict(plane=plane_z, threshold=1e-4))


def test_the_tool_writes_the_clarity_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --clarity-map --arrival-plane z=... --arrival-out FILE.npz on its built-in hall, a short run."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "arrival.npz"
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.1",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--clarity-map", "--arrival-plane", "z=1.5",
                        "--arrival-threshold", "1e-5", "--arrival-out", str(out)], capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        got = {k: f[k] for k in f.files}
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    rate = float(got["sample_rate"])
    assert got["bins"].shape == (3, dims[1], dims[0]) and got["onset"].shape == got["c80_db"].shape == got["ts_s"].shape == (dims[1], dims[0])
    assert list(got["edges"]) == A.edges_from_ms((50, 80), 1, rate) and int(got["captures"]) == steps + 1
    heard = got["onset"] != A.NONE
    assert heard.any() and np.isfinite(got["arrival_s"][heard]).all() and np.isnan(got["arrival_s"][~heard]).all()
    assert (got["arrival_s"][heard] >= 0).all() and (got["arrival_s"][heard] <= steps / rate).all()
    assert got["bins"][0].max() > 0 and np.isfinite(got["direct_db"][heard]).all() and (got["ts_s"][heard] >= 0).all()


def test_the_rate_tool_runs_and_its_outputs_equal_the_definition(tmp_path):
    """tools/arrival_rate.py on a 48 x 48 x 16 room, 48 steps per repeat, two repeats: every row is there, the arrival plan's outputs
    equal arrival.arrival_fold over the snapshots bytewise, and the figures land in the JSON file."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "arrival_rate.py"), "--dims", "48,48,16",
                        "--steps", "48", "--periods", "1,8", "--repeats", "2", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and "bytewise equal" in p.stdout and "ARRIVAL RATE OK" in p.stdout, p.stdout
    report = json.load(open(str(out)))
    assert report["f64"]["bytewise_equal"] is True
    for period, captures in ((1, 48), (8, 6)):
        rows = report["f64"]["every %d" % period]
        assert sorted(rows["rows"]) == ["arrival", "decay", "none"] and rows["captures"] == captures
        assert rows["rows"]["arrival"]["folds"] >= 1 and rows["rows"]["arrival"]["mean_fold_ms"] > 0

"""Intensity maps: time-binned sound intensity of a box accumulated on the device while wv_run keeps going (wv_set_intensity;
csrc/intensity_kernels.hip.h, engine_intensity.hip.h).  The reference of every comparison is a second, identical engine with a SNAPSHOT
plan of the box's HULL at stride 1 and the same cadence, whose snapshots go through intensity.intensity_bins -- the definition, the
float lines on float32 arrays and the rest on float64.  Bins AND velocities are compared BYTEWISE, and every comparison also asserts
that all four planes hold something non-zero.  Small meshes, forms forced, a few dozen steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import set_tuning
from test_gpu_decay import LAYOUTS, reference_snapshots
from test_gpu_decay_bands import FORM_CASES
from test_gpu_snapshots import FORMS, make_engine
from test_receiver_arrays_host import canonical_parameters
from wayverb_amd import engine as E
from wayverb_amd import intensity as I
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACING, RATE, DENSITY = canonical_parameters()


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


def constants(plan):
    """The integrator sees a series sampled every `period` steps: that rate."""
    return dict(spacing=SPACING, sample_rate=RATE / plan.get("period", 1), ambient_density=DENSITY)


def hull_of(plan):
    """plan: box = ((x0, y0, z0), extent in mesh nodes), stride, period, first_step -> the snapshot plan of the box's hull at stride 1
    and the same cadence, and the slices that pick the taken nodes out of a hull snapshot."""
    origin, extent = plan["box"]
    stride = plan.get("stride", 1)
    stride = (stride,) * 3 if np.isscalar(stride) else tuple(stride)
    taken = tuple((e + s - 1) // s for e, s in zip(extent, stride))
    hull, box_in_hull = I.hull_box((origin, taken), stride)
    hplan = dict(box=hull, period=plan.get("period", 1))
    if "first_step" in plan:
        hplan["first_step"] = plan["first_step"]
    return hplan, box_in_hull


def definition(snaps, plan, n_bins, w, **more):
    _, box_in_hull = hull_of(plan)
    c = constants(plan)
    return I.intensity_bins(snaps, box_in_hull, c["spacing"], c["sample_rate"], c["ambient_density"], n_bins, w, return_velocity=True, **more)


def intensity_engine(case, tag, form, plan, n_bins, w):
    set_tuning(**FORMS[form])
    eng = make_engine(cases.CASES[case]() if isinstance(case, str) else case, tag)
    shape = eng.set_intensity(n_bins, w, **plan, **constants(plan))
    return eng, shape


def nonzero(bins, velocity):
    return all(np.abs(bins[a]).max() > 0 for a in range(4)) and all(np.abs(velocity[a]).max() > 0 for a in range(3))


def check(case_name, tag, form, plan, n_bins, w, n_steps, query=None):
    hplan, _ = hull_of(plan)
    snaps, steps = reference_snapshots(case_name, tag, form, hplan, n_steps)
    want, want_v = definition(snaps, plan, n_bins, w)
    eng, shape = intensity_engine(case_name, tag, form, plan, n_bins, w)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert eng.intensity_count() == (len(steps), int(steps[-1]))
        got, captures = eng.fetch_intensity()
        got_v = eng.fetch_intensity_velocity()
        if query is not None:
            assert eng.query(query) > 0
        assert eng.query(E.Engine.QUERY_INTENSITY_CAPTURES) == len(steps)
        folds = eng.query(E.Engine.QUERY_INTENSITY_FOLDS)
    finally:
        eng.close()
    assert captures == len(steps)
    assert got.shape == shape == want.shape and got.dtype == np.float64 and got_v.shape == want_v.shape
    assert folds <= -(-len(steps) // 16) + 1
    assert got.tobytes() == want.tobytes(), "largest difference %g" % np.abs(got - want).max()
    assert got_v.tobytes() == want_v.tobytes(), "largest difference %g" % np.abs(got_v - want_v).max()
    assert nonzero(got, got_v)      # (the comparison is not of zeros)
    return got, got_v, snaps


PLANE = dict(box=((1, 1, 15), (30, 30, 1)))


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_bins_of_the_hull_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes; period 1 (every step ends a pass), 3 (three-step passes stay whole) and 7;
    the plane z = 15 of the 32^3 impulse room less its rim, four captures per bin."""
    n_steps = 64 if form == "graph" else 30
    captures = n_steps // period + 1
    check("impulse_flat", tag, form, dict(PLANE, period=period), -(-captures // 4), 4, n_steps, query)


BOXES = {
    "sub-box-630": dict(box=((3, 2, 4), (10, 9, 7))),             # not a multiple of 64, three workgroups of the fold, a tail
    "sub-box-567-odd": dict(box=((3, 2, 4), (9, 9, 7))),
    "sub-box-16-byte-rows": dict(box=((4, 1, 2), (16, 5, 3))),
    "strides-1-2-3": dict(box=((1, 1, 2), (21, 18, 24)), stride=(1, 2, 3)),
    "interior-stride-3": dict(box=((1, 1, 1), (22, 18, 26)), stride=3),
    "one-node": dict(box=((5, 6, 7), (1, 1, 1))),
    "hull-touches-every-face": dict(box=((1, 1, 1), (22, 18, 26))),   # the neighbours of the outermost nodes are wall nodes
}


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; every step captured, 21 captures (16 in
    the first fold, 5 in the second, which starts from the velocities the first one stored), three captures per bin."""
    got, _, _ = check("random", tag, "triple", dict(BOXES[name], period=1), 7, 3, 20)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_bin_layouts_against_the_stage(name, layout):
    n_bins, w = LAYOUTS[layout]
    got, _, _ = check("random", "f64", "pair", dict(BOXES[name], period=1), n_bins, w, 32)
    if layout == "more-bins-than-captures":
        assert (got[:, 33:] == 0).all() and not np.signbit(got[:, 33:]).any()    # never touched: +0.0


@pytest.mark.parametrize("captures", [1, 16, 17, 33])
def test_capture_counts_around_the_stage(captures):
    """Runs that take exactly 1, 16, 17 and 33 captures: one fold per 16 captures and one for the fetch at the most."""
    n_steps = captures - 1
    plan = dict(BOXES["sub-box-630"], period=1)
    eng, _ = intensity_engine("random", "f64", "single", plan, 5, 5)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert eng.intensity_count() == (captures, n_steps)
        assert eng.query(E.Engine.QUERY_INTENSITY_FOLDS) <= (captures - 1) // 16   # (nothing is folded merely because a run ended)
        got, count = eng.fetch_intensity()
        got_v = eng.fetch_intensity_velocity()
        assert count == captures == eng.query(E.Engine.QUERY_INTENSITY_CAPTURES)
        assert eng.query(E.Engine.QUERY_INTENSITY_FOLDS) <= -(-captures // 16) + 1
    finally:
        eng.close()
    snaps, _ = reference_snapshots("random", "f64", "single", hull_of(plan)[0], 32)
    want, want_v = definition(snaps[:captures], plan, 5, 5)
    assert got.tobytes() == want.tobytes() and got_v.tobytes() == want_v.tobytes() and nonzero(got, got_v)


def test_fetching_mid_run_and_at_the_end():
    plan = dict(BOXES["sub-box-630"], period=1)
    eng, _ = intensity_engine("random", "f64", "pair", plan, 6, 5)
    assert eng.run_steps(13) == (13, 0)
    mid, mid_count = eng.fetch_intensity()
    mid_v = eng.fetch_intensity_velocity()
    again, again_count = eng.fetch_intensity()
    assert eng.run_steps(17) == (17, 0)
    end, end_count = eng.fetch_intensity()
    end_v = eng.fetch_intensity_velocity()
    eng.close()
    snaps, _ = reference_snapshots("random", "f64", "pair", hull_of(plan)[0], 30)
    assert (mid_count, again_count, end_count) == (14, 14, 31)
    want_mid, want_mid_v = definition(snaps[:14], plan, 6, 5)
    want_end, want_end_v = definition(snaps, plan, 6, 5)
    assert mid.tobytes() == again.tobytes() == want_mid.tobytes() and mid_v.tobytes() == want_mid_v.tobytes()
    assert end.tobytes() == want_end.tobytes() and end_v.tobytes() == want_end_v.tobytes() and nonzero(end, end_v)
    assert (end[:, :2] == mid[:, :2]).all() and (end[3, 2] >= mid[3, 2]).all()       # full bins stay, the bin in progress grows


def test_the_energy_planes_are_a_plain_decay_plans_bins():
    plan = dict(BOXES["strides-1-2-3"], period=2)
    got, _, _ = check("random", "f64", "triple", plan, 4, 3, 30)
    set_tuning(**FORMS["triple"])
    eng = make_engine(cases.CASES["random"](), "f64")
    eng.set_decay(4, 3, **plan)
    assert eng.run_steps(30) == (30, 0)
    decay, count = eng.fetch_decay()
    eng.close()
    assert count == 16 and got[3].tobytes() == decay.tobytes() and decay.max() > 0


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_the_receiver_path_carries_the_same_velocities(tag):
    """Four nodes whose 7-point hull does not hold the source node, period 1, first_step 0: the directional receivers' float records
    are (float)(v * p) of the definition's velocities, step by step -- so their sums in double per bin are the definition's sums of
    the rounded products -- and the velocities the receiver path carries after the run equal the plan's, bytewise."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    mesh = case["mesh"]
    sx, sy, sz = mesh.compute_locator(case["source_node"])
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    picks = [(x, y, z) for (x, y, z) in ((3, 2, 4), (12, 10, 10), (7, 6, 5), (4, 10, 9)) if abs(x - sx) + abs(y - sy) + abs(z - sz) > 1]
    assert len(picks) == 4, "the case's source moved next to a picked node"
    n = 24
    recv = make_engine(case, tag)
    recv.set_directional_receivers([mesh.compute_index(*p) for p in picks], SPACING, RATE, DENSITY)
    assert recv.run_steps(n) == (n, 0)                      # records of steps 0 .. n - 1
    records = recv.fetch_directional(0, n)
    recv_v = recv.fetch_directional_velocity(4)
    recv.close()
    eng, _ = intensity_engine(case, tag, "pair", plan, 6, 4)
    assert eng.run_steps(n - 1) == (n - 1, 0)               # captures of steps 0 .. n - 1
    assert eng.intensity_count() == (n, n - 1)
    got, _ = eng.fetch_intensity()
    got_v = eng.fetch_intensity_velocity()
    eng.close()
    snaps, _ = reference_snapshots("random", tag, "pair", hull_of(plan)[0], 32)
    want, want_v = definition(snaps[:n], plan, 6, 4)
    assert got.tobytes() == want.tobytes() and got_v.tobytes() == want_v.tobytes()
    v = None
    sums = np.zeros((3, 6, 4))
    for j in range(n):
        _, v = definition(snaps[j:j + 1], plan, 1, 1, velocity=v, first_capture=j)
        for r, (x, y, z) in enumerate(picks):
            at = (z - 4, y - 2, x - 3)
            p = snaps[j][at[0] + 1, at[1] + 1, at[2] + 1]
            rounded = (v[(slice(None),) + at] * np.float64(p)).astype(np.float32)
            assert records[j, r]["pressure"].tobytes() == p.tobytes()
            assert records[j, r]["intensity"].tobytes() == rounded.tobytes(), (j, r)
            sums[:, min(j // 4, 5), r] = sums[:, min(j // 4, 5), r] + rounded.astype(np.float64)
    per_bin = np.zeros((3, 6, 4))
    for j in range(n):
        per_bin[:, min(j // 4, 5), :] = per_bin[:, min(j // 4, 5), :] + records["intensity"][j].astype(np.float64).T
    assert per_bin.tobytes() == sums.tobytes() and np.abs(sums).min() > 0
    for r, (x, y, z) in enumerate(picks):
        assert recv_v[r].tobytes() == got_v[:, z - 4, y - 2, x - 3].tobytes()
    assert np.abs(recv_v).min() > 0


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("bad_step", [12, 13, 14])
def test_a_run_that_stops_on_a_flag_folds_no_capture_of_a_later_step(form, bad_step):
    """inf in the source signal at step f: the run completes f steps; with a capture every 4 steps bins and velocities have seen those
    of 0, 4, 8, 12 and nothing of 16 (whose field the batch had already produced when the flag was read).  A following run goes on
    from there."""
    set_tuning(**FORMS[form])
    mesh = M.box_mesh(12, 12, 12)
    sig = np.zeros(40)
    sig[0], sig[1] = 1.0, 0.5     # (both parities of the mesh: after an impulse alone a node and its neighbours are never non-zero at the same step, and I is 0)
    sig[bad_step] = np.inf
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=sig,
                recv=[mesh.compute_index(7, 6, 6)])
    plan = dict(box=((1, 1, 5), (10, 10, 1)), period=4)
    engines = [make_engine(case, "f64", hull_of(plan)[0]), make_engine(case, "f64")]
    engines[1].set_intensity(3, 2, **plan, **constants(plan))
    memories = [engines[0].read_boundary_data(d) for d in (1, 2, 3)]
    for eng in engines:
        done, flag = eng.run_steps(40)
        assert done == bad_step and flag & M.ERR_INF
    snaps, steps = engines[0].fetch_snapshots()
    assert list(steps) == [0, 4, 8, 12]
    assert engines[1].intensity_count() == (4, 12)
    got, count = engines[1].fetch_intensity()
    got_v = engines[1].fetch_intensity_velocity()
    want, want_v = definition(snaps, plan, 3, 2)
    assert count == 4 and np.isfinite(got).all() and np.isfinite(got_v).all() and nonzero(got, got_v)
    assert got.tobytes() == want.tobytes() and got_v.tobytes() == want_v.tobytes()
    # the next run continues: the failed steps left inf / nan behind, so both engines get the same finite fields, clean filter memories
    # and a finite source; the capture of step 16, dropped above, is due again and the plan goes on counting from capture 4
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
    assert list(steps) == [0, 4, 8, 12, 16, 20] and engines[1].intensity_count() == (6, 20)
    got, count = engines[1].fetch_intensity()
    got_v = engines[1].fetch_intensity_velocity()
    for eng in engines:
        eng.close()
    want, want_v = definition(snaps, plan, 3, 2)
    assert count == 6 and np.isfinite(got).all() and got[3, 2].max() > 0
    assert got.tobytes() == want.tobytes() and got_v.tobytes() == want_v.tobytes()


@pytest.mark.parametrize("form", ["single", "triple"])
def test_checkpoint_run_rollback_rerun_gives_the_same_bins_twice(form):
    plan = dict(box=((2, 3, 4), (12, 11, 9)), stride=(1, 2, 2), period=5)
    eng, _ = intensity_engine("random", "f64", form, plan, 3, 2)
    assert eng.run_steps(10) == (10, 0)            # captures of 0, 5, 10
    eng.checkpoint()
    assert eng.run_steps(17) == (17, 0)            # 15, 20, 25
    first, first_count = eng.fetch_intensity()
    first_v = eng.fetch_intensity_velocity()
    eng.rollback()
    assert eng.step_count() == 10 and eng.intensity_count() == (3, 10)
    kept, kept_count = eng.fetch_intensity()
    kept_v = eng.fetch_intensity_velocity()
    assert eng.run_steps(17) == (17, 0)
    second, second_count = eng.fetch_intensity()
    second_v = eng.fetch_intensity_velocity()
    assert eng.intensity_count() == (6, 25)
    # a plan set after the checkpoint has no bins to go back to
    eng.set_intensity(3, 2, **plan, **constants(plan))
    with pytest.raises(E.WaveguideError, match="error -6: .*intensity plan was set after the checkpoint"):
        eng.rollback()
    eng.close()
    snaps, _ = reference_snapshots("random", "f64", form, hull_of(plan)[0], 27)
    assert (first_count, kept_count, second_count) == (6, 3, 6)
    want_kept, want_kept_v = definition(snaps[:3], plan, 3, 2)
    want, want_v = definition(snaps, plan, 3, 2)
    assert kept.tobytes() == want_kept.tobytes() and kept_v.tobytes() == want_kept_v.tobytes()
    assert first.tobytes() == second.tobytes() == want.tobytes() and first_v.tobytes() == second_v.tobytes() == want_v.tobytes()
    assert nonzero(first, first_v)


def test_generic_steps_in_between_capture_nothing():
    """wv_step / wv_swap capture nothing and the plan steps they pass are gaps in the series; a plan set at a non-zero step count
    captures that very step at the next run."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    plan = dict(box=((1, 1, 1), (22, 18, 2)), period=3)
    engines = [make_engine(case, "f32"), make_engine(case, "f32")]
    for e in engines:
        assert e.run_steps(9) == (9, 0)
    engines[0].set_intensity(2, 2, **plan, **constants(plan))   # steps 0, 3, 6 lie before the plan; 9 is the count it is set at
    engines[1].set_snapshots(**hull_of(plan)[0])
    assert engines[0].intensity_count() == (0, 0)
    for e in engines:
        assert e.run_steps(4) == (4, 0)               # 9 (at the start of this run), 12
        for _ in range(3):                            # 13 -> 16 by generic steps: 15 is passed
            assert e.step() == 0
            e.swap()
    assert engines[0].intensity_count() == (2, 12)
    for e in engines:
        assert e.run_steps(2) == (2, 0)               # 18
    got, count = engines[0].fetch_intensity()
    got_v = engines[0].fetch_intensity_velocity()
    snaps, steps = engines[1].fetch_snapshots()
    want, want_v = definition(snaps, plan, 2, 2)
    assert list(steps) == [9, 12, 18] and count == 3
    assert got.tobytes() == want.tobytes() and got_v.tobytes() == want_v.tobytes() and nonzero(got, got_v)
    engines[0].set_intensity(None)                    # stops and forgets
    with pytest.raises(E.WaveguideError, match="error -6: .*no intensity plan"):
        engines[0].intensity_count()
    assert engines[0].run_steps(3) == (3, 0)
    for e in engines:
        e.close()


def test_refusals_leave_an_earlier_plan_intact_and_the_plans_exclude_each_other():
    """Every WV_E_INVALID_ARGUMENT leaves the running plan as it was; the five setters refuse each other with the plan to stop in the
    message; a slab of a chain and wv_run_group refuse."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(BOXES["sub-box-630"], period=1)
    c = constants(plan)
    snaps, _ = reference_snapshots("random", "f64", "single", hull_of(plan)[0], 32)
    eng = make_engine(case, "f64")
    eng.set_intensity(4, 2, **plan, **c)
    assert eng.run_steps(5) == (5, 0)
    before, before_count = eng.fetch_intensity()
    for n_bins, w in ((0, 1), (4097, 1), (4, 0)):
        with pytest.raises(E.WaveguideError, match="error -1: .*(n_bins|bin_captures)"):
            eng.set_intensity(n_bins, w, **plan, **c)
    for bad_box in (((1, 1, 1), (24, 18, 26)), ((-1, 1, 1), (4, 4, 4)), ((1, 1, 28), (1, 1, 1))):
        with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
            eng.set_intensity(4, 2, box=bad_box, **c)
    for edge_box in (((0, 1, 1), (4, 4, 4)), ((1, 0, 1), (4, 4, 4)), ((1, 1, 0), (4, 4, 4)), ((1, 1, 1), (23, 4, 4)), ((1, 1, 1), (4, 19, 4)),
                     ((1, 1, 1), (4, 4, 27))):
        with pytest.raises(E.WaveguideError, match="error -1: Can't place directional_receiver at this node as it is adjacent to a boundary."):
            eng.set_intensity(4, 2, box=edge_box, **c)
    with pytest.raises(E.WaveguideError, match="error -1: .*stride"):
        eng.set_intensity(4, 2, stride=(1, 0, 1), **c)
    with pytest.raises(E.WaveguideError, match="error -1: .*period"):
        eng.set_intensity(4, 2, period=0, **c)
    for bad in (dict(c, spacing=0.0), dict(c, sample_rate=-1.0), dict(c, ambient_density=float("inf")), dict(c, spacing=float("nan"))):
        with pytest.raises(E.WaveguideError, match="error -1: .*positive and finite"):
            eng.set_intensity(4, 2, **plan, **bad)
    snapshot_plan = dict(box=plan["box"], period=1)
    bands = np.array([[[1.0, 0, 0, 0, 0]]])
    stop = r"error -6: .*intensity plan is active \(wv_set_intensity\(e, NULL\)"
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_snapshots(**snapshot_plan)
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_spectrum([0.1], **snapshot_plan)
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_decay(4, 2, **snapshot_plan)
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_decay(4, 2, bands=bands, **snapshot_plan)
    after, after_count = eng.fetch_intensity()
    assert after_count == before_count == 6 and after.tobytes() == before.tobytes() == definition(snaps[:6], plan, 4, 2)[0].tobytes()
    assert eng.run_steps(3) == (3, 0) and eng.intensity_count() == (9, 8)
    want, want_v = definition(snaps[:9], plan, 4, 2)
    assert eng.fetch_intensity()[0].tobytes() == want.tobytes() and eng.fetch_intensity_velocity().tobytes() == want_v.tobytes()
    assert nonzero(want, want_v)
    eng.close()
    # the other orders: each of the four other plans is active
    for setter, stop in ((lambda e: e.set_snapshots(**snapshot_plan), r"snapshot plan is active \(wv_set_snapshots\(e, NULL\)"),
                         (lambda e: e.set_spectrum([0.0], **snapshot_plan), r"spectrum plan is active \(wv_set_spectrum\(e, NULL, NULL\)"),
                         (lambda e: e.set_decay(4, 2, **snapshot_plan), r"a decay plan is active \(wv_set_decay\(e, NULL\)"),
                         (lambda e: e.set_decay(4, 2, bands=bands, **snapshot_plan), r"banded decay plan is active \(wv_set_decay_bands\(e, NULL, NULL, 0, 0\)")):
        eng = make_engine(case, "f64")
        setter(eng)
        assert eng.run_steps(2) == (2, 0)
        with pytest.raises(E.WaveguideError, match="error -6: wv_set_intensity: .*" + stop):
            eng.set_intensity(4, 2, **plan, **c)
        with pytest.raises(E.WaveguideError, match="error -6: .*no intensity plan"):
            eng.fetch_intensity()
        assert eng.run_steps(2) == (2, 0)
        eng.close()
    # a slab of a chain
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
        slab.set_intensity(2, 2, box=((1, 1, 1), (4, 4, 1)), **c)
    slab.close()
    # no plan: the library's WV_E_STATE; a group takes no engine with a plan
    eng = E.Engine(mesh, precision="f32")
    with pytest.raises(E.WaveguideError, match="error -6: .*no intensity plan"):
        eng.fetch_intensity_velocity()
    with pytest.raises(E.WaveguideError, match="error -6: .*no directional receivers"):
        eng.fetch_directional_velocity(1)
    group = E.LocalSlabGroup([eng])
    eng.set_intensity(2, 2, box=((1, 1, 1), (4, 4, 1)), **c)
    with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no intensity bins"):
        group.run_steps(4)
    eng.set_intensity(None)
    assert group.run_steps(4) == (4, 0)
    group.close()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise."""
    set_tuning(**FORMS[form])
    case = cases.CASES["random"]()
    out = []
    for plan in (None, dict(box=((1, 1, 1), (22, 18, 26)), stride=(1, 2, 1), period=7, first_step=3)):
        eng = make_engine(case, tag)
        if plan:
            eng.set_intensity(4, 2, **plan, **constants(plan))
        assert eng.run_steps(case["steps"]) == (case["steps"], 0)
        out.append([eng.fetch_receivers(0, case["steps"]), eng.read_field(E.BUF_CURRENT), eng.read_field(E.BUF_PREVIOUS)] +
                   [eng.read_boundary_data(d) for d in (1, 2, 3)])
        if plan:
            assert eng.intensity_count() == (9, 59)   # steps 3, 10, ..., 59
        eng.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert np.abs(out[0][0]).max() > 0


def test_kernel_timing_accounts_for_both_kernels():
    eng, _ = intensity_engine("impulse_flat", "f64", "single", dict(box=((1, 1, 1), (30, 30, 30)), period=1), 3, 8)
    eng.enable_kernel_timing(True)
    assert eng.run_steps(20) == (20, 0)
    eng.fetch_intensity()
    assert eng.query(E.Engine.QUERY_INTENSITY_FOLDS) == 2 and eng.query(E.Engine.QUERY_INTENSITY_NS) > 0
    assert eng.query(E.Engine.QUERY_INTENSITY_GATHERS) == 21 and eng.query(E.Engine.QUERY_INTENSITY_GATHER_NS) > 0
    eng.close()


def test_canonical_returns_the_bins_beside_the_receiver_output():
    """simulation.canonical(..., intensity=dict(plane=, every=, n_bins=)): the records are those of a run without a plan, the bins are
    the definition's over canonical's own snapshots of the plane's hull at the same cadence, with the mesh's spacing, sample_rate / every
    and the environment's density filled in; a second plan beside it is refused with the engine's message."""
    from test_gpu_decay import _box_scene
    set_tuning()
    W, vm, source, receiver = _box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    plan = dict(box=((1, 1, 11), (22, 22, 1)), period=3)    # (an odd period: after an impulse alone even steps only would see one parity of the mesh, and I = 0)
    hplan, box_in_hull = hull_of(plan)
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=hplan)
    bands, (bins, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                          intensity=dict(plane=11 * vm.mesh.spacing, every=3, n_bins=5))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 14 == len(steps) and bins.shape == (4, 5, 1, 22, 22)
    want = I.intensity_bins(fields, box_in_hull, vm.mesh.spacing, rate / 3, env.ambient_density, 5, 3)
    assert bins.tobytes() == want.tobytes() and all(np.abs(bins[a]).max() > 0 for a in range(4))
    with pytest.raises(E.WaveguideError, match="error -6: .*snapshot plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, snapshots=dict(period=8), intensity=dict(plane=0.5))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, intensity=dict(plane=0.5))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, intensity=dict(plane=0.0))     # the floor: no node below it


def test_the_tool_writes_the_intensity_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --intensity-map --intensity-plane z=... --intensity-every --intensity-out FILE.npz on its built-in hall."""
    out = tmp_path / "intensity.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.03",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--intensity-map", "--intensity-plane", "z=1.5",
                        "--intensity-every", "1", "--intensity-bin-ms", "5", "--intensity-out", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        bins, times, direction, diffuse = f["bins"], f["times"], f["net_direction"], f["diffuseness"]
        captures, per_bin, period, rate, plane = int(f["captures"]), int(f["bin_captures"]), int(f["period"]), float(f["sample_rate"]), int(f["plane"])
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    assert bins.dtype == np.float64 and bins.shape == (4, -(-captures // per_bin), dims[1] - 2, dims[0] - 2)
    assert period == 1 and captures == steps + 1 and per_bin == max(1, int(round(0.005 * rate)))
    assert times.shape == (bins.shape[1],) and times[0] == 0 and abs(times[1] - per_bin / rate) < 1e-12 and 1 <= plane <= dims[2] - 2
    assert direction.shape == (3,) + bins.shape[2:] and diffuse.shape == bins.shape[2:]
    assert all(np.abs(bins[a]).max() > 0 for a in range(4)) and np.isfinite(diffuse).any()
    heard = np.isfinite(direction[0])
    assert heard.any() and np.allclose((direction[:, heard] ** 2).sum(axis=0), 1.0)


def test_the_rate_tool_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/intensity_rate.py on a 48^3 room, 48 steps per repeat: every row is there; the plan's E planes equal a decay plan's and
    its velocities equal the receiver-per-node way's bytewise (where the two are defined to agree: period 1); the receiver way's
    records, summed on the host, equal the definition's sums of rounded products; and the figures land in the JSON file.  (Whether
    the bar holds is a matter of the 256^3 run, not of this size: the exit status may say either.)"""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "intensity_rate.py"), "--side", "48", "--steps", "48",
                        "--bin-captures", "5", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode in (0, 1), p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 3 and "INTENSITY RATE" in p.stdout, p.stdout
    report = json.load(open(str(out)))
    assert sorted(report["f64"]["rows"]) == sorted(["no plan", "plan every 1", "plan every 3", "receivers every 1"])
    assert all(report["f64"]["bytewise"].values()) and len(report["f64"]["bytewise"]) == 3
    assert report["f64"]["fold"]["model_bytes"] > 0 and report["f64"]["fold"]["launches"] > 0 and report["f64"]["gather"]["launches"] > 0

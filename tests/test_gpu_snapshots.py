"""Field snapshots taken on the device while wv_run keeps going (wv_set_snapshots; csrc/snapshot_kernels.hip.h, engine_snapshot.hip.h).
Every comparison is BITWISE against the existing path: an identical engine without a plan is advanced by run_steps to each snapshot
step and read with read_planes(dtype=float32), subsampled to the box.  Small meshes, forms forced, a few dozen steps."""
import numpy as np
import pytest

import cases
from helpers import set_tuning, subsample
from plan_cases import FORMS, make_engine      # (their home; the files that import them from here go on doing so)
from test_gpu_parity import _random_case
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu



@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


def plan_steps(plan, set_at, upto):
    first, period = plan.get("first_step", 0), plan.get("period", 1)
    return [s for s in range(first, upto + 1, period) if s >= set_at]


def reference_snapshots(case, tag, plan, steps):
    """The existing path: run_steps to each step, read_planes as float."""
    eng = make_engine(case, tag)
    dims = case["mesh"].dims
    out = {}
    try:
        for s in steps:
            todo = s - eng.step_count()
            assert eng.run_steps(todo) == (todo, 0)
            out[s] = np.ascontiguousarray(subsample(eng.read_planes(0, dims[2], dtype=np.float32), plan, dims))
    finally:
        eng.close()
    return out


def check_against_reference(case, tag, plan, n_steps, expect_query=None):
    eng = make_engine(case, tag, plan)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        got, got_steps = eng.fetch_snapshots()
        if expect_query is not None:
            assert eng.query(expect_query) > 0
        assert eng.query(E.Engine.QUERY_SNAPSHOTS_TAKEN) == len(got_steps)
        assert eng.query(E.Engine.QUERY_SNAPSHOT_BYTES) == got.nbytes
    finally:
        eng.close()
    want_steps = plan_steps(plan, 0, n_steps)
    assert len(want_steps) > 1 and list(got_steps) == want_steps
    assert got.dtype == np.float32
    want = reference_snapshots(case, tag, plan, want_steps)
    for j, s in enumerate(want_steps):
        assert got[j].shape == want[s].shape, (s, got[j].shape, want[s].shape)
        assert got[j].tobytes() == want[s].tobytes(), "snapshot of step %d differs from read_planes" % s
    assert np.abs(got[-1]).max() > 0   # (the comparison is not of zeros)
    return got, got_steps


FORM_CASES = [("single", 1, None), ("single", 5, None), ("graph", 16, None), ("graph", 32, None),
              ("pair", 2, E.Engine.QUERY_PASSES), ("pair", 3, E.Engine.QUERY_PASSES), ("pair", 7, E.Engine.QUERY_PASSES),
              ("triple", 3, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 6, E.Engine.QUERY_TRIPLE_PASSES),
              ("triple", 4, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 7, E.Engine.QUERY_TRIPLE_PASSES)]


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_fields_read_planes_gives(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes, periods that do and do not divide 2 and 3: a full plane of the 32^3
    impulse room (walls with a flat filter)."""
    set_tuning(**FORMS[form])
    case = cases.CASES["impulse_flat"]()
    n_steps = 64 if form == "graph" else 30
    check_against_reference(case, tag, dict(box=((0, 0, 15), (None, None, 1)), period=period), n_steps, query)


BOXES = {
    "full-plane": dict(box=((0, 0, 5), (None, None, 1))),
    "sub-box": dict(box=((3, 2, 4), (10, 9, 7))),
    "sub-box-16-byte-rows": dict(box=((4, 1, 2), (16, 5, 3))),
    "every-face": dict(box="mesh"),
    "every-face-stride-3": dict(box="mesh", stride=3),          # 24 / 3, 20 / 3 and 28 / 3: the last two do not divide
    "strides-1-2-3": dict(box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3)),
    "strides-2-3-1": dict(box=((0, 1, 0), (24, 19, 28)), stride=(2, 3, 1)),
    "strides-3-1-2": dict(box=((2, 0, 1), (22, 20, 27)), stride=(3, 1, 2)),
    "far-corner": dict(box=((22, 18, 26), (2, 2, 2))),           # the last two nodes of every axis: the corner wall node and the dead shell
}


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, both fields written by the caller (two single sweeps
    first, then three-step passes), a soft source and eight receivers; snapshots every 4 steps from step 2."""
    set_tuning(**FORMS["triple"])
    case = cases.CASES["random"]()
    plan = dict(BOXES[name], first_step=2, period=4)
    got, _ = check_against_reference(case, tag, plan, 30, E.Engine.QUERY_TRIPLE_PASSES)
    nx, ny, nz = case["mesh"].dims
    if name == "every-face-stride-3":
        assert got.shape[1:] == (10, 7, 8)
    if name == "every-face":
        assert got.shape[1:] == (nz, ny, nx)


@pytest.mark.parametrize("form", ["pair", "triple"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_ragged_room(form, tag):
    """131 x 9 x 7 (rows of odd length, pad columns behind them) with a re-entrant node, a source and receivers: the whole mesh, and
    a box whose rows start and end off every 16-byte boundary."""
    set_tuning(**FORMS[form])
    case = _random_case((131, 9, 7), seed=147, steps=24)
    check_against_reference(case, tag, dict(box="mesh", period=5), 24)
    check_against_reference(case, tag, dict(box=((1, 1, 1), (129, 7, 5)), stride=(2, 1, 1), period=3, first_step=1), 24)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise."""
    set_tuning(**FORMS[form])
    case = cases.CASES["random"]()
    out = []
    for plan in (None, dict(box="mesh", stride=(1, 2, 1), period=7, first_step=3)):
        eng = make_engine(case, tag, plan)
        assert eng.run_steps(case["steps"]) == (case["steps"], 0)
        out.append([eng.fetch_receivers(0, case["steps"]), eng.read_field(E.BUF_CURRENT), eng.read_field(E.BUF_PREVIOUS)] +
                   [eng.read_boundary_data(d) for d in (1, 2, 3)])
        if plan:
            assert eng.snapshot_count() == (9, 0)   # steps 3, 10, ..., 59
        eng.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("bad_step", [12, 13, 14])
def test_a_run_that_stops_on_a_flag_holds_no_snapshot_of_a_later_step(form, bad_step):
    """inf in the source signal at step f: the run completes f steps; snapshots every 4 steps are held for 0, 4, 8, 12 and none beyond
    (12 is both the last completed step count and a snapshot step when f = 12)."""
    set_tuning(**FORMS[form])
    mesh = M.box_mesh(12, 12, 12)
    sig = np.zeros(40)
    sig[0] = 1.0
    sig[bad_step] = np.inf
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=sig,
                recv=[mesh.compute_index(7, 6, 6)])
    plan = dict(box=((0, 0, 6), (None, None, 1)), period=4)
    eng = make_engine(case, "f64", plan)
    done, flag = eng.run_steps(40)
    assert done == bad_step and flag & M.ERR_INF
    got, steps = eng.fetch_snapshots()
    eng.close()
    assert list(steps) == [0, 4, 8, 12] and all(s <= bad_step for s in steps)
    assert np.isfinite(got).all()
    want = reference_snapshots(case, "f64", plan, [0, 4, 8, 12])
    for j, s in enumerate(steps):
        assert got[j].tobytes() == want[int(s)].tobytes()


def test_keep_holds_the_last_ones_only():
    """keep = 2 over ten snapshots: the last two are held; fetching an earlier one is WV_E_INVALID_ARGUMENT, fetching one not yet taken
    likewise."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["impulse_flat"]()
    plan = dict(box=((0, 0, 16), (None, None, 1)), period=3, first_step=3, keep=2)
    eng = make_engine(case, "f32", plan)
    assert eng.run_steps(30) == (30, 0)
    assert eng.snapshot_count() == (10, 8)
    got, steps = eng.fetch_snapshots()
    assert list(steps) == [27, 30]
    one, one_step = eng.fetch_snapshots(9, 1)
    assert one_step[0] == 30 and one.tobytes() == got[1].tobytes()
    with pytest.raises(E.WaveguideError, match="error -1: .*dropped"):
        eng.fetch_snapshots(7, 1)
    with pytest.raises(E.WaveguideError, match="error -1: .*not taken"):
        eng.fetch_snapshots(9, 2)
    eng.close()
    want = reference_snapshots(case, "f32", plan, [27, 30])
    assert got[0].tobytes() == want[27].tobytes() and got[1].tobytes() == want[30].tobytes()


@pytest.mark.parametrize("form", ["single", "triple"])
def test_checkpoint_run_rollback_rerun_gives_the_same_snapshots_twice(form):
    set_tuning(**FORMS[form])
    case = cases.CASES["random"]()
    plan = dict(box=((2, 3, 4), (12, 11, 9)), stride=(1, 2, 2), period=5)
    eng = make_engine(case, "f64", plan)
    assert eng.run_steps(10) == (10, 0)            # snapshots of 0, 5, 10
    eng.checkpoint()
    assert eng.run_steps(17) == (17, 0)            # 15, 20, 25
    first, first_steps = eng.fetch_snapshots()
    assert list(first_steps) == [0, 5, 10, 15, 20, 25]
    eng.rollback()
    assert eng.step_count() == 10
    kept, kept_steps = eng.fetch_snapshots()
    assert list(kept_steps) == [0, 5, 10] and kept.tobytes() == first[:3].tobytes()
    assert eng.run_steps(17) == (17, 0)
    second, second_steps = eng.fetch_snapshots()
    eng.close()
    assert list(second_steps) == list(first_steps) and second.tobytes() == first.tobytes()
    want = reference_snapshots(case, "f64", plan, [int(s) for s in first_steps])
    for j, s in enumerate(first_steps):
        assert first[j].tobytes() == want[int(s)].tobytes()


def test_a_plan_set_at_a_non_zero_step_count_captures_that_very_step_at_the_next_run():
    """... and steps of the plan before it are not taken; wv_step / wv_swap take none, and snapshot steps they pass are passed."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    eng = make_engine(case, "f32")
    ref = make_engine(case, "f32")
    dims = case["mesh"].dims
    assert eng.run_steps(9) == (9, 0) and ref.run_steps(9) == (9, 0)
    plan = dict(box=((0, 0, 0), (None, None, 2)), period=3)      # steps 0, 3, 6 lie before the plan; 9 is the count it is set at
    eng.set_snapshots(**plan)
    assert eng.snapshot_count() == (0, 0)
    want = {9: subsample(ref.read_planes(0, dims[2], dtype=np.float32), plan, dims)}
    assert eng.run_steps(4) == (4, 0)                                    # 9 (at the start of this run), 12
    assert ref.run_steps(3) == (3, 0)
    want[12] = subsample(ref.read_planes(0, dims[2], dtype=np.float32), plan, dims)
    assert ref.run_steps(1) == (1, 0)
    for e in (eng, ref):                                                  # 13 -> 16 by generic steps: 15 is passed
        for _ in range(3):
            assert e.step() == 0
            e.swap()
    assert eng.snapshot_count() == (2, 0)
    assert eng.run_steps(2) == (2, 0) and ref.run_steps(2) == (2, 0)     # 18
    want[18] = subsample(ref.read_planes(0, dims[2], dtype=np.float32), plan, dims)
    got, steps = eng.fetch_snapshots()
    assert list(steps) == [9, 12, 18]
    assert got[0].tobytes() == np.ascontiguousarray(want[9]).tobytes()
    assert got[1].tobytes() == np.ascontiguousarray(want[12]).tobytes()
    assert got[2].tobytes() == np.ascontiguousarray(want[18]).tobytes()
    eng.set_snapshots(None)                                               # stops and forgets
    with pytest.raises(E.WaveguideError):
        eng.snapshot_count()
    assert eng.run_steps(3) == (3, 0)
    eng.close()
    ref.close()


def test_kernel_timing_accounts_for_the_capture_kernels():
    set_tuning(**FORMS["single"])
    case = cases.CASES["impulse_flat"]()
    eng = make_engine(case, "f64", dict(box="mesh", period=2))
    eng.enable_kernel_timing(True)
    assert eng.run_steps(12) == (12, 0)
    assert eng.query(E.Engine.QUERY_SNAPSHOTS_TAKEN) == 7
    assert eng.query(E.Engine.QUERY_SNAPSHOT_BYTES) == 7 * 32 ** 3 * 4
    assert eng.query(E.Engine.QUERY_SNAPSHOT_NS) > 0
    eng.close()


def test_refusals():
    """A box that leaves the mesh, a zero stride, a zero period: WV_E_INVALID_ARGUMENT; a slab of a chain: WV_E_STATE."""
    mesh = M.box_mesh(16, 12, 10)
    eng = E.Engine(mesh, precision="f32")
    for bad in (dict(box=((0, 0, 0), (17, 12, 10))), dict(box=((0, 0, 0), (16, 13, 10))), dict(box=((0, 0, 0), (16, 12, 11))),
                dict(box=((-1, 0, 0), (4, 4, 4))), dict(box=((0, 0, 10), (1, 1, 1)))):
        with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
            eng.set_snapshots(**bad)
    plan = E.WvSnapshotPlan(0, 0, 0, 4, 4, 4, 1, 0, 1, 0, 1, 0, 0)
    assert eng.lib.wv_set_snapshots(eng.h, plan) == -1 and b"stride" in eng.lib.wv_last_error()
    plan = E.WvSnapshotPlan(0, 0, 0, 4, 4, 4, 1, 1, 1, 0, 0, 0, 0)
    assert eng.lib.wv_set_snapshots(eng.h, plan) == -1 and b"period" in eng.lib.wv_last_error()
    assert eng.run_steps(3) == (3, 0)      # untouched by the refusals
    eng.close()
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
        slab.set_snapshots(box=((0, 0, 0), (4, 4, 1)))
    slab.close()


def test_canonical_returns_the_snapshots_beside_the_receiver_output():
    """simulation.canonical(..., snapshots=...) passes the plan to the engine: the same records as without one, and the plane every
    eighth step beside them."""
    from wayverb_amd import simulation as W
    set_tuning()
    mesh = M.box_mesh(24, 24, 24, coefficients=np.array([M.flat_coefficients(0.1)], dtype=M.coefficients_dtype))
    vm = W.VoxelsAndMesh(None, None, 0, None, None, mesh, (0.0, 0.0, 0.0))
    env = W.Environment()
    sp = mesh.spacing
    source, receiver = (12 * sp, 12 * sp, 12 * sp), (15 * sp, 12 * sp, 12 * sp)
    seconds = 39.5 / W.compute_sample_rate(sp, env.speed_of_sound)      # 40 steps
    plain = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32")
    bands, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                         snapshots=dict(box=((0, 0, 12), (None, None, 1)), period=8))
    assert plain[0][0].shape[0] == 40 and bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert list(steps) == [0, 8, 16, 24, 32, 40] and fields.shape == (6, 1, 24, 24) and fields.dtype == np.float32
    assert not fields[0].any() and all(f.any() for f in fields[1:])     # step 0: before the source's first sample
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, snapshots=dict(period=8))


def test_fetching_without_a_plan_and_stepping_a_group_with_one_are_refused():
    """No plan: the library's WV_E_STATE, not a Python error.  wv_run_group takes no snapshots: an engine with a plan is refused there
    (WV_E_STATE) instead of silently recording nothing."""
    mesh = M.box_mesh(16, 12, 10)
    eng = E.Engine(mesh, precision="f32")
    with pytest.raises(E.WaveguideError, match="error -6: .*no snapshot plan"):
        eng.fetch_snapshots(0, 1)
    with pytest.raises(E.WaveguideError, match="error -6: .*no snapshot plan"):
        eng.fetch_snapshots()
    group = E.LocalSlabGroup([eng])
    eng.set_snapshots(box=((0, 0, 0), (4, 4, 1)), period=2)
    with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group takes no snapshots"):
        group.run_steps(4)
    assert eng.run_steps(4) == (4, 0) and list(eng.fetch_snapshots()[1]) == [0, 2, 4]
    eng.set_snapshots(None)
    assert group.run_steps(4) == (4, 0)
    group.close()

"""A capture that holds NaN, +inf and -inf, folded on the DEVICE by every one of the eleven kinds of plan.  include/wayverb_amd.h
states the rule for four folds -- "a NaN is no onset" (arrival, lateral, banded arrival, interaural) -- and for the peaks -- "a NaN
changes nothing" -- and interaural_fold_kernel takes fmaxf(|a|, |b|), "the other operand where one is a NaN"; the tests that stop a
run on a flag all show that the capture of a BAD step is dropped, so none of them ever folded such a capture.  One is reachable with no
fault involved: CaptureStage::begin_run captures the step the engine stands at when it is a plan step, and staged_begin_run commits
that capture at once, before the step that raises the flag is computed.  A caller who writes a field that holds an inf and calls wv_run
at a plan step gets that field folded into the sums, for good.  What v_max_f32, the float compares and the (float) casts of the three
gather kernels do with NaN and +-inf on gfx950 is something the host builds under tests/cpp cannot tell.

The construction is tests/test_gpu_plan_extremes.py's: a 12^3 box in f64, a hard source of zeros, fields of uniform(-1, 1) (scaled) on
the inside nodes, and two engines with identical calls -- one with the plan under test, the companion with a SNAPSHOT plan of what that
plan captures, whose float32 snapshots are the captures handed to plan_twin.PlanTwin.expected().  The sequence (tests/eleven_kinds.py
has the fields and plays it on the oracle for tests/test_eleven_kinds.py): the plan from step 0; 13 steps (captures 0 .. 13); one
outside step, so that the engine stands at step 14 and that is the plan's next; `current` written with 15 of the box's inside nodes
replaced by 5 NaN, 5 +inf, 5 -inf; run_steps(4), which captures and commits step 14 as written and comes back with a flag; finite
fields, clean filter memories and a finite source put back; on to step 30.  The poisoned capture lies inside the first fold of 16
captures, among the last samples of it that the interaural ring carries into the second.  A second case poisons capture 0: the field
is written, then the plan is set at the step the engine stands at.

The comparison is eleven_kinds.assert_outputs_but_nan_bytes: dtype and shape, NaN exactly where the definition has one, every other
entry BYTEWISE, +-inf and signed zeros included.  The bytes of a NaN are not compared: an x86 host makes the negative quiet NaN out of
inf - inf and gfx950 the positive one, and the NumPy definitions of eight kinds give NaNs of both signs on such captures (banded,
intensity, arrival, lateral, modulation, banded arrival and both interaural plans).  What keeps that mask from hiding a failure is
asserted on the expected values first (eleven_kinds.assert_poison_conditions): fewer than 15 % NaNs in every output, something bad
and something finite and non-zero in every output that can go bad, and the onset rules."""
import numpy as np
import pytest

import eleven_kinds as K
import plan_twin as P
from helpers import set_tuning
from test_gpu_snapshots import FORMS, make_engine
from wayverb_amd import engine as E

pytestmark = pytest.mark.gpu

CASES = [(kind, {}) for kind in K.KINDS11] + [("interaural", K.UNFILTERED)]
IDS = list(K.KINDS11) + ["interaural-unfiltered"]


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


@pytest.fixture(scope="module")
def eleven_kinds():
    with K.registered():
        yield


@pytest.mark.parametrize("poison_capture", [K.POISON_STEP, 0], ids=["capture14", "capture0"])
@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("kind,over", CASES, ids=IDS)
def test_a_poisoned_capture_is_folded_as_the_definition_folds_it(eleven_kinds, kind, over, form, poison_capture):
    set_tuning(**FORMS[form])
    plan = K.plan_of(kind, **dict(dict(threshold=K.THRESHOLD) if kind in K.ONSET_KINDS else {}, **over))
    case = K.poison_case()
    mesh = case["mesh"]
    inside, start, back = K.poison_fields(mesh)
    nodes = K.poisoned_nodes(mesh.dims, inside)
    captured = P.capture_box(plan)
    snapshot_plan = dict(box=captured["box"], stride=captured["stride"], first_step=0, period=1)
    where = (kind, over, form, poison_capture)
    engines = [make_engine(case, "f64"), make_engine(case, "f64")]
    try:
        memories = [engines[0].read_boundary_data(d) for d in (1, 2, 3)]
        for eng in engines:
            eng.write_field(start[0], E.BUF_PREVIOUS)
            eng.write_field(start[1], E.BUF_CURRENT)
        if poison_capture:
            engines[0].set_snapshots(**snapshot_plan)
            P.set_plan(engines[1], plan)
            for eng in engines:
                assert eng.run_steps(K.POISON_STEP - 1) == (K.POISON_STEP - 1, 0)
                assert eng.step() == 0
                eng.swap()
        assert all(eng.step_count() == poison_capture for eng in engines)
        written = K.poison(engines[0].read_field(E.BUF_CURRENT), nodes)
        for eng in engines:
            eng.write_field(written, E.BUF_CURRENT)
        if not poison_capture:      # the plan is set at the step the engine stands at, the field already written
            engines[0].set_snapshots(**snapshot_plan)
            P.set_plan(engines[1], plan)
        # begin_run captures and commits the step as written; the run then comes back with a flag
        stopped = [eng.run_steps(4) for eng in engines]
        assert stopped[0] == stopped[1] and stopped[0][1] != 0, (stopped, where)
        assert P.KINDS[kind].count(engines[1])[0] == poison_capture + 1, where      # the poisoned capture is in, none of a bad step
        sig = np.zeros(40)
        for eng in engines:
            eng.write_field(back[0], E.BUF_PREVIOUS)
            eng.write_field(back[1], E.BUF_CURRENT)
            for d, clean in zip((1, 2, 3), memories):
                eng.write_boundary_data(d, clean)
            eng.set_source(E.SOURCE_HARD, case["source_node"], sig)
            todo = K.LAST_STEP - eng.step_count()
            assert eng.run_steps(todo) == (todo, 0), where
        snaps, steps = engines[0].fetch_snapshots()
        assert list(steps) == list(range(K.LAST_STEP + 1)) and snaps.dtype == np.float32, where
        # the companion holds the poisoned step as written: NaN, +inf and -inf exactly where they were put, nothing else that is not finite
        bad = snaps[poison_capture]
        nan_at, plus_at, minus_at = K.in_capture(nodes, captured, mesh.dims)
        assert np.array_equal(np.isnan(bad), nan_at) and np.array_equal(bad == np.inf, plus_at) and np.array_equal(bad == -np.inf, minus_at), where
        assert nan_at.sum() == plus_at.sum() == minus_at.sum() == 5 and np.isfinite(np.delete(snaps, poison_capture, axis=0)).all(), where
        twin = P.PlanTwin(None, mesh, np.float64)
        twin.set_plan(plan)
        twin.log = [(int(s), a) for s, a in zip(steps, snaps)]
        with np.errstate(all="ignore"):
            want = twin.expected()
        K.assert_poison_conditions(plan, want, snaps, K.in_capture(nodes, plan, mesh.dims), poison_capture)
        got = dict(count=P.KINDS[kind].count(engines[1]), **P.KINDS[kind].fetch(engines[1]))
        K.assert_outputs_but_nan_bytes(got, want, where)
    finally:
        for eng in engines:
            eng.close()

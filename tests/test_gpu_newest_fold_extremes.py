"""tests/test_gpu_plan_extremes.py's test_subnormal_and_huge_captures, asked of the three newest folds: arrival_bands_fold_kernel,
waterfall_fold_kernel and interaural_fold_kernel -- the latter in its filtered instance and in the one that keeps its samples as
floats (SMAX == 0), whose history ring of doubles is read back into those floats.  That file asks it of the eight older kinds for the
reason its docstring gives: the host builds of the kernels (tests/cpp) meet such values too, but a host build cannot tell what the
DEVICE's float-denormal mode does to them.

Everything is that test's, imported from it: the 12^3 box in f64 with a hard source of zeros, fields of uniform(-1, 1) * scale
through write_field, 20 steps with every step captured, at 1e-41 (captures that are subnormal floats) and 1e30 (near the top of the
float range, negative zeros placed among them), a companion engine with a SNAPSHOT plan of what the plan captures, whose snapshots are
first held bytewise to NumPy's own conversion of the f64 fields and then fed to the shipped definitions.  Every output must equal the
definition's BYTEWISE; no NaN appears.  The plans are eleven_kinds.plan_of's with scaled_bands()'s cascade for sections (the banded
arrival plan takes it twice, as two bands); the banded arrival and both interaural plans also run with a threshold_map of subnormal
floats.  Behind a filter at 1e-41 more than half of the first section's states are subnormal doubles, shown with a few lines of NumPy
(eleven_kinds.first_section_state) over the captures of one ear."""
import numpy as np
import pytest

import eleven_kinds as K
import plan_twin as P
from helpers import set_tuning, subsample
from test_gpu_plan_extremes import BOX, SCALES, STEPS, fields_of, stepwise_fields, the_case
from test_gpu_snapshots import FORMS, make_engine
from wayverb_amd import engine as E

pytestmark = pytest.mark.gpu

TINY32 = np.finfo(np.float32).tiny
assert BOX == K.BOX and SCALES == (1e-41, 1e30)


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


@pytest.fixture(scope="module")
def eleven_kinds():
    with K.registered():
        yield


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name,with_map", K.EXTREME_CASES, ids=["%s%s" % (n, "-map" if m else "") for n, m in K.EXTREME_CASES])
def test_subnormal_and_huge_captures(eleven_kinds, name, with_map, scale):
    set_tuning(**FORMS["pair"])
    case = the_case()
    mesh = case["mesh"]
    plan = K.extreme_plan(name, scale, with_map)
    kind = plan["kind"]
    previous, current, placed = fields_of(mesh, scale)
    captured = P.capture_box(plan)
    engines = [make_engine(case, "f64", dict(box=captured["box"], stride=captured["stride"], period=1)), make_engine(case, "f64")]
    try:
        P.set_plan(engines[1], plan)
        for eng in engines:
            eng.write_field(previous, E.BUF_PREVIOUS)
            eng.write_field(current, E.BUF_CURRENT)
            assert eng.run_steps(STEPS) == (STEPS, 0)
        snaps, steps = engines[0].fetch_snapshots()
        assert list(steps) == list(range(STEPS + 1))
        # the captures are NumPy's conversion of the f64 fields, subnormals rounded as it rounds them
        with np.errstate(under="ignore"):
            cast = np.stack([np.ascontiguousarray(subsample(f, captured, mesh.dims)) for f in stepwise_fields(scale)]).astype(np.float32)
        assert snaps.dtype == cast.dtype and snaps.shape == cast.shape and snaps.tobytes() == cast.tobytes()
        assert np.isfinite(snaps).all()
        if scale < 1:
            assert ((snaps != 0) & (np.abs(snaps) < TINY32)).mean() > 0.5
            if plan.get("threshold_map") is not None:
                assert ((plan["threshold_map"] != 0) & (plan["threshold_map"] < TINY32)).all()
        else:
            # the negative zeros of capture 0 are the placed ones, all of them that lie in what is captured, and there are some
            here = np.ascontiguousarray(subsample(placed.reshape(mesh.dims[::-1]), captured, mesh.dims))
            assert here.sum() >= 10 and np.array_equal(np.signbit(snaps[0]) & (snaps[0] == 0), here) and np.abs(snaps).max() > 1e29
        twin = P.PlanTwin(None, mesh, np.float64)
        twin.set_plan(plan)
        twin.log = [(int(s), a) for s, a in zip(steps, snaps)]
        with np.errstate(under="ignore"):
            want = twin.expected()
        K.assert_extreme_conditions(name, plan, scale, want, snaps)
        P.assert_outputs(engines[1], kind, want, (name, with_map, scale))
    finally:
        for eng in engines:
            eng.close()

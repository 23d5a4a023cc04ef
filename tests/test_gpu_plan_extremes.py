"""Every fold and both gather kernels on captures that are SUBNORMAL floats, and on captures near the top of the float range with
negative zeros among them -- what tests/test_gpu_decay_bands.py's test_subnormal_floats_and_subnormal_states asks of the banded-decay
fold, asked of the seven other kinds of plan.  The host builds of the kernels (tests/cpp) meet such values too, but a host build
cannot tell what the DEVICE's float-denormal mode does to them: intensity_gather_kernel subtracts and converts floats,
arrival_fold_kernel and lateral_fold_kernel compare |p| >= thr in float, and every gather converts a double to a float.

The construction is that test's: a 12^3 box in f64, a hard source of zeros, `previous` and `current` written through write_field
as uniform(-1, 1) * scale on the inside nodes, 20 steps, every step captured.  A companion engine with a SNAPSHOT plan of the same
capture box (the hull, for intensity and lateral plans) supplies the float32 captures; they are first held, bytewise, to NumPy's
own conversion of the f64 fields an engine without any plan shows step by step, and then fed to the shipped definitions
(plan_twin.PlanTwin.expected).  Every output must equal the definition's BYTEWISE; no NaN appears (squares and hull
differences stay finite at 1e30), so no NaN bytes are compared."""
import numpy as np
import pytest

import plan_twin as P
from helpers import set_tuning, subsample
from test_gpu_snapshots import FORMS, make_engine
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import lateral as L
from wayverb_amd import mesh as M
from wayverb_amd import modulation as MOD

pytestmark = pytest.mark.gpu

STEPS = 20
SCALES = (1e-41, 1e30)
BOX = ((1, 1, 4), (10, 9, 3))          # 270 nodes: two workgroups of a fold, the second one partly idle; its hull reaches three faces of the mesh
EDGES = [0, 1, 5, 16]
MAIN = {"snapshots": "snapshots", "spectrum": "spectrum", "modulation": "sums"}     # the output that must not be all zeros; of every other kind `bins`
TINY32, TINY64 = np.finfo(np.float32).tiny, np.finfo(np.float64).tiny


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


def the_case():
    mesh = M.box_mesh(12, 12, 12)
    return dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=np.zeros(24),
                recv=[mesh.compute_index(7, 6, 6)])


def fields_of(mesh, scale):
    """(previous, current, placed): uniform(-1, 1) * scale on the inside nodes and +0.0 on every other; at 1e30 a tenth of the inside
    nodes of `current`, the nodes `placed`, hold -0.0 -- the only negative zeros there are."""
    rng = np.random.default_rng(11)
    inside = (mesh.nodes["boundary_type"] & M.ID_INSIDE) != 0
    previous, current = [np.where(inside, rng.uniform(-1, 1, mesh.num_nodes) * scale, 0.0) for _ in range(2)]
    placed = np.zeros(mesh.num_nodes, dtype=bool)
    if scale > 1:
        placed[rng.choice(np.nonzero(inside)[0], int(inside.sum()) // 10, replace=False)] = True
        current[placed] = -0.0
    assert not np.signbit(previous[previous == 0]).any() and np.array_equal(np.signbit(current) & (current == 0), placed)
    return previous, current, placed


def scaled_bands():
    """test_subnormal_floats_and_subnormal_states' sections: the first section's numerator scaled by 1e-280, so that at 1e-41 its
    output and the states behind it are subnormal doubles; the last section scales by 1e+280 back to where a square is not zero."""
    bw = D.butterworth_bandpass(0.05, 0.2, 1.0)
    first = bw[0].copy()
    first[:3] *= 1e-280
    return np.array([[first, bw[2], [1e280, 0.0, 0.0, 0.0, 0.0]]])


def plan_of(kind, scale, with_map):
    plan = dict(kind=kind, box=BOX, stride=(1, 1, 1), first_step=0, period=1)
    if kind == "spectrum":
        plan["freqs"] = [0.0, 0.5, 0.123, 0.31]
    elif kind in ("decay", "intensity"):
        plan["n_bins"], plan["bin_captures"] = 4, 5
    elif kind in ("arrival", "lateral"):
        plan["edges"], plan["threshold"], plan["threshold_map"] = EDGES, 0.0, None
        if with_map:
            # around half the field's scale, a decade either way: at 1e-41 every entry is a subnormal float.  A field of uniform(-1, 1)
            # has a standard deviation of 0.58 and the update keeps it there (the scheme conserves energy), so over 21 captures a node
            # passes about twice that and seldom three times: the upper third of the thresholds, above 2.3 * scale, is seldom reached
            factors = 10.0 ** np.random.default_rng(12).uniform(-1, 1, P.taken(plan)[::-1])
            plan["threshold_map"] = (0.5 * scale * factors).astype(np.float32)
    elif kind == "modulation":
        plan["freqs"], plan["bands"] = [0.0, 0.5, 0.123, 0.31], scaled_bands()
    return plan


_fields = {}     # scale -> the f64 field after 0 .. STEPS steps, [STEPS + 1][nz][ny][nx], from an engine without a plan: computed once


def stepwise_fields(scale):
    if scale not in _fields:
        case = the_case()
        previous, current, _ = fields_of(case["mesh"], scale)
        eng = make_engine(case, "f64")
        try:
            eng.write_field(previous, E.BUF_PREVIOUS)
            eng.write_field(current, E.BUF_CURRENT)
            out = [eng.read_field(E.BUF_CURRENT).copy()]
            for _ in range(STEPS):
                assert eng.run_steps(1) == (1, 0)
                out.append(eng.read_field(E.BUF_CURRENT).copy())
        finally:
            eng.close()
        fields = np.stack(out).reshape((STEPS + 1,) + case["mesh"].dims[::-1])
        fields.setflags(write=False)
        _fields[scale] = fields
    return _fields[scale]


CASES = [(kind, False) for kind in P.KINDS8 if kind != "banded"] + [("arrival", True), ("lateral", True)]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("kind,with_map", CASES, ids=["%s%s" % (k, "-map" if m else "") for k, m in CASES])
def test_subnormal_and_huge_captures(kind, with_map, scale):
    set_tuning(**FORMS["pair"])
    case = the_case()
    mesh = case["mesh"]
    plan = plan_of(kind, scale, with_map)
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
        main = want[MAIN.get(kind, "bins")]
        assert np.any(main != 0) and all(np.isfinite(v).all() for v in want.values() if isinstance(v, np.ndarray) and v.dtype.kind in "fc")
        if kind in ("arrival", "lateral"):
            heard = want["onset"] != L.NONE
            if with_map:       # nodes with an onset and nodes without, onsets at several captures
                assert heard.any() and (~heard).any() and len(np.unique(want["onset"][heard])) >= 3
            else:              # |p| >= 0 holds at capture 0, of a zero too
                assert (want["onset"] == 0).all()
        if kind == "modulation" and scale < 1:
            with np.errstate(under="ignore"):
                _, _, state = MOD.modulation_fold(snaps, steps, plan["freqs"], plan["bands"], return_state=True)
            state = np.asarray(state)
            assert ((state[0, :2] != 0) & (np.abs(state[0, :2]) < TINY64)).mean() > 0.5
        P.assert_outputs(engines[1], kind, want, (kind, with_map, scale))
    finally:
        for eng in engines:
            eng.close()

"""Energy decay maps: time-binned field energy accumulated on the device while wv_run keeps going (wv_set_decay;
csrc/decay_kernels.hip.h, engine_decay.hip.h).  The reference of every comparison is a second, identical engine with a SNAPSHOT plan of
the same box and cadence, whose snapshots are binned in NumPy in capture order: `E[b] = E[b] + p * p` on float64 arrays is an exact
product and a rounded sum, which is the definition.  Equality is BYTEWISE.  Small meshes, forms forced, a few dozen steps."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import numpy_bins, set_tuning
from test_gpu_snapshots import FORMS, make_engine
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()



_reference = {}


def reference_snapshots(case_name, tag, form, plan, n_steps):
    """(snapshots, steps) of an identical engine with a snapshot plan of the same box and cadence; computed once per key, read only."""
    key = (case_name, tag, form, repr(sorted(plan.items())), n_steps)
    if key not in _reference:
        set_tuning(**FORMS[form])
        eng = make_engine(cases.CASES[case_name](), tag, plan)
        try:
            assert eng.run_steps(n_steps) == (n_steps, 0)
            snaps, steps = eng.fetch_snapshots()
        finally:
            eng.close()
        snaps.setflags(write=False)
        _reference[key] = (snaps, steps)
    return _reference[key]


def decay_engine(case_name, tag, form, plan, n_bins, bin_captures):
    set_tuning(**FORMS[form])
    eng = make_engine(cases.CASES[case_name](), tag)
    shape = eng.set_decay(n_bins, bin_captures, **plan)
    return eng, shape


def check(case_name, tag, form, plan, n_bins, bin_captures, n_steps, query=None):
    snaps, steps = reference_snapshots(case_name, tag, form, plan, n_steps)
    want = numpy_bins(snaps, n_bins, bin_captures)
    eng, shape = decay_engine(case_name, tag, form, plan, n_bins, bin_captures)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert eng.decay_count() == (len(steps), int(steps[-1]))
        got, captures = eng.fetch_decay()
        if query is not None:
            assert eng.query(query) > 0
        assert eng.query(E.Engine.QUERY_DECAY_CAPTURES) == len(steps)
        folds = eng.query(E.Engine.QUERY_DECAY_FOLDS)
    finally:
        eng.close()
    assert captures == len(steps) and len(steps) > 1
    assert got.shape == shape == want.shape and got.dtype == np.float64
    assert folds <= -(-len(steps) // 16) + 1
    assert got.tobytes() == want.tobytes(), "largest difference %g" % np.abs(got - want).max()
    assert got.max() > 0 and np.abs(snaps[-1]).max() > 0   # (the comparison is not of zeros)
    return got, snaps


FORM_CASES = [("single", 1, None), ("single", 5, None), ("graph", 16, None),
              ("pair", 2, E.Engine.QUERY_PASSES), ("pair", 3, E.Engine.QUERY_PASSES), ("pair", 7, E.Engine.QUERY_PASSES),
              ("triple", 3, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 4, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 7, E.Engine.QUERY_TRIPLE_PASSES)]


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_bins_of_the_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes, periods that do and do not divide 2 and 3: one plane of the 32^3 impulse
    room, four captures per bin.  The bins summed over time are the plain ordered sum of p^2 only up to rounding, so the check on the
    whole is the bytewise one."""
    n_steps = 64 if form == "graph" else 30
    captures = n_steps // period + 1
    check("impulse_flat", tag, form, dict(box=((0, 0, 15), (None, None, 1)), period=period), -(-captures // 4), 4, n_steps, query)


BOXES = {
    "sub-box-630": dict(box=((3, 2, 4), (10, 9, 7))),             # not a multiple of 64, an odd number of rows; two nodes per lane
    "sub-box-567-odd": dict(box=((3, 2, 4), (9, 9, 7))),          # an odd B: one node per lane, three workgroups, a tail
    "sub-box-16-byte-rows": dict(box=((4, 1, 2), (16, 5, 3))),
    "every-face-stride-3": dict(box="mesh", stride=3),            # 24 / 3, 20 / 3 and 28 / 3: the last two do not divide
    "strides-1-2-3": dict(box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3)),
    "one-node": dict(box=((5, 6, 7), (1, 1, 1))),
}


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; every step captured, 21 captures
    (more than the stage holds), three captures per bin."""
    check("random", tag, "triple", dict(BOXES[name], period=1), 7, 3, 20)


# (n_bins, bin_captures) against the 16-slot stage, 33 captures: 16 + 16 + 1 for the fetch
LAYOUTS = {
    "W1-every-capture-a-new-bin": (33, 1),       # r = t
    "W5-edges-inside-and-across-folds": (7, 5),
    "W16-a-stage-per-bin": (3, 16),
    "W17": (2, 17),
    "W40-whole-folds-in-one-bin": (2, 40),      # (the second bin stays +0.0)
    "one-bin": (1, 1),
    "open-ended-last-bin": (4, 3),               # 12 captures fill the bins, the last takes the other 21
    "more-bins-than-captures": (4096, 1),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_bin_layouts_against_the_stage(name, layout):
    n_bins, bin_captures = LAYOUTS[layout]
    got, _ = check("random", "f64", "pair", dict(BOXES[name], period=1), n_bins, bin_captures, 32)
    if layout == "more-bins-than-captures":
        assert (got[33:] == 0).all() and not np.signbit(got[33:]).any()    # never touched: +0.0


@pytest.mark.parametrize("captures", [1, 16, 17, 33])
def test_capture_counts_around_the_stage(captures):
    """Runs that take exactly 1, 16, 17 and 33 captures: one fold per 16 captures and one for the fetch at the most."""
    n_steps = captures - 1
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    eng, _ = decay_engine("random", "f64", "single", plan, 5, 5)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert eng.decay_count() == (captures, n_steps)
        assert eng.query(E.Engine.QUERY_DECAY_FOLDS) <= (captures - 1) // 16   # (nothing is folded merely because a run ended)
        got, count = eng.fetch_decay()
        assert count == captures == eng.query(E.Engine.QUERY_DECAY_CAPTURES)
        assert eng.query(E.Engine.QUERY_DECAY_FOLDS) <= -(-captures // 16) + 1
    finally:
        eng.close()
    snaps, steps = reference_snapshots("random", "f64", "single", plan, 32)
    assert got.tobytes() == numpy_bins(snaps[:captures], 5, 5).tobytes() and got.max() > 0


def test_fetching_mid_run_and_at_the_end():
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    eng, _ = decay_engine("random", "f64", "pair", plan, 6, 5)
    assert eng.run_steps(13) == (13, 0)
    mid, mid_count = eng.fetch_decay()
    again, again_count = eng.fetch_decay()
    assert eng.run_steps(17) == (17, 0)
    end, end_count = eng.fetch_decay()
    eng.close()
    snaps, steps = reference_snapshots("random", "f64", "pair", plan, 30)
    assert (mid_count, again_count, end_count) == (14, 14, 31)
    assert mid.tobytes() == again.tobytes() == numpy_bins(snaps[:14], 6, 5).tobytes()
    assert end.tobytes() == numpy_bins(snaps, 6, 5).tobytes() and end.max() > 0
    assert (end[:2] == mid[:2]).all() and (end[2] >= mid[2]).all()       # full bins stay, the bin in progress grows


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("bad_step", [12, 13, 14])
def test_a_run_that_stops_on_a_flag_folds_no_capture_of_a_later_step(form, bad_step):
    """inf in the source signal at step f: the run completes f steps; with a capture every 4 steps the bins hold those of 0, 4, 8, 12
    and nothing of 16 (whose field the batch had already produced when the flag was read).  A following run goes on from there."""
    set_tuning(**FORMS[form])
    mesh = M.box_mesh(12, 12, 12)
    sig = np.zeros(40)
    sig[0] = 1.0
    sig[bad_step] = np.inf
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=sig,
                recv=[mesh.compute_index(7, 6, 6)])
    plan = dict(box=((0, 0, 6), (None, None, 1)), period=4)
    engines = [make_engine(case, "f64", plan), make_engine(case, "f64")]
    engines[1].set_decay(3, 2, **plan)
    memories = [engines[0].read_boundary_data(d) for d in (1, 2, 3)]
    for eng in engines:
        done, flag = eng.run_steps(40)
        assert done == bad_step and flag & M.ERR_INF
    snaps, steps = engines[0].fetch_snapshots()
    assert list(steps) == [0, 4, 8, 12]
    assert engines[1].decay_count() == (4, 12)
    got, count = engines[1].fetch_decay()
    assert count == 4 and np.isfinite(got).all() and got.max() > 0
    assert got.tobytes() == numpy_bins(snaps, 3, 2).tobytes()
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
    assert list(steps) == [0, 4, 8, 12, 16, 20] and engines[1].decay_count() == (6, 20)
    got, count = engines[1].fetch_decay()
    for eng in engines:
        eng.close()
    assert count == 6 and np.isfinite(got).all() and got[2].max() > 0
    assert got.tobytes() == numpy_bins(snaps, 3, 2).tobytes()


@pytest.mark.parametrize("form", ["single", "triple"])
def test_checkpoint_run_rollback_rerun_gives_the_same_bins_twice(form):
    plan = dict(box=((2, 3, 4), (12, 11, 9)), stride=(1, 2, 2), period=5)
    eng, _ = decay_engine("random", "f64", form, plan, 3, 2)
    assert eng.run_steps(10) == (10, 0)            # captures of 0, 5, 10
    eng.checkpoint()
    assert eng.run_steps(17) == (17, 0)            # 15, 20, 25
    first, first_count = eng.fetch_decay()
    eng.rollback()
    assert eng.step_count() == 10 and eng.decay_count() == (3, 10)
    kept, kept_count = eng.fetch_decay()
    assert eng.run_steps(17) == (17, 0)
    second, second_count = eng.fetch_decay()
    assert eng.decay_count() == (6, 25)
    # a plan set after the checkpoint has no bins to go back to
    eng.set_decay(3, 2, **plan)
    with pytest.raises(E.WaveguideError, match="error -6: .*after the checkpoint"):
        eng.rollback()
    eng.close()
    snaps, steps = reference_snapshots("random", "f64", form, plan, 27)
    assert (first_count, kept_count, second_count) == (6, 3, 6)
    assert kept.tobytes() == numpy_bins(snaps[:3], 3, 2).tobytes()
    assert first.tobytes() == second.tobytes() == numpy_bins(snaps, 3, 2).tobytes() and first.max() > 0


def test_generic_steps_in_between_capture_nothing():
    """wv_step / wv_swap capture nothing and the plan steps they pass are passed; a plan set at a non-zero step count captures that
    very step at the next run."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    plan = dict(box=((0, 0, 0), (None, None, 2)), period=3)
    engines = [make_engine(case, "f32"), make_engine(case, "f32")]
    for e in engines:
        assert e.run_steps(9) == (9, 0)
    engines[0].set_decay(2, 2, **plan)                # steps 0, 3, 6 lie before the plan; 9 is the count it is set at
    engines[1].set_snapshots(**plan)
    assert engines[0].decay_count() == (0, 0)
    for e in engines:
        assert e.run_steps(4) == (4, 0)               # 9 (at the start of this run), 12
        for _ in range(3):                            # 13 -> 16 by generic steps: 15 is passed
            assert e.step() == 0
            e.swap()
    assert engines[0].decay_count() == (2, 12)
    for e in engines:
        assert e.run_steps(2) == (2, 0)               # 18
    got, count = engines[0].fetch_decay()
    snaps, steps = engines[1].fetch_snapshots()
    assert list(steps) == [9, 12, 18] and count == 3
    assert got.tobytes() == numpy_bins(snaps, 2, 2).tobytes() and got.max() > 0
    engines[0].set_decay(None)                        # stops and forgets
    with pytest.raises(E.WaveguideError, match="error -6: .*no decay plan"):
        engines[0].decay_count()
    assert engines[0].run_steps(3) == (3, 0)
    for e in engines:
        e.close()


def test_refusals_leave_an_earlier_plan_intact():
    """n_bins 0 and 4097, zero bin_captures, a zero stride or period, a box off the mesh: WV_E_INVALID_ARGUMENT; either other plan while
    a decay plan is active and a decay plan while either other is: WV_E_STATE with the plan to stop in the message; after each refusal
    the earlier plan's results are what they were and it goes on capturing."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    snaps, _ = reference_snapshots("random", "f64", "single", plan, 32)
    eng = make_engine(case, "f64")
    eng.set_decay(4, 2, **plan)
    assert eng.run_steps(5) == (5, 0)
    before, before_count = eng.fetch_decay()
    for n_bins, bin_captures in ((0, 1), (4097, 1), (4, 0)):
        with pytest.raises(E.WaveguideError, match="error -1: .*(n_bins|bin_captures)"):
            eng.set_decay(n_bins, bin_captures, **plan)
    for bad_box in (((0, 0, 0), (25, 20, 28)), ((-1, 0, 0), (4, 4, 4)), ((0, 0, 28), (1, 1, 1))):
        with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
            eng.set_decay(4, 2, box=bad_box)
    with pytest.raises(E.WaveguideError, match="error -1: .*stride"):
        eng.set_decay(4, 2, box="mesh", stride=(1, 0, 1))
    with pytest.raises(E.WaveguideError, match="error -1: .*period"):
        eng.set_decay(4, 2, box="mesh", period=0)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*decay plan is active \(wv_set_decay\(e, NULL\)"):
        eng.set_snapshots(**plan)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*decay plan is active \(wv_set_decay\(e, NULL\)"):
        eng.set_spectrum([0.1], **plan)
    after, after_count = eng.fetch_decay()
    assert after_count == before_count == 6 and after.tobytes() == before.tobytes() == numpy_bins(snaps[:6], 4, 2).tobytes()
    assert eng.run_steps(3) == (3, 0) and eng.decay_count() == (9, 8)
    assert eng.fetch_decay()[0].tobytes() == numpy_bins(snaps[:9], 4, 2).tobytes() and after.max() > 0
    eng.close()
    # the other orders: a snapshot plan is active
    eng = make_engine(case, "f64", plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*snapshot plan is active \(wv_set_snapshots\(e, NULL\)"):
        eng.set_decay(4, 2, **plan)
    assert eng.run_steps(2) == (2, 0)
    got, steps = eng.fetch_snapshots()
    assert list(steps) == [0, 1, 2, 3, 4] and got.tobytes() == snaps[:5].tobytes()
    eng.close()
    # ... a spectrum plan is active
    eng = make_engine(case, "f64")
    eng.set_spectrum([0.0], **plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*spectrum plan is active \(wv_set_spectrum\(e, NULL, NULL\)"):
        eng.set_decay(4, 2, **plan)
    assert eng.run_steps(2) == (2, 0)
    spectrum, count = eng.fetch_spectrum()
    plain = np.zeros(snaps.shape[1:])
    for p in snaps[:5]:
        plain = plain + p.astype(np.float64)
    assert count == 5 and spectrum[0].real.tobytes() == plain.tobytes() and np.abs(plain).max() > 0
    eng.close()
    # a slab of a chain
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
        slab.set_decay(2, 2, box=((0, 0, 0), (4, 4, 1)))
    slab.close()
    # no plan: the library's WV_E_STATE; a group takes no engine with a plan
    eng = E.Engine(mesh, precision="f32")
    with pytest.raises(E.WaveguideError, match="error -6: .*no decay plan"):
        eng.fetch_decay()
    group = E.LocalSlabGroup([eng])
    eng.set_decay(2, 2, box=((0, 0, 0), (4, 4, 1)))
    with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no decay bins"):
        group.run_steps(4)
    eng.set_decay(None)
    assert group.run_steps(4) == (4, 0)
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
        if plan:
            eng.set_decay(4, 2, **plan)
        assert eng.run_steps(case["steps"]) == (case["steps"], 0)
        out.append([eng.fetch_receivers(0, case["steps"]), eng.read_field(E.BUF_CURRENT), eng.read_field(E.BUF_PREVIOUS)] +
                   [eng.read_boundary_data(d) for d in (1, 2, 3)])
        if plan:
            assert eng.decay_count() == (9, 59)   # steps 3, 10, ..., 59
        eng.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert np.abs(out[0][0]).max() > 0


def test_kernel_timing_accounts_for_the_fold_kernels():
    eng, _ = decay_engine("impulse_flat", "f64", "single", dict(box="mesh", period=1), 3, 8)
    eng.enable_kernel_timing(True)
    assert eng.run_steps(20) == (20, 0)
    eng.fetch_decay()
    assert eng.query(E.Engine.QUERY_DECAY_FOLDS) == 2 and eng.query(E.Engine.QUERY_DECAY_NS) > 0
    eng.close()


def _box_scene():
    from wayverb_amd import simulation as W
    mesh = M.box_mesh(24, 24, 24, coefficients=np.array([M.flat_coefficients(0.1)], dtype=M.coefficients_dtype))
    vm = W.VoxelsAndMesh(None, None, 0, None, None, mesh, (0.0, 0.0, 0.0))
    sp = mesh.spacing
    return W, vm, (12 * sp, 12 * sp, 12 * sp), (15 * sp, 12 * sp, 12 * sp)


def test_decay_maps_end_to_end_on_one_plane():
    """decay_maps on a decay-plan run of the 32^3 impulse room, one plane, eight captures per bin, every step, against decay.py applied
    to bins accumulated from the snapshots: equal, and the early decay time is finite wherever the level is.  128 captures in 16 bins:
    the first sound reaches the plane's corners after some 40 steps, which leaves every node ten edges behind its arrival.  The plane
    is z = 6, ten nodes from the hard source: in the plane next to the source (z = 15) the three nodes nearest to it hold more than
    90 % of their energy in the impulse itself, their curve falls 12.9 dB inside the first bin, no point lies in 0 .. -10 dB and the
    reference's edt throws there -- NaN by the definition, not a defect (the restated oracle on the CPU shows it; on z = 6 it shows all
    900 heard nodes finite, the unheard 124 being the outside shell)."""
    plan = dict(box=((0, 0, 6), (None, None, 1)), period=1)
    got, snaps = check("impulse_flat", "f32", "triple", plan, 16, 8, 127)
    rate = 8000.0
    maps = D.decay_maps(got[:, 0], 8, 1, rate)
    want = D.decay_maps(numpy_bins(snaps, 16, 8)[:, 0], 8, 1, rate)
    print("EDT: %d of %d nodes heard, %d finite; range %g .. %g s" % (np.isfinite(maps["level_db"]).sum(), maps["level_db"].size,
          np.isfinite(maps["edt_s"]).sum(), np.nanmin(maps["edt_s"]), np.nanmax(maps["edt_s"])))
    assert sorted(maps) == ["edc_db", "edt_r", "edt_s", "level_db", "t20_r", "t20_s", "t30_r", "t30_s"]
    for name in maps:
        assert maps[name].tobytes() == want[name].tobytes(), name
    assert maps["edt_s"].shape == maps["level_db"].shape == got.shape[2:] and maps["edc_db"].shape == (16,) + got.shape[2:]
    heard = np.isfinite(maps["level_db"])
    assert heard.any() and np.isfinite(maps["edt_s"][heard]).all() and (maps["edt_s"][heard] > 0).all()
    assert np.isnan(maps["edt_s"][~heard]).all()


def test_canonical_returns_the_bins_beside_the_receiver_output():
    """simulation.canonical(..., decay=...): the records are those of a run without a plan, the bins are the engine-level ones (binned
    from canonical's own snapshots of the same box and cadence); a second plan beside it is refused with the engine's message."""
    set_tuning()
    W, vm, source, receiver = _box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    box = ((0, 0, 12), (None, None, 1))
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=dict(box=box, period=2))
    bands, (bins, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                          decay=dict(n_bins=5, bin_captures=4, box=box, period=2))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 21 and bins.shape == (5, 1, 24, 24)
    assert bins.tobytes() == numpy_bins(fields, 5, 4).tobytes() and bins.max() > 0
    with pytest.raises(E.WaveguideError, match="error -6: .*snapshot plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, snapshots=dict(period=8), decay=dict(n_bins=2, bin_captures=2))
    with pytest.raises(E.WaveguideError, match="error -6: .*spectrum plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, spectrum=dict(freqs_hz=[10.0]), decay=dict(n_bins=2, bin_captures=2))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, decay=dict(n_bins=2, bin_captures=2))


def test_the_tool_writes_the_decay_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --decay-map z=... --decay-bin-ms --decay-every --decay-out FILE.npz on its built-in hall, a short run."""
    out = tmp_path / "decay.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.03",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--decay-map", "z=1.5", "--decay-bin-ms", "5",
                        "--decay-out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        bins, captures, per_bin, period, rate = f["bins"], int(f["captures"]), int(f["bin_captures"]), int(f["period"]), float(f["sample_rate"])
        level, edt, plane, origin, spacing = f["level_db"], f["edt_s"], int(f["plane"]), f["origin"], float(f["spacing"])
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    assert bins.dtype == np.float64 and bins.shape[1:] == (dims[1], dims[0]) and bins.shape[0] == -(-captures // per_bin)
    assert period == 3 and captures == steps // 3 + 1 and per_bin == max(1, int(round(0.005 * rate / 3)))
    assert 0 <= plane < dims[2] and origin.shape == (3,) and spacing > 0 and bins.max() > 0
    assert level.shape == edt.shape == bins.shape[1:] and np.isfinite(level).any()


def test_the_rate_tool_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/decay_rate.py on a 48^3 room, 48 steps per repeat: every row is there, the bins of the snapshot-and-host way equal the
    decay plan's bytewise in all four, and the figures land in the JSON file.  (Whether the bar holds is a matter of the 512^3 run, not
    of this size: the exit status may say either.)"""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "decay_rate.py"), "--side", "48", "--steps", "48",
                        "--bin-captures", "5", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode in (0, 1), p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 4 and "DECAY RATE" in p.stdout, p.stdout
    import json
    report = json.load(open(str(out)))
    rows = ["%s %s every %d" % (way, box, period) for way in "ab" for box in ("field", "plane") for period in (1, 3)]
    assert sorted(report["f64"]["rows"]) == sorted(rows)
    assert len(report["f64"]["verdicts"]) == 4 and all(v["bytewise_equal_to_old"] for v in report["f64"]["verdicts"].values())

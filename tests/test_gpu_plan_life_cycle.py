"""The life cycle of a capture plan that accumulates on the device -- capture, commit, fold, fetch, checkpoint, rollback, stop -- once
for all ten kinds.  csrc/engine_staged.hip.h and capture_stage.h hold one copy of it for every kind, so every test here runs every
kind through the table of tests/plan_twin.py, tests/eleven_kinds.py and tests/plan_cases.py, with the union of what the kinds' own
files used to assert one by one.  The reference of every comparison is a second, identical engine with a SNAPSHOT plan of what the
kind captures (the box, its hull, or the whole mesh for the ears of an interaural plan), whose snapshots the shipped definition folds
in capture order; equality is BYTEWISE on every output (plan_twin.assert_outputs).  Small meshes, forms forced, a few dozen steps.

What differs between the kinds is in tables: tests/plan_cases.py has the plan's own parameters test by test, as the kinds' files had
them (`details`), and the boxes of the kinds that need their neighbours on the grid (PLACES); here are the clauses a kind adds to a
test (GROWS, LAST_BIN)."""
import numpy as np
import pytest

import eleven_kinds as K
import plan_cases as C
import plan_twin as P
from helpers import set_tuning
from wayverb_amd import engine as E
from wayverb_amd import mesh as M

pytestmark = pytest.mark.gpu

KINDS10 = tuple(kind for kind in K.KINDS11 if kind != "snapshots")


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    C.default_tuning_afterwards()


@pytest.fixture(scope="module", autouse=True)
def eleven_kinds():
    with K.registered():
        yield


outputs, same, place, plan_for, SUB_BOX = C.outputs, P.assert_same, C.place, C.plan_for, C.SUB_BOX


def finite(got):
    return all(np.isfinite(v).all() for v in K.float_outputs(got).values())


# ---- capture counts around the stage ------------------------------------------------------------------------------------------------

# The ten kinds' own files name this test too, under the ids they always had, with the counts of plan_cases.FILE_COUNTS; here are the
# counts none of them names -- and all six for a kind that has no entry there.
COUNT_CASES = [(kind, captures) for kind in KINDS10 for captures in C.COUNTS if captures not in C.FILE_COUNTS.get(kind, ())]


@pytest.mark.parametrize("kind,captures", COUNT_CASES, ids=["%s-%d" % c for c in COUNT_CASES])
def test_capture_counts_around_the_stage(kind, captures):
    """Runs that take exactly 1, 15, 16, 17, 32 and 33 captures: one fold per 16 captures and one for the fetch at the most, nothing
    folded merely because a run ended; the bytes are the definition's over the first `captures` snapshots.  (The lateral plan in
    three-step passes on the odd box, one node per lane; the others in single steps with two.)"""
    C.capture_counts(kind, captures)


# ---- fetching mid-run and at the end --------------------------------------------------------------------------------------------------
# the kind's clause on (the outputs after 14 captures, after 31): full bins stay, the bin in progress grows

GROWS = {
    "decay": lambda mid, end: (end["bins"][:2] == mid["bins"][:2]).all() and (end["bins"][2] >= mid["bins"][2]).all(),
    "banded": lambda mid, end: (end["bins"][:, :2] == mid["bins"][:, :2]).all() and (end["bins"][:, 2] >= mid["bins"][:, 2]).all(),
    "intensity": lambda mid, end: (end["bins"][:, :2] == mid["bins"][:, :2]).all() and (end["bins"][3, 2] >= mid["bins"][3, 2]).all(),
    "modulation": lambda mid, end: (end["energy"] >= mid["energy"]).all(),
    "waterfall": lambda mid, end: end["waterfall"][:2].tobytes() == mid["waterfall"][:2].tobytes()
                                  and end["waterfall"][2].tobytes() != mid["waterfall"][2].tobytes(),
}


@pytest.mark.parametrize("kind", KINDS10)
def test_fetching_mid_run_and_at_the_end(kind):
    """13 steps, two fetches, 17 steps, a fetch: the first fetch folds 14 captures of a stage of 16, and the states it leaves carry the
    next 17; fetching twice changes nothing.  Onsets lie on both sides of the fetch."""
    row = C.kind_row(kind)
    plan = plan_for(kind, "mid_run", "random", SUB_BOX)
    snaps, steps = C.reference_snapshots("random", "f64", "pair", row.captures(plan), 30)
    plan = C.resolved(plan, snaps)
    eng = C.plan_engine("random", "f64", "pair", plan)
    try:
        assert eng.run_steps(13) == (13, 0)
        mid, again = outputs(eng, kind), outputs(eng, kind)
        assert eng.run_steps(17) == (17, 0)
        end = outputs(eng, kind)
    finally:
        eng.close()
    assert (mid["count"], again["count"], end["count"]) == ((14, 13), (14, 13), (31, 30))
    assert [o.get("captures", o["count"][0]) for o in (mid, again, end)] == [14, 14, 31]
    want_mid, want_end = C.expected(plan, snaps[:14], steps[:14]), C.expected(plan, snaps, steps)
    same(mid, want_mid, (kind, "mid"))
    same(again, want_mid, (kind, "again"))
    same(end, want_end, (kind, "end"))
    assert row.meaningful(want_mid, plan) and row.meaningful(want_end, plan, at=13)
    assert kind not in GROWS or GROWS[kind](mid, end)


# ---- the same steps in calls of 1, 7 and 30 -----------------------------------------------------------------------------------------------

CALL_CASES = [("pair", "f64", 1), ("pair", "f32", 1), ("single", "f32", 2), ("triple", "f32", 2)]


@pytest.mark.parametrize("form,tag,period", CALL_CASES, ids=["%s-%s-every%d" % c for c in CALL_CASES])
@pytest.mark.parametrize("kind", KINDS10)
def test_calls_of_1_7_and_30_steps_give_the_same_bytes(kind, form, tag, period):
    """30 steps in calls of 1, 7 and 30: the definition's bytes whichever way; in calls of 7 a fetch after 14 steps (a fold of 15
    captures, then 15 more: a ring of 16 slots wraps inside the second)."""
    row = C.kind_row(kind)
    plan = plan_for(kind, "calls", "random", SUB_BOX, period=period)
    snaps, steps = C.reference_snapshots("random", tag, form, row.captures(plan), 30)
    plan = C.resolved(plan, snaps)
    want = C.expected(plan, snaps, steps)
    assert want["count"] == (30 // period + 1, 30) and row.meaningful(want, plan)
    for call in (1, 7, 30):
        eng = C.plan_engine("random", tag, form, plan)
        try:
            done = 0
            while done < 30:
                n = min(call, 30 - done)
                assert eng.run_steps(n) == (n, 0)
                done += n
                if call == 7 and done == 14:
                    held = 14 // period + 1
                    same(outputs(eng, kind), C.expected(plan, snaps[:held], steps[:held]), (kind, "mid"))
            same(outputs(eng, kind), want, (kind, call))
        finally:
            eng.close()


# ---- a run that stops on a flag ---------------------------------------------------------------------------------------------------------
# the kind's clause on the continued run's outputs: the last bin took something

LAST_BIN = {
    "decay": lambda got: got["bins"][2].max() > 0,
    "banded": lambda got: got["bins"][:, 2].max() > 0,
    "intensity": lambda got: got["bins"][3, 2].max() > 0,
    "waterfall": lambda got: np.abs(got["waterfall"][2]).max() > 0,
    "arrival_bands": lambda got: (got["bins"][:, -1] > 0).any(),
}


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("bad_step", [12, 13, 14])
@pytest.mark.parametrize("kind", KINDS10)
def test_a_run_that_stops_on_a_flag_folds_no_capture_of_a_later_step(kind, bad_step, form):
    """inf in the source signal at step f: the run completes f steps; with a capture every 4 steps the plan holds those of 0, 4, 8, 12
    and nothing of 16, whose field (inf / nan) the batch had already produced when the flag was read -- in no sum, no onset and no
    filter state.  The next run continues: the failed steps left inf / nan behind, so both engines get the same finite fields, clean
    filter memories and a finite source; the capture of step 16, dropped above, is due again, the plan goes on counting from capture 4,
    and its outputs are the definition's over the six snapshots in one go, finite."""
    set_tuning(**C.FORMS[form])
    mesh = M.box_mesh(12, 12, 12)
    sig = np.zeros(40)
    sig[0] = 1.0
    if kind == "intensity":
        sig[1] = 0.5     # (both parities of the mesh: after an impulse alone a node and its neighbours are never non-zero at the same step, and I is 0)
    sig[bad_step] = np.inf
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=sig,
                recv=[mesh.compute_index(7, 6, 6)])
    row = C.kind_row(kind)
    plan = plan_for(kind, "flag", mesh.dims, place(kind, "flag"), period=4)
    engines = [C.make_engine(case, "f64", row.captures(plan)), C.make_engine(case, "f64")]
    try:
        P.set_plan(engines[1], plan)
        memories = [engines[0].read_boundary_data(d) for d in (1, 2, 3)]
        for eng in engines:
            done, flag = eng.run_steps(40)
            assert done == bad_step and flag & M.ERR_INF
        snaps, steps = engines[0].fetch_snapshots()
        assert list(steps) == [0, 4, 8, 12]
        got = outputs(engines[1], kind)
        want = C.expected(plan, snaps, steps)
        assert got["count"] == (4, 12) and got.get("captures", 4) == 4 and finite(got) and row.meaningful(want, plan)
        same(got, want, (kind, "stopped"))
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
        assert list(steps) == [0, 4, 8, 12, 16, 20]
        got = outputs(engines[1], kind)
    finally:
        for eng in engines:
            eng.close()
    want = C.expected(plan, snaps, steps)
    assert got["count"] == (6, 20) and got.get("captures", 6) == 6 and finite(got) and row.meaningful(want, plan)
    same(got, want, (kind, "continued"))
    assert kind not in LAST_BIN or LAST_BIN[kind](got)


# ---- checkpoint, run, rollback, rerun -----------------------------------------------------------------------------------------------------

def rollback_case(kind):
    """(case, box, cadence, the two runs, the capture the checkpoint lies behind where the test wants onsets on both sides of it).  The
    kinds that sum: captures of 0, 5, 10, then 15, 20, 25 of a strided box of "random".  The kinds that wait for an onset: the impulse
    room's plane at every step -- the wavefront is crossing it at the checkpoint, so some onsets lie before it and some behind.  The
    interaural plan: every second step of the strided box, 6 captures, then 17 more with a full stage among them."""
    if kind in ("arrival", "lateral", "arrival_bands"):
        return "impulse_flat", place(kind, "plane"), dict(period=1), (10, 17), 10
    return "random", place(kind, "rollback"), dict(stride=(1, 2, 2), period=2 if kind == "interaural" else 5), (10, 34 if kind == "interaural" else 17), None


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("kind", KINDS10)
def test_checkpoint_run_rollback_rerun_gives_the_same_outputs_twice(kind, form):
    """The checkpoint holds sums, onsets AND filter states: after the rollback the captures that follow are folded from the state the
    checkpoint's last capture left, and the re-run's outputs are the first run's and the definition's.  A plan set after the checkpoint
    has nothing to go back to: a new plan REPLACES the old one and forgets, and wv_rollback refuses in its full sentence."""
    case, box, cadence, (before, after), at = rollback_case(kind)
    row = C.kind_row(kind)
    plan = plan_for(kind, "rollback", case, box, **cadence)
    snaps, steps = C.reference_snapshots(case, "f64", form, row.captures(plan), before + after)
    plan = C.resolved(plan, snaps)
    kept_captures = before // plan["period"] + 1
    want_kept, want = C.expected(plan, snaps[:kept_captures], steps[:kept_captures]), C.expected(plan, snaps, steps)
    assert row.meaningful(want, plan, at=at)
    eng = C.plan_engine(case, "f64", form, plan)
    try:
        assert eng.run_steps(before) == (before, 0)
        eng.checkpoint()
        assert eng.run_steps(after) == (after, 0)
        first = outputs(eng, kind)
        eng.rollback()
        assert eng.step_count() == before and row.count(eng) == want_kept["count"]
        kept = outputs(eng, kind)
        assert eng.run_steps(after) == (after, 0)
        second = outputs(eng, kind)
        P.set_plan(eng, plan)
        assert row.count(eng) == (0, 0)
        C.refuses(eng.rollback, row.rollback)
        empty = outputs(eng, kind)
        row.stop(eng)                                  # stops and forgets
        C.refuses(lambda: row.count(eng), row.no_plan["count"])
        C.refuses(lambda: row.fetch(eng), row.no_plan["fetch"])
        assert eng.run_steps(3) == (3, 0)
    finally:
        eng.close()
    assert want_kept["count"] == (kept_captures, before) and want["count"] == (len(steps), int(steps[-1])) and before < int(steps[-1]) <= before + after
    same(kept, want_kept, (kind, "kept"))
    assert kind != "waterfall" or row.meaningful(want_kept, plan)       # (three captures already fill its sums)
    same(first, want, (kind, "first"))
    same(second, want, (kind, "second"))
    same(empty, C.expected(plan, snaps[:0], steps[:0]), (kind, "empty"))


# ---- generic steps in between ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS10)
def test_generic_steps_in_between_capture_nothing(kind):
    """wv_step / wv_swap capture nothing and the plan steps they pass are passed -- gaps in the series the filters see; a plan set at a
    non-zero step count captures that very step at the next run: the pinned example of period 3 set at step 9.  The plan's own setter
    stops it, its count and fetch then refuse in their full sentences, and a decay plan takes its place."""
    set_tuning(**C.FORMS["pair"])
    case = C.case_of("random")
    row = C.kind_row(kind)
    plan = plan_for(kind, "generic", "random", place(kind, "generic"), period=3)
    engines = [C.make_engine(case, "f32"), C.make_engine(case, "f32")]
    try:
        for e in engines:
            assert e.run_steps(9) == (9, 0)
        P.set_plan(engines[0], plan)                      # steps 0, 3, 6 lie before the plan; 9 is the count it is set at
        engines[1].set_snapshots(**row.captures(plan))
        assert row.count(engines[0]) == (0, 0)
        for e in engines:
            assert e.run_steps(4) == (4, 0)               # 9 (at the start of this run), 12
            for _ in range(3):                            # 13 -> 16 by generic steps: 15 is passed
                assert e.step() == 0
                e.swap()
        assert row.count(engines[0]) == (2, 12)
        for e in engines:
            assert e.run_steps(2) == (2, 0)               # 18
        got = outputs(engines[0], kind)
        snaps, steps = engines[1].fetch_snapshots()
        assert list(steps) == [9, 12, 18]
        want = C.expected(plan, snaps, steps)
        assert got["count"] == (3, 18) and got.get("captures", 3) == 3
        same(got, want, kind)
        assert row.meaningful(want, plan) and (kind not in ("arrival", "lateral", "arrival_bands") or C.heard_and_unheard(want))
        assert kind not in ("waterfall", "interaural") or np.abs(got[row.answer[1]][1]).max() > 0       # the second bin took something
        row.stop(engines[0])                              # stops, forgets and frees ...
        C.refuses(lambda: row.count(engines[0]), row.no_plan["count"])
        C.refuses(lambda: row.fetch(engines[0]), row.no_plan["fetch"])
        decay = C.cadence_of(plan)
        engines[0].set_decay(2, 2, **decay)               # ... and a decay plan takes its place
        assert engines[0].run_steps(3) == (3, 0) and engines[0].decay_count() == (2, 21)
        assert engines[0].fetch_decay()[0].max() > 0
    finally:
        for e in engines:
            e.close()


# ---- a plan changes nothing the run computes -------------------------------------------------------------------------------------------

# The ten kinds' own files name this test too, under the ids they always had, in the forms of plan_cases.FILE_FORMS; here are the forms
# none of them names -- and every form for a kind that has no entry there.
NOTHING_CASES = [(kind, form) for kind in KINDS10 for form in sorted(C.ALL_FORMS) if form not in C.FILE_FORMS.get(kind, ())]


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("kind,form", NOTHING_CASES, ids=["%s-%s" % c for c in NOTHING_CASES])
def test_a_plan_changes_nothing_the_run_computes(kind, form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise."""
    C.changes_nothing(kind, tag, form)


# ---- kernel timing ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS10)
def test_kernel_timing_accounts_for_the_fold_and_the_gather_kernels(kind):
    """The queries are 0 before the first capture; a run of n steps takes n + 1 captures and folds a stage whenever a 17th arrives, the
    fetch folds the rest; the time of the fold kernels is accounted for, and of the gather kernels of the kinds that gather ahead of
    the fold, one launch per capture; no other kind's fold ran.  (20 steps; 40 for the kinds that wait for an onset.)"""
    n = 40 if kind in ("arrival", "lateral", "arrival_bands") else 20
    row = C.kind_row(kind)
    eng = C.plan_engine("impulse_flat", "f64", "single", plan_for(kind, "timing", "impulse_flat", place(kind, "timing")))
    try:
        assert [eng.query(q) for q in row.queries.values()] == [0] * len(row.queries)
        eng.enable_kernel_timing(True)
        assert eng.run_steps(n) == (n, 0)
        assert eng.query(row.queries["captures"]) == n + 1 and eng.query(row.queries["folds"]) == n // 16
        row.fetch(eng)
        assert eng.query(row.queries["folds"]) == n // 16 + 1 <= -(-(n + 1) // 16) + 1 and eng.query(row.queries["ns"]) > 0
        if "gathers" in row.queries:
            assert eng.query(row.queries["gathers"]) == n + 1 and eng.query(row.queries["gather_ns"]) > 0
        others = {C.COLUMNS[k].queries["folds"] for k in KINDS10} - {row.queries["folds"]}
        assert all(eng.query(q) == 0 for q in others)
    finally:
        eng.close()

"""Capture plans -- snapshots, field spectra, decay maps (plain and band-limited), intensity, arrival, lateral, modulation and banded
arrival maps -- through random rooms and random sequences of API calls, against the oracle: tests/plan_twin.py draws the room (box,
L, blob, sphere; rows of one wave and of three) and the calls (runs of random lengths, steps driven from outside, values / fields /
filter memories written between them, the source moved, the receivers replaced, a plan set mid-sequence or replaced by another,
outputs fetched mid-way, checkpoints and rollbacks) and says, with no GPU in it, what the engine must show after each of them.  Four
families of scripts (plan_twin.FAMILIES): `plans` hands six kinds over to each other; `all-plans` eight, and adds a plan replaced by
one of its own kind with no stop in between, a setter of another kind that must be refused in plan_refused's words, a rollback that
must be refused, and a plan stopped with calls going on before the next one is set; `modulation` and `arrival-bands` stay with one
kind.  all_tiles is off, so rooms that leave mesh outside are marched from their work lists; the stepping form is the engine's own
choice or a forced one.  After EVERY call both fields, at every fetch, handover, stop and the end every output of the active plan, and
at the end the step count, the filter memories and the receiver rows must be the twin's BYTEWISE: the definitions are exact, no
tolerance appears anywhere.

What this is after: a capture that reads a stale x-wall copy, a node of a unit that is never visited, a field whose role was swapped
by an odd batch, a step whose source sample already rode in the launch before it; something one kind of plan leaves behind for the
next through the life cycle they share (csrc/engine_staged.hip.h) -- a stage, an event, a saved block, a `next`, a generation that
makes a rollback refuse or fail to -- and the per-lane state of the folds under boxes, strides, periods, threshold maps, rollbacks in
the middle of a stage and gaps of outside steps that no fixed scenario of the plans' own files draws."""
import pytest

import plan_twin as P
from helpers import set_tuning
from wayverb_amd import engine as E

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "passes": dict(pair=1), "three-step-passes": dict(pair=1, triple=1),
         "three-step-passes-all-units": dict(pair=1, triple=1, tile_lists=0), "single-steps": dict(pair=0),
         "two-launch-steps": dict(pair=0, whole_step=0), "graph-and-passes": dict(pair=1, graph=1)}
FAMILY_MODES = {"plans": tuple(MODES), "all-plans": ("default", "three-step-passes", "single-steps", "graph-and-passes"),
                "modulation": ("default", "three-step-passes", "single-steps"), "arrival-bands": ("default", "three-step-passes", "single-steps")}
# the modes of one seed follow each other, so that one script is held at a time.  (`all-plans` is parametrised in
# tests/test_gpu_all_plan_sequences.py, under the names its 128 cases have always had; it runs through run_case like the others.)
CASES = [(family, seed, mode) for family, modes in FAMILY_MODES.items() if family != "all-plans"
         for seed in range(P.FAMILIES[family].seeds) for mode in modes]

_script = {}     # (family, seed) -> the twin's script of the seed at hand
# family -> mode -> seed -> (two-step passes, three-step passes, one-launch steps, share of the mesh marched)
_tally = {family: {mode: {} for mode in modes} for family, modes in FAMILY_MODES.items()}


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


def script_of(oracle, family, seed):
    if (family, seed) not in _script:
        _script.clear()
        _script[family, seed] = P.build_script(oracle, family, seed)
    return _script[family, seed]


def run_case(oracle, family, seed, mode):
    script = script_of(oracle, family, seed)
    set_tuning(**MODES[mode])
    eng = E.Engine(script["mesh"], precision=script["tag"], all_tiles=False)
    try:
        P.replay(eng, script)
        _tally[family][mode][seed] = (eng.query(E.Engine.QUERY_PASSES), eng.query(E.Engine.QUERY_TRIPLE_PASSES), eng.query(E.Engine.QUERY_WHOLE_STEPS),
                                      eng.query(E.Engine.QUERY_MARCH_LIVE_PERMILLE))
    finally:
        eng.close()


# (the cases of `plans` keep the names they had before there were families)
@pytest.mark.parametrize("family,seed,mode", CASES, ids=["-".join(str(v) for v in (case[1:] if case[0] == "plans" else case)) for case in CASES])
def test_random_plan_sequence(oracle, built_library, family, seed, mode):
    run_case(oracle, family, seed, mode)


def met_in_a_quarter_of_the_seeds(family, conditions):
    """Over the seeds that ran in this process, and only if all of them did."""
    tally, seeds = _tally[family], P.FAMILIES[family].seeds
    if any(len(tally[mode]) < seeds for mode in tally):
        return
    met = {"%s: %s" % (mode, what): sum(1 for t in tally[mode].values() if holds(t)) for mode, what, holds in conditions}
    print(met)
    for what, n in met.items():
        assert 4 * n >= seeds, (what, n)


def test_every_mode_met_its_form():
    """`plans`: each mode took the form it is named after, and the two modes with work lists marched less than the whole mesh, in a
    quarter of the seeds at the least."""
    met_in_a_quarter_of_the_seeds("plans", [
        ("passes", "two-step passes", lambda t: t[0] > 0),
        ("three-step-passes", "three-step passes", lambda t: t[1] > 0),
        ("default", "one-launch steps", lambda t: t[2] > 0),
        ("single-steps", "one-launch steps", lambda t: t[2] > 0),
        ("passes", "less than the whole mesh marched", lambda t: t[3] < 1000),
        ("three-step-passes", "less than the whole mesh marched", lambda t: t[3] < 1000)])

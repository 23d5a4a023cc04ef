"""Every ordered pair of the eleven kinds of capture plan, one handing over to the other: 121 pairs, the 11 of a kind with itself
included, in single steps and in three-step passes.  All eleven share staged_install, plan_release, the per-kind Checkpoint::PlanSave
(reused when sizes match, reallocated when they differ) and the generation counter (csrc/engine_staged.hip.h); the random `all-plans`
family of tests/test_gpu_all_plan_sequences.py draws eight kinds, and the banded arrival, waterfall and interaural plans run only in
families of their own kind, so of the 110 ordered pairs of different kinds the 54 with one of the three newest had never been run --
nor had any plan been replaced by one of its own kind of ANOTHER state size across two checkpoints.  Nothing here is random but the
noise in the fields: one script for every pair (eleven_kinds.handover_script has it, step by step), built on the oracle with
plan_twin.PlanTwin and played by plan_twin.replay, which compares both fields after every call, every output of the active plan at
every fetch, handover and stop -- a refused setter changes nothing, a refused rollback changes nothing, a rollback gives the count and
every output as at the checkpoint, the second pass of 19 steps gives bytewise what the first gave -- and at the end the step count,
the filter memories and the receiver rows, all BYTEWISE.

A 12^3 box with filtered walls, noise in both fields, a hard source of 80 noise samples, one receiver; f32 where the two kinds' places
in KINDS11 add up to an odd number, f64 otherwise.  tests/test_eleven_kinds.py holds on the CPU that in every script both plans have
captures, that b folds before and after its checkpoint, and that its outputs are not all zeros."""
import pytest

import eleven_kinds as K
import plan_twin as P
from helpers import set_tuning
from test_gpu_snapshots import FORMS
from wayverb_amd import engine as E

pytestmark = pytest.mark.gpu

PAIRS = [(a, b) for a in K.KINDS11 for b in K.KINDS11]
assert len(PAIRS) == 121

_script = {}     # (a, b) -> the script of the pair at hand: the two forms of a pair follow each other


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


@pytest.fixture(scope="module")
def eleven_kinds():
    with K.registered():
        yield


def script_of(oracle, a, b):
    if (a, b) not in _script:
        _script.clear()
        _script[a, b] = K.handover_script(oracle, a, b, f32=(K.KINDS11.index(a) + K.KINDS11.index(b)) % 2 == 1)[0]
    return _script[a, b]


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("a,b", PAIRS, ids=["%s-to-%s" % pair for pair in PAIRS])
def test_one_kind_hands_over_to_another(oracle, eleven_kinds, a, b, form):
    script = script_of(oracle, a, b)
    set_tuning(**FORMS[form])
    eng = E.Engine(script["mesh"], precision=script["tag"])
    try:
        P.replay(eng, script)
    finally:
        eng.close()

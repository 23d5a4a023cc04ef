"""What the capture plans' setters SAY to a faulty argument, code and whole sentence, against tests/golden/plan_argument_refusals.json:
every single fault a setter can refuse -- a stride of 0, a period of 0, a box one node past each face of the mesh, and the plan's own:
counts, edges, thresholds, a NaN frequency, an infinite coefficient, a non-positive constant, a bad entry of a threshold map, a node on a
face of the mesh for the two plans that take gradients -- and every ORDERED PAIR of two of them at once: which of the two is said is part
of what a caller sees.  tests/plan_argument_faults.py holds the cases and records the fixture; it was recorded from the commit before the
setters' shared checks were given one statement (snapshot_plan.h), so the move changed no code, no sentence and no precedence.

No stepping: a 12 x 10 x 9 box mesh in fp32, a plan of 24 nodes.  After EVERY case, single or pair, the step count and both fields are
what they were, byte for byte, the valid plan is taken, and stopping it again leaves them so.  (The refusal of a plane of 2^31 nodes
needs a mesh no device holds: tests/cpp/snapshot_plan_test.cpp holds it on the shared function.)"""
import json

import pytest

import plan_argument_faults as F

pytestmark = pytest.mark.gpu

WV_E_INVALID_ARGUMENT = -1    # (include/wayverb_amd.h)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(F.GOLDEN))


@pytest.fixture(scope="module")
def eng(built_library):
    engine = F.make_engine()
    yield engine
    engine.close()


@pytest.mark.parametrize("kind", F.KINDS)
def test_single_faults_and_ordered_pairs_are_refused_in_the_recorded_words(eng, golden, kind):
    want = golden[kind]
    assert want["faults"] == list(F.FAULTS[kind]) and sorted(want["single"]) == sorted(want["pairs"]) == sorted(want["faults"])
    before = F.state(eng)

    def words(index):
        return None if index is None else want["answers"][index]

    def unchanged_and_usable(case):
        assert F.state(eng) == before, case
        assert F.answer(eng, kind, []) is None, case                       # the valid plan is still taken (and stopped again)
        assert F.state(eng) == before, case

    for name in want["faults"]:
        assert want["single"][name] is not None, name                      # a single fault is always refused
        assert F.answer(eng, kind, [name]) == words(want["single"][name]), name
        unchanged_and_usable(name)
    for first in want["faults"]:
        for second, index in zip(want["faults"], want["pairs"][first]):
            assert F.answer(eng, kind, [first, second]) == words(index), (first, second)
            unchanged_and_usable((first, second))


def test_the_fixture_covers_what_it_says(golden):
    """Every setter's distinct answers are WV_E_INVALID_ARGUMENT (or 'null argument') sentences that begin with the setter's name or are
    the reference's sentence for a node beside a face; the shared four are said by all eight setters."""
    names = {"snapshots": "wv_set_snapshots", "spectrum": "wv_set_spectrum", "decay": "wv_set_decay", "decay_bands": "wv_set_decay_bands",
             "intensity": "wv_set_intensity", "arrival": "wv_set_arrival", "lateral": "wv_set_lateral", "modulation": "wv_set_modulation"}
    assert sorted(k for k in golden if k != "decay split") == sorted(F.KINDS)
    for kind in F.KINDS:
        sentences = [text for _, text in golden[kind]["answers"]]
        assert all(code == WV_E_INVALID_ARGUMENT for code, _ in golden[kind]["answers"]), kind
        for tail in (": strides must be >= 1", ": period must be >= 1", ": the box leaves the mesh"):
            assert names[kind] + tail in sentences, (kind, tail)
        for text in sentences:
            assert text.startswith(names[kind] + ": ") or text == "null argument" or text.startswith("Can't place directional_receiver"), (kind, text)
        # two faults at once are seldom both harmless: a handful of pairs undo each other (one origin overwrites the other)
        taken = sum(index is None for row in golden[kind]["pairs"].values() for index in row)
        assert taken < len(golden[kind]["faults"]) ** 2 // 4, kind


def test_the_decay_setters_refuse_the_other_kind_of_decay_plan_before_any_argument(eng, golden):
    """Under a plain decay plan wv_set_decay_bands says so whatever its arguments are, and the other way round: WV_E_STATE, one
    sentence per direction."""
    before = F.state(eng)
    want = golden["decay split"]
    assert F.observe_split(eng) == want
    for setter, other in (("decay_bands", "a plain decay plan is active"), ("decay", "a banded decay plan is active")):
        assert sorted(want[setter]) == sorted(["valid"] + list(F.FAULTS[setter]))
        answers = {tuple(a) for a in want[setter].values()}
        assert len(answers) == 1 and other in next(iter(answers))[1], setter
    assert F.state(eng) == before

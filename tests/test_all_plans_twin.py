"""The generator and the reference of tests/test_gpu_plan_sequences.py's family `all-plans` alone, on the CPU: the oracle, no engine.  What the comparison
on the GPU needs before it means anything -- every one of the eight kinds of plan fetched with something in it, plans of every kind
handed over to plans of other kinds, replaced by plans of their own, stopped and followed by others, refused setters and refused
rollbacks, rollbacks across captures, more captures under one plan than a stage holds, lateral plans with several onsets and bins --
is counted over all seeds and asserted here; the counts' bounds are the issue's, and the generator's probabilities
(its weights in plan_twin.FAMILIES) were chosen to meet them.  `python tests/test_all_plans_twin.py` prints the table of the counts."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

import plan_twin as T
from wayverb_amd import lateral as L
from wayverb_amd import mesh as M

FAMILY = T.FAMILIES["all-plans"]


def counts(stats):
    """Every figure the conditions are about, by name."""
    def scripts(what):
        return sum(1 for s in stats if what(s))
    pairs = set().union(*[s["pairs"] for s in stats])
    return {
        "scripts in which each kind is fetched with something non-zero": {k: scripts(lambda s: k in s["fetched"]) for k in T.KINDS8},
        "distinct ordered (from, to) pairs of different kinds": len(pairs),
        "pairs with each kind as from": {k: sum(1 for a, _ in pairs if a == k) for k in T.KINDS8},
        "pairs with each kind as to": {k: sum(1 for _, b in pairs if b == k) for k in T.KINDS8},
        "further pairs met only across a stop": len(set().union(*[s["pairs_over_a_stop"] for s in stats]) - pairs),
        "scripts with a rollback across captures": scripts(lambda s: s["rolled_across"]),
        "scripts with a capture strictly inside a run of six steps or more": scripts(lambda s: s["cut_segment"]),
        "scripts with a same replacement": scripts(lambda s: s["same"]),
        "scripts with a refused-plan": scripts(lambda s: s["refused_plans"]),
        "scripts with a refused-rollback": scripts(lambda s: s["refused_rollbacks"]),
        "what the refused rollbacks were refused for": sorted(set().union(*[s["refused_for"] for s in stats])),
        "scripts with a stop followed by a run and a new plan": scripts(lambda s: s["stop_run_plan"]),
        "scripts that hold more than 16 captures under a single plan": scripts(lambda s: s["most_under_one_plan"] > 16),
        "scripts that end with fewer than 2 captures in total": scripts(lambda s: s["captures"] < 2),
        "distinct lateral onset values": len(set().union(*[s["onsets"] for s in stats])),
        "lateral nodes fetched with an onset": sum(s["with_onset"] for s in stats),
        "lateral nodes fetched without an onset": sum(s["without_onset"] for s in stats),
        "scripts in which a lateral fetch has 3 or more bins of E non-zero": scripts(lambda s: s["lateral_bins"] >= 3),
        "most steps run in one script": max(s["steps"] for s in stats),
    }


@pytest.fixture(scope="module")
def scripts(oracle, built_library):
    return [T.build_script(oracle, "all-plans", seed) for seed in range(FAMILY.seeds)]


@pytest.fixture(scope="module")
def met(scripts):
    table = counts([s["stats"] for s in scripts])
    for name, value in table.items():
        print("%-70s %s" % (name, value))
    return table


def test_every_kind_is_first_in_every_room_and_once_in_f32(scripts):
    first = {(s["stats"]["first"], s["room"]) for s in scripts}
    assert first == {(k, r) for k in T.KINDS8 for r in ("box", "L", "blob", "sphere")}
    assert sorted(s["stats"]["first"] for s in scripts if s["tag"] == "f32") == sorted(T.KINDS8)
    assert all(20 <= len(s["ops"]) <= 33 for s in scripts)


def test_every_kind_of_plan_is_fetched_with_something_in_it(met):
    for kind, n in met["scripts in which each kind is fetched with something non-zero"].items():
        assert n >= 4, kind


def test_plans_of_every_kind_are_handed_over_to_other_kinds(met):
    assert met["distinct ordered (from, to) pairs of different kinds"] >= 28
    for kind in T.KINDS8:
        assert met["pairs with each kind as from"][kind] >= 3, kind
        assert met["pairs with each kind as to"][kind] >= 3, kind


def test_rollbacks_cross_captures(met):
    assert met["scripts with a rollback across captures"] >= 8


def test_captures_fall_inside_runs_of_six_steps_and_more(met):
    assert met["scripts with a capture strictly inside a run of six steps or more"] >= 10


def test_plans_are_replaced_by_plans_of_their_own_kind(met):
    assert met["scripts with a same replacement"] >= 6


def test_setters_and_rollbacks_are_refused(met):
    assert met["scripts with a refused-plan"] >= 8
    assert met["scripts with a refused-rollback"] >= 5
    assert met["what the refused rollbacks were refused for"] == ["plan", "receivers", "source"]


def test_plans_are_stopped_and_others_set_after_a_run_without_one(met):
    assert met["scripts with a stop followed by a run and a new plan"] >= 5


def test_single_plans_hold_more_captures_than_one_stage(met):
    assert met["scripts that hold more than 16 captures under a single plan"] >= 8


def test_few_sequences_end_with_fewer_than_two_captures(met):
    assert met["scripts that end with fewer than 2 captures in total"] <= 3


def test_lateral_plans_see_onsets_and_bins(met):
    assert met["distinct lateral onset values"] >= 5
    assert met["lateral nodes fetched with an onset"] > 0 and met["lateral nodes fetched without an onset"] > 0
    assert met["scripts in which a lateral fetch has 3 or more bins of E non-zero"] >= 3


def test_sequences_stay_small(met):
    assert met["most steps run in one script"] <= 400


def test_refusals_hold_the_active_plans_words(scripts):
    """Every refused-plan op names the plan that was active, the setter that was called, and no other plan."""
    seen = 0
    for s in scripts:
        active = None
        for op in s["ops"]:
            if op["op"] in ("plan", "same"):
                active = op["plan"]["kind"]
            elif op["op"] == "stop":
                active = None
            elif op["op"] == "refused-plan":
                seen += 1
                assert op["plan"]["kind"] != active and op["words"].startswith(T.KINDS[op["plan"]["kind"]].setter + ": ")
                assert sum(1 for k in T.KINDS.values() if k.active in op["words"]) == (0 if (active, op["plan"]["kind"]) == ("decay", "banded") else 1)
                assert T.KINDS[active].active in op["words"] or "a plain decay plan is active" in op["words"]
    assert seen >= 8


PINNED_THRESHOLD = 0.02
PINNED_ONSET = [[[0, 1, 0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0, 1, 0], [0, 1, -1, 1, -1, 1, 0, 1], [1, 0, 1, 0, 1, 0, 1, 0], [0, 1, 0, 1, 0, 1, 0, 1],
                 [1, 0, 1, 0, 1, 0, 1, 0]],
                [[1, -1, 1, -1, 1, 0, 1, 0], [-1, 1, 0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0, 1, 0], [-1, 1, 0, 2, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0, 1, 0],
                 [0, 1, 0, 1, 0, 1, -1, 1]]]      # [z][y][x] of the box, -1 where no onset


def test_the_pinned_example_of_generic_steps_in_between_for_a_lateral_plan(oracle):
    """test_generic_steps_in_between_capture_nothing of tests/test_gpu_lateral.py on the twin: a lateral plan of period 3 set at step 9
    captures 9 at the start of the next run and 12 in it, three generic steps pass 15, and the next run captures 18 -- captures 0, 1
    and 2 of the plan, which the onsets are numbered by.  An impulse moves one colour of the checkerboard at a time: the nodes an odd
    number of links from (5, 5, 4) hold something at step 9 (onset 0), the others at step 12 (onset 1); seven nodes stay below the
    threshold of 0.02 in all three captures, one reaches it only at step 18 (onset 2).  No |p| lies within 5 % of the threshold."""
    mesh = M.box_mesh(12, 10, 9)
    twin = T.PlanTwin(oracle, mesh, np.float32)
    twin.cur[mesh.compute_index(5, 5, 4)] = np.float32(1.0)
    assert twin.run(9) == 9
    plan = dict(kind="lateral", box=((2, 2, 3), (8, 6, 2)), stride=(1, 1, 1), first_step=0, period=3, edges=[0, 1], threshold=PINNED_THRESHOLD,
                threshold_map=None)
    twin.set_plan(plan)
    assert twin.expected()["count"] == (0, 0) and (twin.expected()["onset"] == L.NONE).all()
    assert twin.run(4) == 4
    for _ in range(3):
        twin.outside_step()
    assert [s for s, _ in twin.log] == [9, 12]
    assert twin.run(2) == 2
    want = twin.expected()
    assert [s for s, _ in twin.log] == [9, 12, 18] and twin.log[0][1].shape == (4, 8, 10)       # the hull of the box
    assert want["count"] == (3, 18) and want["captures"] == 3 and want["bins"].shape == (10, 2, 2, 6, 8)
    onset = np.where(want["onset"] == L.NONE, -1, want["onset"].astype(np.int64))
    assert onset.tolist() == PINNED_ONSET
    assert all(np.abs(want["bins"][a]).max() > 0 for a in range(10)) and want["pre"].any()
    twin.checkpoint()
    assert twin.run(4) == 4 and [s for s, _ in twin.log] == [9, 12, 18, 21]
    assert any(twin.expected()[k].tobytes() != want[k].tobytes() for k in L.KEYS)
    twin.rollback()
    again = twin.expected()
    assert twin.step_no == 18 and twin.next == 21 and again["count"] == (3, 18)
    assert all(again[k].tobytes() == want[k].tobytes() for k in L.KEYS)


if __name__ == "__main__":
    from oracle.oracle import Oracle
    oracle = Oracle()
    print("weights", FAMILY.weights)
    for name, value in counts([T.build_script(oracle, "all-plans", seed)["stats"] for seed in range(FAMILY.seeds)]).items():
        print("%-70s %s" % (name, value))

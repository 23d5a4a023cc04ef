"""The generator and the reference of tests/test_gpu_plan_sequences.py alone, on the CPU: the oracle, no engine.  The scripts of all four
families are the ones tests/golden/plan_sequence_digests.json pins, and what the comparison on the GPU needs before it means anything
-- every kind of plan fetched with something in it, captures inside cut runs, rollbacks across captures, writes between captures,
boxes with outside nodes, nodes with and without an onset -- is counted over all seeds and asserted here, for the families `plans`,
`modulation` and `arrival-bands` (tests/test_all_plans_twin.py has `all-plans`); the counts' bounds are the issues', and the
generator's probabilities (the families' weights) were chosen to meet them."""
import json
import os

import numpy as np
import pytest

import plan_twin as P
from helpers import GOLDEN
from wayverb_amd import mesh as M


@pytest.fixture(scope="module")
def scripts(oracle, built_library):
    return {family: [P.build_script(oracle, family, seed) for seed in range(P.FAMILIES[family].seeds)] for family in P.FAMILIES}


@pytest.fixture(scope="module")
def stats(scripts):
    return [s["stats"] for s in scripts["plans"]]


def test_the_generator_writes_the_pinned_scripts(scripts):
    """Every script of every family, byte for byte: the digests were recorded from the four generators this one replaced
    (profiles/r20/README.md).  A draw added, dropped or moved shows here."""
    with open(os.path.join(GOLDEN, "plan_sequence_digests.json")) as f:
        pinned = json.load(f)["digests"]
    assert {family: len(digests) for family, digests in pinned.items()} == {"plans": 40, "all-plans": 32, "modulation": 10, "arrival-bands": 8}
    for family, digests in pinned.items():
        assert [P.digest(s) for s in scripts[family]] == digests, family


def count(stats, what):
    n = sum(1 for s in stats if what(s))
    print(n)
    return n


def test_every_kind_of_plan_is_fetched_with_something_in_it(stats):
    for kind in P.KINDS6:
        assert count(stats, lambda s: kind in s["fetched"]) >= 5, kind


def test_few_sequences_end_with_fewer_than_two_captures(stats):
    assert count(stats, lambda s: s["captures"] < 2) <= 4


def test_captures_fall_inside_runs_of_six_steps_and_more(stats):
    assert count(stats, lambda s: s["cut_segment"]) >= 10


def test_rollbacks_cross_captures(stats):
    assert count(stats, lambda s: s["rolled_across"]) >= 8


def test_fields_and_memories_are_written_between_a_plans_captures(stats):
    assert count(stats, lambda s: s["write_between"]) >= 8


def test_boxes_in_rooms_that_leave_mesh_outside_hold_outside_nodes(stats):
    assert count(stats, lambda s: s["room"] != "box" and s["outside_in_box"]) >= 6


def test_arrival_plans_see_nodes_with_and_without_an_onset(stats):
    onsets = set().union(*[s["onsets"] for s in stats])
    print(sorted(onsets), sum(s["with_onset"] for s in stats), sum(s["without_onset"] for s in stats))
    assert sum(s["with_onset"] for s in stats) > 0 and sum(s["without_onset"] for s in stats) > 0 and len(onsets) >= 3


def test_sequences_stay_small(stats):
    assert max(s["steps"] for s in stats) <= 400


def test_the_pinned_example_of_generic_steps_in_between(oracle):
    """test_generic_steps_in_between_capture_nothing of every plan's file: a plan of period 3 set at step 9 captures 9 at the start of
    the next run and 12 in it, three generic steps pass 15, and the next run captures 18."""
    mesh = M.box_mesh(12, 10, 9)
    twin = P.PlanTwin(oracle, mesh, np.float32)
    twin.cur[mesh.compute_index(5, 5, 4)] = np.float32(1.0)
    assert twin.run(9) == 9
    twin.set_plan(dict(kind="snapshots", box=((0, 0, 0), (12, 10, 2)), stride=(1, 1, 1), first_step=0, period=3))
    assert twin.expected()["count"] == (0, 0)
    assert twin.run(4) == 4
    for _ in range(3):
        twin.outside_step()
    assert [s for s, _ in twin.log] == [9, 12]
    assert twin.run(2) == 2
    want = twin.expected()
    assert list(want["steps"]) == [9, 12, 18] and want["snapshots"].shape == (3, 2, 10, 12) and want["snapshots"][0].any()
    twin.checkpoint()
    assert twin.run(4) == 4 and [s for s, _ in twin.log] == [9, 12, 18, 21]
    twin.rollback()
    assert twin.step_no == 18 and twin.next == 21 and twin.expected()["snapshots"].tobytes() == want["snapshots"].tobytes()


def test_the_modulation_scripts_held_what_the_comparison_needs(scripts):
    """The four kinds of room, both precisions, captures in every script and more than one stage holds in half of them, sums that
    were not zeros in seven scripts of ten at the least, a plan replaced mid-sequence and a rollback across captures in three each at
    the least."""
    stats = [s["stats"] for s in scripts["modulation"]]
    assert len(stats) == 10
    assert {s["room"] for s in stats} == {"box", "L", "blob", "sphere"}
    assert {s["tag"] for s in scripts["modulation"]} == {"f32", "f64"}
    assert sum(1 for s in stats if s["fetched_something"]) >= 7
    assert sum(1 for s in stats if s["replaced"]) >= 3 and sum(1 for s in stats if s["rolled_across"]) >= 3
    assert all(s["captures"] > 0 for s in stats) and sum(1 for s in stats if s["captures"] > 16) >= 5


def test_the_arrival_bands_scripts_held_what_the_comparison_needs(scripts):
    """The four kinds of room, both precisions, captures in every script and more than one stage holds in three of them at the least,
    outputs with onsets and without, bins and pre in five scripts of eight at the least, a tail bin that took energy in two, a plan
    stopped or replaced mid-sequence in three and a rollback across captures in two at the least."""
    stats = [s["stats"] for s in scripts["arrival-bands"]]
    assert len(stats) == 8
    assert {s["room"] for s in stats} == {"box", "L", "blob", "sphere"}
    assert {s["tag"] for s in scripts["arrival-bands"]} == {"f32", "f64"}
    assert sum(1 for s in stats if s["fetched_something"]) >= 5 and sum(1 for s in stats if s["tails"]) >= 2
    assert sum(1 for s in stats if s["stopped"]) >= 2 and sum(1 for s in stats if s["replaced"] or s["stopped"]) >= 3 and sum(1 for s in stats if s["rolled_across"]) >= 2
    assert all(s["captures"] > 0 for s in stats) and sum(1 for s in stats if s["captures"] > 16) >= 3

"""The waterfall plan in the twin machinery of tests/plan_twin.py, on the CPU: the oracle, no engine.  One kind and one family join
plan_twin's tables for this module only (tests/waterfall_twin.py); the eight scripts are the ones
tests/golden/waterfall_sequence_digests.json pins, and what the replay on the GPU (tests/test_gpu_waterfall.py) needs before it means
anything is asserted here.  The bounds are the issue's; the seed of the generator was chosen to meet them, nothing else was."""
import json
import os

import numpy as np
import pytest

import plan_twin as P
import waterfall_twin as T
from helpers import GOLDEN
from wayverb_amd import waterfall as WF

PINNED = os.path.join(GOLDEN, "waterfall_sequence_digests.json")


@pytest.fixture(scope="module")
def scripts(oracle, built_library):
    committed = (sorted(P.KINDS), sorted(P.FAMILIES))
    with T.registered():
        assert sorted(set(P.KINDS) - set(committed[0])) == [T.KIND] and sorted(set(P.FAMILIES) - set(committed[1])) == [T.FAMILY]
        yield [P.build_script(oracle, T.FAMILY, seed) for seed in range(T.SEEDS)]
    assert (sorted(P.KINDS), sorted(P.FAMILIES)) == committed      # (other modules see the committed tables)


def test_the_family_has_one_kind_eight_seeds_and_the_weights_of_arrival_bands(scripts):
    family = P.FAMILIES[T.FAMILY]
    assert family.kinds == (T.KIND,) and family.seeds == 8 == len(scripts) and family.first(3) == T.KIND
    assert family.weights == P.FAMILIES["arrival-bands"].weights and family.calls == P.FAMILIES["arrival-bands"].calls
    assert family.rng_base not in [f.rng_base for name, f in P.FAMILIES.items() if name != T.FAMILY]
    assert P.KINDS[T.KIND].setter == "wv_set_waterfall" and "wv_set_waterfall(e, NULL, NULL)" in P.KINDS[T.KIND].active
    assert P.refusal_words(T.KIND, "spectrum") == "wv_set_spectrum: a waterfall plan is active (wv_set_waterfall(e, NULL, NULL) stops it); the plans exclude each other"


def test_the_generator_writes_the_pinned_scripts(scripts):
    with open(PINNED) as f:
        pinned = json.load(f)["digests"]
    assert len(pinned) == 8 == len(set(pinned))
    assert [P.digest(s) for s in scripts] == pinned


def test_the_scripts_hold_what_the_comparison_needs(scripts):
    """The four kinds of room and both precisions; captures in every script, more than the stage holds in three at the least; sums
    that were not zeros in five; a fold that crossed a bin edge in four; a capture in the open-ended last bin beyond its first
    bin_captures in two; a plan stopped or replaced in three; a rollback across captures in two."""
    stats, held = [s["stats"] for s in scripts], [T.held(s) for s in scripts]
    print([dict(h, **{k: s[k] for k in ("room", "captures", "replaced", "stopped", "rolled_across")}) for h, s in zip(held, stats)])
    assert {s["room"] for s in stats} == {"box", "L", "blob", "sphere"}
    assert {s["tag"] for s in scripts} == {"f32", "f64"}
    assert all(s["captures"] > 0 for s in stats)
    assert sum(1 for h in held if h["most"] > 16) >= 3
    assert sum(1 for s in stats if s["fetched_something"]) >= 5
    assert sum(1 for h in held if h["crossed"]) >= 4
    assert sum(1 for h in held if h["beyond"]) >= 2
    assert sum(1 for s in stats if s["replaced"] or s["stopped"]) >= 3
    assert sum(1 for s in stats if s["rolled_across"]) >= 2
    assert max(s["steps"] for s in stats) <= 400


def test_every_expected_output_is_the_definition_over_the_twins_captures(scripts):
    """A script's `want` at its end is waterfall_fold of the captures the twin logged: shape, dtype, and the bins no capture reached
    are +0.0."""
    for script in scripts:
        want, plan = script["final"]["want"], script["final"].get("plan")
        if want is None:
            continue
        bins = want["waterfall"]
        assert bins.dtype == np.complex128 and bins.ndim == 5 and want["captures"] == want["count"][0]
        last = [op["plan"] for op in script["ops"] if "plan" in op and op["op"] in ("plan", "same")][-1]
        assert bins.shape[:2] == (last["n_bins"], len(last["freqs"]))
        reached = min(-(-want["captures"] // last["bin_captures"]), last["n_bins"])
        untouched = np.stack([bins[reached:].real, bins[reached:].imag])
        assert not untouched.any() and not np.signbit(untouched).any()


def test_the_pinned_example_of_generic_steps_in_between(oracle, scripts):
    """A plan of period 3 set at step 9 captures 9 at the start of the next run and 12 in it, three generic steps pass 15, and the next
    run captures 18: the twin's account, which tests/test_gpu_waterfall.py holds the engine to.  (`scripts` keeps the kind registered.)"""
    from wayverb_amd import mesh as M
    mesh = M.box_mesh(12, 10, 9)
    twin = P.PlanTwin(oracle, mesh, np.float32)
    twin.cur[mesh.compute_index(5, 5, 4)] = np.float32(1.0)
    assert twin.run(9) == 9
    twin.set_plan(dict(kind=T.KIND, box=((0, 0, 0), (12, 10, 2)), stride=(1, 1, 1), first_step=0, period=3, freqs=[0.0, 0.25], n_bins=2, bin_captures=2))
    assert twin.expected()["count"] == (0, 0) and not twin.expected()["waterfall"].any()
    assert twin.run(4) == 4
    for _ in range(3):
        twin.outside_step()
    assert twin.run(2) == 2
    want = twin.expected()
    steps = [s for s, _ in twin.log]
    assert steps == [9, 12, 18] and want["count"] == (3, 18) and want["waterfall"].shape == (2, 2, 2, 10, 12)
    snaps = np.stack([a for _, a in twin.log])
    assert want["waterfall"].tobytes() == WF.waterfall_fold(snaps, steps, [0.0, 0.25], 2, 2).tobytes() and want["waterfall"][1].any()

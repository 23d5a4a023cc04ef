"""The interaural plan's place in the twin machinery of tests/plan_twin.py, from this file alone: one entry of KINDS, one family of
FAMILIES, and `registered()`, which puts both into plan_twin's tables for as long as a module's tests run and takes them out again --
other test modules of the same process see the committed tables.  tests/test_interaural_twin.py (CPU) and tests/test_gpu_interaural.py
use it; what the scripts must hold before the replay means anything is counted by `held`.

The twin needs the two ear planes rather than the box.  It gets them the way the lateral kind gets its neighbours: the entry says
`hull=True`, so a capture is the hull of the plan's box at stride 1 -- every taken node with the nodes one step from it along every
axis, the diagonal ones included -- and the generator draws ear offsets whose components are -1, 0 or 1, which all lie in that hull.
(Ears further out, up to +-8, are tests/test_gpu_interaural.py's own cases: plan_twin's hull is one node wide.)"""
import contextlib
from types import SimpleNamespace

import numpy as np

import plan_twin as P
from wayverb_amd import interaural as IA
from wayverb_amd.intensity import _shift

KIND = FAMILY = "interaural"
SEEDS = 8
STAGE = 16     # captures the stage holds (csrc/spectrum_plan.h)
LAGS = (0, 1, 3, 4, 5, 8, 11, 16)      # every lag class of the fold kernel, at and on either side of its chunks of four


def random_interaural_plan(rng, mesh, step_no, live):
    """A lateral plan's cadence (the hull inside the mesh), 1-4 edges 1-4 captures apart, two ears a node from the seat at the most (the
    same node for both in a quarter of the plans), a largest lag out of LAGS, a cascade of 1-2 sections in half the plans, a threshold."""
    plan = P.random_cadence(rng, mesh, step_no, live, KIND, hull=True)
    n_edges = int(rng.integers(1, 5))
    plan["edges"] = [0] + [int(e) for e in np.cumsum(rng.integers(1, 5, n_edges - 1))]
    plan["ear_a"] = tuple(int(v) for v in rng.integers(-1, 2, 3))
    plan["ear_b"] = plan["ear_a"] if rng.random() < 0.25 else tuple(int(v) for v in rng.integers(-1, 2, 3))
    plan["max_lag"] = int(rng.choice(LAGS))
    plan["sections"] = P.random_bands(rng)[0] if rng.random() < 0.5 else None
    return P.with_threshold(rng, plan)


def ear_planes(p, snaps):
    """The two ear planes float32[T, nz, ny, nx] out of the hull's snapshots."""
    sz, sy, sx = P.hull_of(p)[1]
    return [np.ascontiguousarray(snaps[:, _shift(sz, ear[2]), _shift(sy, ear[1]), _shift(sx, ear[0])]) for ear in (p["ear_a"], p["ear_b"])]


def expect_interaural(p, snaps, steps):
    a, b = ear_planes(p, snaps)
    out = IA.interaural_fold(a, b, P.threshold_of(p), p["edges"], p["max_lag"], p["sections"])
    return dict(captures=len(snaps), onset=out["onset"], pre=out["pre"], bins=out["bins"])


ENTRY = P.kind_entry(
    draw=random_interaural_plan, hull=True,
    expect=expect_interaural,
    something=lambda want, p: bool(np.any(want["bins"]) or np.any(want["pre"])),
    set=lambda eng, p, c: P.behind(eng.set_interaural(p["edges"], p["ear_a"], p["ear_b"], p["max_lag"], p["threshold"], p["sections"],
                                                      threshold_map=p["threshold_map"], **c), (len(p["edges"]), 2 * p["max_lag"] + 3)),
    stop=lambda eng: eng.set_interaural(None), count=lambda eng: eng.interaural_count(),
    fetch=lambda eng: P.fetch_keyed(eng.fetch_interaural, ("onset", "pre", "bins")),
    setter="wv_set_interaural", active="an interaural plan is active (wv_set_interaural(e, NULL, NULL, NULL) stops it)")

# `arrival-bands`' family in everything but the kind, the seed of the generator and the statistics a script reports (no tails here).
# rng_base: 23000, the first one tried; its eight scripts hold everything test_interaural_twin.py asserts
FAMILY_ENTRY = SimpleNamespace(**dict(vars(P.FAMILIES["arrival-bands"]), rng_base=23000, kinds=(KIND,), first=lambda seed: KIND,
                                      stats=P.COMMON_STATS + ("fetched_something", "replaced", "stopped")))


@contextlib.contextmanager
def registered():
    assert KIND not in P.KINDS and FAMILY not in P.FAMILIES
    P.KINDS[KIND], P.FAMILIES[FAMILY] = ENTRY, FAMILY_ENTRY
    try:
        yield
    finally:
        del P.KINDS[KIND], P.FAMILIES[FAMILY]


def held(script):
    """What one script holds, read off its calls: the most captures any plan of it showed; the lag classes (0, 4, 8, 16) and whether a
    cascade ran among the plans that showed a capture; whether some plan carried a history across a fold (more captures than the stage
    holds, with a lag); whether some plan with captures had both ears on one node."""
    most, classes, filtered, carried, equal = 0, set(), set(), False, False
    plan = None
    for op in [op for op in script["ops"]] + [dict(op="end", want=script["final"]["want"])]:
        want = op.get("want")
        if want is not None and plan is not None and want["count"][0]:
            count, L = want["count"][0], plan["max_lag"]
            most = max(most, count)
            classes.add(0 if L == 0 else 4 if L <= 4 else 8 if L <= 8 else 16)
            filtered.add(plan["sections"] is not None)
            carried = carried or (count > STAGE and L > 0)
            equal = equal or plan["ear_a"] == plan["ear_b"]
        if op["op"] in ("plan", "same"):
            plan = op["plan"]
        elif op["op"] == "stop":
            plan = None
    return dict(most=most, classes=sorted(classes), filtered=sorted(filtered), carried=carried, equal=equal)

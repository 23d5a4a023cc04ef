"""The waterfall plan's place in the twin machinery of tests/plan_twin.py, from this file alone: one entry of KINDS, one family of
FAMILIES, and `registered()`, which puts both into plan_twin's tables for as long as a module's tests run and takes them out again --
other test modules of the same process see the committed tables.  tests/test_waterfall_twin.py (CPU) and tests/test_gpu_waterfall.py
use it; what the scripts must hold before the replay means anything is counted by `held`."""
import contextlib
from types import SimpleNamespace

import numpy as np

import plan_twin as P
from wayverb_amd import waterfall as WF

KIND = FAMILY = "waterfall"
SEEDS = 8
STAGE = 16     # captures the stage holds (csrc/spectrum_plan.h)


def random_waterfall_plan(rng, mesh, step_no, live):
    """A spectrum plan's cadence and frequencies (K on either side of the fold's chunk of 4, both ends of the range among them) and a
    decay plan's bins: 1-6 of 1-5 captures."""
    plan = P.random_cadence(rng, mesh, step_no, live, KIND)
    k = int(rng.choice([1, 3, 4, 5, 9]))
    freqs = [float(f) for f in rng.uniform(0.0, 0.5, k)]
    if k >= 3:
        freqs[0], freqs[1] = 0.0, 0.5
    plan["freqs"] = freqs
    plan["n_bins"], plan["bin_captures"] = int(rng.integers(1, 7)), int(rng.integers(1, 6))
    return plan


ENTRY = P.kind_entry(
    draw=random_waterfall_plan,
    expect=lambda p, snaps, steps: dict(captures=len(snaps), waterfall=WF.waterfall_fold(snaps, steps, p["freqs"], p["n_bins"], p["bin_captures"])),
    something=lambda want, p: bool(np.any(want["waterfall"])),
    set=lambda eng, p, c: P.behind(eng.set_waterfall(p["freqs"], p["n_bins"], p["bin_captures"], **c), (p["n_bins"], len(p["freqs"]))),
    stop=lambda eng: eng.set_waterfall(None, None, None), count=lambda eng: eng.waterfall_count(),
    fetch=lambda eng: P.fetch_with_captures(eng.fetch_waterfall, "waterfall"),
    setter="wv_set_waterfall", active="a waterfall plan is active (wv_set_waterfall(e, NULL, NULL) stops it)")

# `arrival-bands`' family in everything but the kind, the seed of the generator and the statistics a script reports (no tails here).
# rng_base: the first of 22000, 22001, ... with which the eight scripts hold everything test_waterfall_twin.py asserts (found by trying
# them in order on the CPU; the nineteen before it miss one condition or another, most often a script without a capture)
FAMILY_ENTRY = SimpleNamespace(**dict(vars(P.FAMILIES["arrival-bands"]), rng_base=22019, kinds=(KIND,), first=lambda seed: KIND,
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
    """What one script holds, read off its calls: the most captures any plan of it showed; whether some fold crossed a bin edge; whether
    a capture went into the open-ended last bin beyond the bin's first bin_captures.

    The folds are counted only where the script itself says where they begin and end: between two points at which the plan's outputs
    are compared (a fetch, a stop, a handover, the end -- each folds whatever is staged) or between the plan's setting and the first
    of them, with nothing but runs, outside steps and writes in between (a checkpoint folds too, at a count the script does not say; a
    rollback moves the count).  From a fold at count c0 the stage fills from slot 0, so the folds up to the next point at c1 take the
    captures [c0, c0 + 16), [c0 + 16, c0 + 32), ..., [.., c1)."""
    most, crossed, beyond = 0, False, False
    plan, base = None, None      # the active plan; the count at the last known fold, None where it is not known
    points = [op for op in script["ops"]] + [dict(op="end", want=script["final"]["want"])]
    for op in points:
        name, want = op["op"], op.get("want")
        if want is not None and plan is not None:
            count = want["count"][0]
            most = max(most, count)
            beyond = beyond or count > plan["n_bins"] * plan["bin_captures"]
            if base is not None:
                for first in range(base, count, STAGE):
                    last = min(first + STAGE, count) - 1
                    crossed = crossed or min(first // plan["bin_captures"], plan["n_bins"] - 1) != min(last // plan["bin_captures"], plan["n_bins"] - 1)
            base = count
        if name in ("plan", "same"):
            plan, base = op["plan"], 0
        elif name == "stop":
            plan, base = None, None
        elif name in ("checkpoint", "rollback"):
            base = None
    return dict(most=most, crossed=crossed, beyond=beyond)

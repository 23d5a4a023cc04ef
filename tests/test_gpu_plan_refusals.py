"""What the capture plans' setters, counts, fetches and wv_rollback SAY when they refuse, code and full text, against
tests/golden/plan_refusals.json.  No stepping: a 12 x 10 x 9 box mesh in fp32, every plan a few hundred nodes.

The golden file was recorded from the commit BEFORE the five accumulating plans were given one life cycle
(`python tests/test_gpu_plan_refusals.py --record`, on a GPU), so it pins that the move changed no message -- but for REWORDED, the
four strings in which wv_set_snapshots and wv_set_spectrum took up the wording the five later setters already had.  The golden keeps
what the old code said; the table is applied to it here, and an entry of the table that does not find its old text fails."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_refusals.json")

pytestmark = pytest.mark.gpu

KINDS = ("snapshots", "spectrum", "decay", "decay_bands", "intensity", "arrival", "lateral")
STAGED = KINDS[1:]    # the kinds a checkpoint keeps a copy of
CONSTANTS = dict(spacing=0.05, sample_rate=8000.0, ambient_density=1.2)
BANDS = np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]], [[0.5, 0.25, 0.0, -0.1, 0.0]]])    # two cascades of one section

SET = {
    "snapshots": lambda e: e.set_snapshots(box=((1, 1, 1), (4, 3, 2))),
    "spectrum": lambda e: e.set_spectrum([0.0, 0.125], box=((1, 1, 1), (4, 3, 2))),
    "decay": lambda e: e.set_decay(3, box=((1, 1, 1), (4, 3, 2))),
    "decay_bands": lambda e: e.set_decay(3, box=((1, 1, 1), (4, 3, 2)), bands=BANDS),
    "intensity": lambda e: e.set_intensity(3, **CONSTANTS),
    "arrival": lambda e: e.set_arrival((0, 4), 1e-3, box=((1, 1, 1), (4, 3, 2))),
    "lateral": lambda e: e.set_lateral((0, 4), 1e-3, **CONSTANTS),
}
STOP = {
    "snapshots": lambda e: e.set_snapshots(None),
    "spectrum": lambda e: e.set_spectrum(None),
    "decay": lambda e: e.set_decay(None),
    "decay_bands": lambda e: e.set_decay(None),    # (wv_set_decay(e, NULL) stops either kind)
    "intensity": lambda e: e.set_intensity(None),
    "arrival": lambda e: e.set_arrival(None),
    "lateral": lambda e: e.set_lateral(None),
}
NO_PLAN = {
    "spectrum_count": lambda e: e.spectrum_count(),
    "fetch_spectrum": lambda e: e.fetch_spectrum(),
    "decay_count": lambda e: e.decay_count(),
    "fetch_decay": lambda e: e.fetch_decay(banded=False),
    "fetch_decay_bands": lambda e: e.fetch_decay(banded=True),
    "intensity_count": lambda e: e.intensity_count(),
    "fetch_intensity": lambda e: e.fetch_intensity(),
    "fetch_intensity_velocity": lambda e: e.fetch_intensity_velocity(),
    "arrival_count": lambda e: e.arrival_count(),
    "fetch_arrival": lambda e: e.fetch_arrival(),
    "lateral_count": lambda e: e.lateral_count(),
    "fetch_lateral": lambda e: e.fetch_lateral(),
}

TAIL = "; the plans exclude each other"
BANDED = "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)" + TAIL
# (active plan, setter called) -> (what the golden holds, what the engine says now)
REWORDED = {
    ("spectrum", "snapshots"): ("wv_set_snapshots: a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it); the two plans exclude each other",
                                "wv_set_snapshots: a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)" + TAIL),
    ("snapshots", "spectrum"): ("wv_set_spectrum: a snapshot plan is active (wv_set_snapshots(e, NULL) stops it); the two plans exclude each other",
                                "wv_set_spectrum: a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)" + TAIL),
    ("decay_bands", "snapshots"): ("wv_set_snapshots: a decay plan is active (wv_set_decay(e, NULL) stops it)" + TAIL, "wv_set_snapshots: " + BANDED),
    ("decay_bands", "spectrum"): ("wv_set_spectrum: a decay plan is active (wv_set_decay(e, NULL) stops it)" + TAIL, "wv_set_spectrum: " + BANDED),
}


def refusal(call, eng):
    """[code, text] of the error `call` raises; the call succeeding is a failure of the test."""
    from wayverb_amd import engine as E
    try:
        call(eng)
    except E.WaveguideError as err:
        m = re.fullmatch(r"wayverb_amd error (-?\d+): (.*)", str(err), flags=re.S)
        assert m, str(err)
        return [int(m.group(1)), m.group(2)]
    raise AssertionError("the call was not refused")


def engine():
    from wayverb_amd import engine as E
    from wayverb_amd import mesh as M
    return E.Engine(M.box_mesh(12, 10, 9), precision="f32")


def observe():
    """Everything the golden file holds, from the engine as built."""
    out = dict(refusals={}, rollback={}, no_plan={})
    eng = engine()
    try:
        out["no_plan"] = {name: refusal(call, eng) for name, call in NO_PLAN.items()}
        for active in KINDS:
            SET[active](eng)
            out["refusals"][active] = {setter: refusal(SET[setter], eng) for setter in KINDS if setter != active}
            STOP[active](eng)
            for setter in KINDS:    # with the plan stopped every setter that was refused goes through
                SET[setter](eng)
                STOP[setter](eng)
        for kind in STAGED:
            eng.checkpoint()
            SET[kind](eng)
            out["rollback"][kind] = refusal(lambda e: e.rollback(), eng)
            STOP[kind](eng)
            eng.rollback()    # without the plan there is nothing the checkpoint lacks
            eng.drop_checkpoint()
    finally:
        eng.close()
    return out


@pytest.fixture(scope="module")
def observed(built_library):
    return observe()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_every_setter_refuses_under_every_other_plan_in_the_recorded_words(observed, golden):
    want = {active: dict(row) for active, row in golden["refusals"].items()}
    for (active, setter), (old, new) in REWORDED.items():
        assert want[active][setter][1] == old, (active, setter)
        want[active][setter] = [want[active][setter][0], new]
    assert sorted(want) == sorted(KINDS) and all(sorted(want[a]) == sorted(k for k in KINDS if k != a) for a in KINDS)
    assert len({code for row in want.values() for code, _ in row.values()}) == 1    # WV_E_STATE throughout
    for active in KINDS:
        for setter in KINDS:
            if setter != active:
                assert observed["refusals"][active][setter] == want[active][setter], (active, setter)
    # both same-family cases are among them, each naming the other kind of decay plan
    assert "a banded decay plan is active" in want["decay_bands"]["decay"][1] and "a plain decay plan is active" in want["decay"]["decay_bands"][1]


def test_rollback_refuses_a_plan_set_behind_the_checkpoint_in_the_recorded_words(observed, golden):
    assert sorted(golden["rollback"]) == sorted(STAGED)
    assert observed["rollback"] == golden["rollback"]
    for kind, what in (("spectrum", "its sums"), ("decay", "its bins"), ("intensity", "its bins"), ("arrival", "its state"), ("lateral", "its state")):
        assert what in golden["rollback"][kind][1]


def test_counts_and_fetches_without_a_plan_say_so_in_the_recorded_words(observed, golden):
    assert sorted(golden["no_plan"]) == sorted(NO_PLAN)
    assert observed["no_plan"] == golden["no_plan"]
    assert all("plan is set" in text for _, text in golden["no_plan"].values())


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_plan_refusals.py --record    (on a GPU; rewrites tests/golden/plan_refusals.json)")
    with open(GOLDEN, "w") as f:
        json.dump(observe(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", GOLDEN)

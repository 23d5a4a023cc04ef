"""Capture plans -- snapshots, field spectra, decay maps (plain and band-limited), intensity maps, arrival maps -- through random rooms
and random sequences of API calls, against the oracle: tests/plan_twin.py draws the room (box, L, blob, sphere; rows of one wave and
of three) and the calls (runs of random lengths, steps driven from outside, values / fields / filter memories written between
them, the source moved, the receivers replaced, a plan set mid-sequence or replaced by one of another kind, outputs fetched mid-way,
checkpoints and rollbacks) and says, with no GPU in it, what the engine must show after each of them.  all_tiles is off, so rooms
that leave mesh outside are marched from their work lists; the stepping form is the engine's own choice or one of six forced ones.
After every call both fields, at every fetch and at the end every output of the active plan, and at the end the filter memories and
receiver rows must be the twin's BYTEWISE: the definitions are exact, no tolerance appears anywhere.

What this is after: a capture that reads a stale x-wall copy, a node of a unit that is never visited, a field whose role was swapped
by an odd batch, or a step whose source sample already rode in the launch before it."""
import numpy as np
import pytest

import plan_twin as P
from helpers import set_tuning
from wayverb_amd import arrival as A
from wayverb_amd import engine as E

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "passes": dict(pair=1), "three-step-passes": dict(pair=1, triple=1),
         "three-step-passes-all-units": dict(pair=1, triple=1, tile_lists=0), "single-steps": dict(pair=0),
         "two-launch-steps": dict(pair=0, whole_step=0), "graph-and-passes": dict(pair=1, graph=1)}

_script = {}     # the twin's script of the seed at hand: the modes of one seed follow each other, so one is held at a time
_tally = {mode: {} for mode in MODES}     # mode -> seed -> (passes, three-step passes, one-launch steps, share of the mesh marched)


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


def script_of(oracle, seed):
    if seed not in _script:
        _script.clear()
        _script[seed] = P.build_script(oracle, seed)
    return _script[seed]


def set_plan(eng, plan):
    common = dict(box=plan["box"], stride=plan["stride"], first_step=plan["first_step"], period=plan["period"])
    kind = plan["kind"]
    if kind == "snapshots":
        shape = eng.set_snapshots(**common)
    elif kind == "spectrum":
        shape = eng.set_spectrum(plan["freqs"], **common)[1:]
    elif kind == "decay":
        shape = eng.set_decay(plan["n_bins"], plan["bin_captures"], **common)[1:]
    elif kind == "banded":
        shape = eng.set_decay(plan["n_bins"], plan["bin_captures"], bands=plan["bands"], **common)[2:]
    elif kind == "intensity":
        shape = eng.set_intensity(plan["n_bins"], plan["bin_captures"], **common, **P.intensity_constants(plan))[2:]
    else:
        shape = eng.set_arrival(plan["edges"], plan["threshold"], threshold_map=plan["threshold_map"], **common)[1:]
    assert tuple(shape) == P.taken(plan)[::-1]


def stop_plan(eng, kind):
    """Through the plan's own setter."""
    {"snapshots": lambda: eng.set_snapshots(None), "spectrum": lambda: eng.set_spectrum(None), "decay": lambda: eng.set_decay(None),
     "banded": lambda: eng.set_decay(None), "intensity": lambda: eng.set_intensity(None), "arrival": lambda: eng.set_arrival(None)}[kind]()


def outputs(eng, kind):
    """Every output of the active plan, under the names of PlanTwin.expected."""
    if kind == "snapshots":
        count = eng.snapshot_count()
        snaps, steps = eng.fetch_snapshots()
        return dict(count=count, steps=steps, snapshots=snaps)
    if kind == "spectrum":
        count = eng.spectrum_count()
        sums, captures = eng.fetch_spectrum()
        return dict(count=count, captures=captures, spectrum=sums)
    if kind in ("decay", "banded"):
        count = eng.decay_count()
        bins, captures = eng.fetch_decay()
        return dict(count=count, captures=captures, bins=bins)
    if kind == "intensity":
        count = eng.intensity_count()
        bins, captures = eng.fetch_intensity()
        return dict(count=count, captures=captures, bins=bins, velocity=eng.fetch_intensity_velocity())
    count = eng.arrival_count()
    out, captures = eng.fetch_arrival()
    assert sorted(out) == sorted(A.KEYS)
    return dict(count=count, captures=captures, **out)


def assert_outputs(eng, kind, want, where):
    got = outputs(eng, kind)
    assert sorted(got) == sorted(want), where
    for name in sorted(want):
        if isinstance(want[name], np.ndarray):
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape, where)
            assert got[name].tobytes() == want[name].tobytes(), (name, where)
        else:
            assert got[name] == want[name], (name, got[name], want[name], where)


def replay(eng, script):
    """The script's calls on the engine, each followed by the comparison the script holds for it."""
    log = []
    kind = None
    for op in script["ops"]:
        name = op["op"]
        log.append(name if name != "plan" else "plan:%s" % op["plan"]["kind"])
        where = (script["room"], script["mesh"].dims, script["tag"], log)
        if name == "run":
            assert eng.run_steps(op["n"]) == (op["done"], 0), where
        elif name == "outside":
            for _ in range(op["n"]):
                assert eng.step() == 0
                eng.swap()
        elif name == "value":
            eng.write_value(op["node"], float(op["value"]), op["which"])
        elif name == "field":
            eng.write_field(op["field"], op["which"])
        elif name == "source":
            eng.set_source(op["kind"], op["node"], op["signal"])
        elif name == "receivers":
            eng.set_receivers(op["recv"])
        elif name == "memories":
            if op["data"] is not None:
                eng.write_boundary_data(op["d"], op["data"])
        elif name == "plan":
            if op["stop"] is not None:
                assert_outputs(eng, op["stop"], op["want"], where)
                stop_plan(eng, op["stop"])
            set_plan(eng, op["plan"])
            kind = op["plan"]["kind"]
        elif name == "fetch":
            assert_outputs(eng, kind, op["want"], where)
        elif name == "checkpoint":
            eng.checkpoint()
        else:
            eng.rollback()
        assert eng.read_field(E.BUF_CURRENT).tobytes() == op["cur"].tobytes(), where
        assert eng.read_field(E.BUF_PREVIOUS).tobytes() == op["prev"].tobytes(), where
    final = script["final"]
    where = (script["room"], script["mesh"].dims, script["tag"], log, "the end")
    assert eng.step_count() == final["step_no"], where
    assert_outputs(eng, kind, final["want"], where)
    for d in (1, 2, 3):
        assert eng.read_boundary_data(d)["filter_memory"].tobytes() == final["memories"][d - 1].tobytes(), where
    if final["recv"] and final["rows"]:
        got = eng.fetch_receivers(final["recv_from"], len(final["rows"]))
        want = np.array(final["rows"], dtype=np.float64).reshape(len(final["rows"]), len(final["recv"]))
        assert np.array_equal(got, want, equal_nan=True), where


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", range(P.SEEDS))
def test_random_plan_sequence(oracle, built_library, seed, mode):
    script = script_of(oracle, seed)
    set_tuning(**MODES[mode])
    eng = E.Engine(script["mesh"], precision=script["tag"], all_tiles=False)
    try:
        replay(eng, script)
        _tally[mode][seed] = (eng.query(E.Engine.QUERY_PASSES), eng.query(E.Engine.QUERY_TRIPLE_PASSES), eng.query(E.Engine.QUERY_WHOLE_STEPS),
                              eng.query(E.Engine.QUERY_MARCH_LIVE_PERMILLE))
    finally:
        eng.close()


def test_every_mode_met_its_form():
    """Over the seeds that ran in this process, and only if all of them did: each mode took the form it is named after, and the two
    modes with work lists marched less than the whole mesh, in a quarter of the seeds at the least."""
    if any(len(_tally[mode]) < P.SEEDS for mode in MODES):
        return
    met = {
        "passes: two-step passes": sum(1 for t in _tally["passes"].values() if t[0] > 0),
        "three-step-passes: three-step passes": sum(1 for t in _tally["three-step-passes"].values() if t[1] > 0),
        "default: one-launch steps": sum(1 for t in _tally["default"].values() if t[2] > 0),
        "single-steps: one-launch steps": sum(1 for t in _tally["single-steps"].values() if t[2] > 0),
        "passes: less than the whole mesh marched": sum(1 for t in _tally["passes"].values() if t[3] < 1000),
        "three-step-passes: less than the whole mesh marched": sum(1 for t in _tally["three-step-passes"].values() if t[3] < 1000),
    }
    print(met)
    for what, n in met.items():
        assert 4 * n >= P.SEEDS, (what, n)

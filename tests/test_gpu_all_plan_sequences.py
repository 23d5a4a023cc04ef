"""All eight kinds of capture plan -- snapshots, field spectra, decay maps (plain and band-limited), intensity, arrival, lateral and
modulation maps -- in ONE random sequence of API calls, against the oracle: tests/all_plans_twin.py draws the room and the calls of
tests/test_gpu_plan_sequences.py and, beside them, a plan replaced by one of its own kind with no stop in between, a setter of another
kind that must be refused in plan_refused's words, a rollback that must be refused, and a plan stopped with calls going on before the
next one is set.  After EVERY call both fields, at every fetch, every handover and the end every output of the active plan, and at
the end the step count, the filter memories and the receiver rows must be the twin's BYTEWISE: no tolerance appears anywhere.

What this is after: something one kind of plan leaves behind for the next through the life cycle they share
(csrc/engine_staged.hip.h) -- a stage, an event, a saved block, a `next`, a generation that makes a rollback refuse or fail to -- and
the per-lane state of the lateral fold (csrc/lateral_kernels.hip.h) under boxes, strides, periods, threshold maps, rollbacks in the
middle of a stage and gaps of outside steps that no fixed scenario of tests/test_gpu_lateral.py draws."""
import numpy as np
import pytest

import all_plans_twin as T
import plan_twin as P
import test_gpu_plan_sequences as S
from helpers import set_tuning
from wayverb_amd import engine as E
from wayverb_amd import lateral as L

pytestmark = pytest.mark.gpu

MODES = {name: S.MODES[name] for name in ("default", "three-step-passes", "single-steps", "graph-and-passes")}

_script = {}     # the twin's script of the seed at hand: the modes of one seed follow each other, so one is held at a time
_tally = {mode: {} for mode in MODES}     # mode -> seed -> (two-step passes, three-step passes, one-launch steps)


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


def script_of(oracle, seed):
    if seed not in _script:
        _script.clear()
        _script[seed] = T.build_script(oracle, seed)
    return _script[seed]


def set_plan(eng, plan):
    common = dict(box=plan["box"], stride=plan["stride"], first_step=plan["first_step"], period=plan["period"])
    if plan["kind"] == "lateral":
        shape = eng.set_lateral(plan["edges"], plan["threshold"], threshold_map=plan["threshold_map"], **common, **P.intensity_constants(plan))
        assert tuple(shape) == (10, len(plan["edges"])) + P.taken(plan)[::-1]
    elif plan["kind"] == "modulation":
        shape = eng.set_modulation(plan["freqs"], plan["bands"], **common)
        assert tuple(shape) == (plan["bands"].shape[0], len(plan["freqs"])) + P.taken(plan)[::-1]
    else:
        S.set_plan(eng, plan)


def stop_plan(eng, kind):
    """Through the plan's own setter; its count then says that no plan is set."""
    if kind == "lateral":
        eng.set_lateral(None)
    elif kind == "modulation":
        eng.set_modulation(None, None)
    else:
        S.stop_plan(eng, kind)
    count = {"snapshots": eng.snapshot_count, "spectrum": eng.spectrum_count, "decay": eng.decay_count, "banded": eng.decay_count,
             "intensity": eng.intensity_count, "arrival": eng.arrival_count, "lateral": eng.lateral_count, "modulation": eng.modulation_count}[kind]
    with pytest.raises(E.WaveguideError, match="error -6: .* plan is set"):
        count()


def outputs(eng, kind):
    """Every output of the active plan, under the names of AllPlansTwin.expected."""
    if kind == "lateral":
        count = eng.lateral_count()
        out, captures = eng.fetch_lateral()
        assert sorted(out) == sorted(L.KEYS)
        return dict(count=count, captures=captures, **out)
    if kind == "modulation":
        count = eng.modulation_count()
        energy, sums = eng.fetch_modulation()
        return dict(count=count, energy=energy, sums=sums)
    return S.outputs(eng, kind)


def assert_outputs(eng, kind, want, where):
    got = outputs(eng, kind)
    assert sorted(got) == sorted(want), where
    for name in sorted(want):
        if isinstance(want[name], np.ndarray):
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape, where)
            assert got[name].tobytes() == want[name].tobytes(), (name, where)
        else:
            assert got[name] == want[name], (name, got[name], want[name], where)


def assert_rollback_refused(eng, words=""):
    with pytest.raises(E.WaveguideError, match="error -6: wv_rollback: .*%s" % (words or " after the checkpoint")):
        eng.rollback()


def replay(eng, script):
    """The script's calls on the engine, each followed by the comparison the script holds for it."""
    log = []
    kind = None
    for op in script["ops"]:
        name = op["op"]
        log.append(name if name not in ("plan", "same", "refused-plan") else "%s:%s" % (name, op["plan"]["kind"]))
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
        elif name in ("plan", "same"):
            if op["stop"] is not None:
                assert kind == op["stop"], where
                assert_outputs(eng, op["stop"], op["want"], where)
                if name == "plan":         # (`same`: the setter replaces its own plan, no stop in between)
                    stop_plan(eng, op["stop"])
            set_plan(eng, op["plan"])
            kind = op["plan"]["kind"]
            if op["rollback_refused"]:
                assert_rollback_refused(eng)
        elif name == "fetch":
            assert kind == op["kind"], where
            assert_outputs(eng, kind, op["want"], where)
        elif name == "refused-plan":
            with pytest.raises(E.WaveguideError) as refusal:
                set_plan(eng, op["plan"])
            assert str(refusal.value).endswith("error -6: " + op["words"]), (str(refusal.value), where)
        elif name == "refused-rollback":
            assert_rollback_refused(eng, op["words"])
        elif name == "stop":
            assert kind == op["stop"], where
            assert_outputs(eng, kind, op["want"], where)
            stop_plan(eng, kind)
            kind = None
        elif name == "checkpoint":
            eng.checkpoint()
        else:
            eng.rollback()
        assert eng.read_field(E.BUF_CURRENT).tobytes() == op["cur"].tobytes(), where
        assert eng.read_field(E.BUF_PREVIOUS).tobytes() == op["prev"].tobytes(), where
    final = script["final"]
    where = (script["room"], script["mesh"].dims, script["tag"], log, "the end")
    assert eng.step_count() == final["step_no"], where
    assert kind == final["plan"]["kind"], where
    assert_outputs(eng, kind, final["want"], where)
    for d in (1, 2, 3):
        assert eng.read_boundary_data(d)["filter_memory"].tobytes() == final["memories"][d - 1].tobytes(), where
    if final["recv"] and final["rows"]:
        got = eng.fetch_receivers(final["recv_from"], len(final["rows"]))
        want = np.array(final["rows"], dtype=np.float64).reshape(len(final["rows"]), len(final["recv"]))
        assert got.dtype == want.dtype and got.shape == want.shape, where
        # (a row of an outside step is NaN in every column, and so is the twin's: the payload of a NaN is nobody's contract)
        gaps = np.isnan(want)
        assert np.array_equal(np.isnan(got), gaps) and np.where(gaps, 0.0, got).tobytes() == np.where(gaps, 0.0, want).tobytes(), where


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", range(T.SEEDS))
def test_random_sequence_of_all_plans(oracle, built_library, seed, mode):
    script = script_of(oracle, seed)
    set_tuning(**MODES[mode])
    eng = E.Engine(script["mesh"], precision=script["tag"], all_tiles=False)
    try:
        replay(eng, script)
        _tally[mode][seed] = (eng.query(E.Engine.QUERY_PASSES), eng.query(E.Engine.QUERY_TRIPLE_PASSES), eng.query(E.Engine.QUERY_WHOLE_STEPS))
    finally:
        eng.close()


def test_every_mode_met_its_form():
    """Over the seeds that ran in this process, and only if all of them did: each forced mode took the form it is named after in a
    quarter of the seeds at the least (a plan of period 1 or 2 leaves no room for a three-step pass, one of period 1 none for any).
    Of `graph-and-passes` only the passes can be seen: the engine has no query that counts replayed graphs (it replays one for an
    even batch of 16 steps or more on a mesh with clean outside nodes, engine_batch.hip.h), so that a graph was replayed is NOT shown."""
    if any(len(_tally[mode]) < T.SEEDS for mode in MODES):
        return
    met = {
        "three-step-passes: three-step passes": sum(1 for t in _tally["three-step-passes"].values() if t[1] > 0),
        "graph-and-passes: two-step passes": sum(1 for t in _tally["graph-and-passes"].values() if t[0] > 0),
        "single-steps: one-launch steps": sum(1 for t in _tally["single-steps"].values() if t[2] > 0),
        "single-steps: no pass": sum(1 for t in _tally["single-steps"].values() if t[0] == 0 and t[1] == 0),
        "default: one-launch steps": sum(1 for t in _tally["default"].values() if t[2] > 0),
    }
    print(met)
    for what, n in met.items():
        assert 4 * n >= T.SEEDS, (what, n)

"""Banded arrival plans through random rooms and random sequences of API calls, against the oracle: tests/plan_twin.py's PlanTwin with
the banded arrival plan's outputs on top (BandedArrivalTwin overrides `expected`; plan_twin.py itself is untouched), its rooms, boxes
and bands, and a generator in tests/test_gpu_modulation_sequences.py's style whose every plan is a banded arrival plan: runs of uneven
lengths, steps driven from outside, values / fields / filter memories written between them, the plan stopped or replaced by another
mid-sequence, outputs fetched mid-way, checkpoints and rollbacks.  After every call both fields, at every fetch and at the end the
plan's count and all six outputs must be the twin's BYTEWISE.  Eight seeds, the engine's own stepping form and two forced ones."""
import numpy as np
import pytest

import plan_twin as P
from helpers import set_tuning
from test_gpu_snapshots import subsample
from wayverb_amd import arrival as A
from wayverb_amd import engine as E
from wayverb_amd import mesh as M

pytestmark = pytest.mark.gpu

SEEDS = 8
MODES = {"default": {}, "three-step-passes": dict(pair=1, triple=1), "single-steps": dict(pair=0)}
# (chosen so that the counts the last test asserts hold with room to spare: the bounds are fixed, these are not)
WEIGHTS = dict(run=18, outside=1.5, value=1, field=2, memories=1, plan=2, stop=2, fetch=6, checkpoint=5, rollback=12)

_script = {}
_stats = {}


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


class BandedArrivalTwin(P.PlanTwin):
    def expected(self):
        p = self.plan
        if p["kind"] != "arrival_bands":
            return super().expected()
        n = len(self.log)
        shape = tuple(self.log[0][1].shape) if n else subsample(np.zeros(self.mesh.dims[::-1], np.float32), p, self.mesh.dims).shape
        snaps = np.stack([a for _, a in self.log]) if n else np.zeros((0,) + shape, np.float32)
        thr = p["threshold_map"] if p["threshold_map"] is not None else p["threshold"]
        out = A.banded_arrival_fold(snaps, thr, p["edges"], p["bands"], tail=p["tail"], lag=p["lag"])
        return dict(count=(n, int(self.log[-1][0]) if n else 0), **out)


def random_bands_plan(rng, mesh, step_no, live):
    """plan_twin.random_plan's arrival plan -- a box, strides, a cadence, 1-6 edges, a threshold and, in 4 plans of 10, a per-node map --
    with plan_twin.random_bands' 1-3 bands of 1-2 sections, a lag of 0-5 captures per band and, in 8 plans of 10, a tail of 1-6 bins of
    1-4 captures that begins 1-3 captures behind the last of then 3 edges at the most."""
    plan = P.random_plan(rng, mesh, step_no, live, "arrival")
    plan["kind"] = "arrival_bands"
    plan["bands"] = P.random_bands(rng)
    plan["lag"] = [int(v) for v in rng.integers(0, 6, plan["bands"].shape[0])]
    plan["tail"] = None
    if rng.random() < 0.8:
        plan["edges"] = plan["edges"][:3]      # (so that runs of a few dozen captures reach the tail)
        plan["tail"] = (int(rng.integers(1, 7)), plan["edges"][-1] + int(rng.integers(1, 4)), int(rng.integers(1, 5)))
    return plan


def build_script(oracle, seed):
    """plan_twin.build_script's scheme with one kind of plan: the room, the calls and what the engine must show after each of them."""
    rng = np.random.default_rng(19000 + seed)
    room, mesh = P.random_plan_room(rng, seed, oracle.classify)
    tag, dtype = P.precision_of(seed)
    t = mesh.nodes["boundary_type"]
    live = np.nonzero(t != 0)[0]
    inside = np.nonzero(t & M.ID_INSIDE)[0]
    twin = BandedArrivalTwin(oracle, mesh, dtype)
    stats = dict(room=room, fetched_something=False, captures=0, rolled_across=False, replaced=0, stopped=0, tails=0, steps=0)
    can_roll_back = False

    def fetched():
        want = twin.expected()
        heard = want["onset"] != A.NONE
        if heard.any() and (~heard).any() and np.any(want["bins"]) and np.any(want["pre"]):
            stats["fetched_something"] = True
        if want["bins"].shape[1] > len(twin.plan["edges"]) and np.any(want["bins"][:, len(twin.plan["edges"]):]):
            stats["tails"] += 1
        return want

    ops = []
    for i in range(int(rng.integers(14, 25))):
        names = [k for k in WEIGHTS if (k != "rollback" or can_roll_back) and (k not in ("fetch", "stop") or twin.plan is not None)]
        w = np.array([WEIGHTS[k] for k in names], dtype=np.float64)
        name = "source" if i == 0 else "plan" if i == 1 or twin.plan is None else str(rng.choice(names, p=w / w.sum()))   # (a stop is followed by a re-set)
        op = dict(op=name)
        if name == "run":
            op["n"] = int(rng.integers(1, 12)) if rng.random() < 0.7 else int(rng.integers(16, 40))
            op["done"] = twin.run(op["n"])
            stats["steps"] += op["done"]
        elif name == "outside":
            op["n"] = int(rng.integers(1, 4))
            for _ in range(op["n"]):
                twin.outside_step()
        elif name == "value":
            op["node"] = int(rng.choice(live))
            op["value"] = dtype(rng.uniform(-0.5, 0.5))
            op["which"] = E.BUF_CURRENT if rng.random() < 0.7 else E.BUF_PREVIOUS
            (twin.cur if op["which"] == E.BUF_CURRENT else twin.prev)[op["node"]] = op["value"]
        elif name == "field":
            op["field"] = np.where(t != 0, rng.uniform(-0.25, 0.25, mesh.num_nodes), 0.0).astype(dtype)
            op["which"] = E.BUF_CURRENT if rng.random() < 0.5 else E.BUF_PREVIOUS
            if op["which"] == E.BUF_CURRENT:
                twin.cur = op["field"].copy()
            else:
                twin.prev = op["field"].copy()
        elif name == "source":
            kind = int(rng.choice([E.SOURCE_HARD, E.SOURCE_SOFT]))
            op.update(kind=kind, node=int(rng.choice(inside)), signal=rng.uniform(-0.3, 0.3, int(rng.integers(250, 400))))
            twin.kind, twin.node, twin.signal, twin.pos = kind, op["node"], op["signal"], 0
        elif name == "memories":
            op["d"] = int(rng.integers(1, 4))
            op["data"] = None
            if len(twin.bd[op["d"] - 1]):
                twin.bd[op["d"] - 1]["filter_memory"] = rng.uniform(-1e-3, 1e-3, twin.bd[op["d"] - 1]["filter_memory"].shape)
                op["data"] = twin.bd[op["d"] - 1].copy()
        elif name == "plan":
            op["want"] = None
            if twin.plan is not None:      # (no plan leaves unseen: its outputs are compared before another takes its place)
                stats["captures"] += len(twin.log)
                stats["replaced"] += 1
                op["want"] = fetched()
            op["plan"] = random_bands_plan(rng, mesh, twin.step_no, live)
            twin.set_plan(op["plan"])
            can_roll_back = False          # (a plan set after the checkpoint: wv_rollback refuses, tests/test_gpu_arrival_bands.py pins that)
        elif name == "fetch":
            op["want"] = fetched()
        elif name == "stop":                # a NULL plan: compared, stopped, forgotten; runs go on without one until the next "plan"
            stats["captures"] += len(twin.log)
            stats["stopped"] += 1
            op["want"] = fetched()
            twin.set_plan(None)
            can_roll_back = False
        elif name == "checkpoint":
            twin.checkpoint()
            can_roll_back = True
        else:
            if len(twin.log) > len(twin.saved["log"]):
                stats["rolled_across"] = True
            twin.rollback()
        op["cur"], op["prev"] = twin.cur.copy(), twin.prev.copy()
        ops.append(op)
    stats["captures"] += len(twin.log)
    final = dict(want=fetched() if twin.plan is not None else None, step_no=twin.step_no, memories=[b["filter_memory"].copy() for b in twin.bd])
    return dict(room=room, mesh=mesh, tag=tag, dtype=dtype, ops=ops, final=final, stats=stats)


def script_of(oracle, seed):
    if seed not in _script:
        _script.clear()
        _script[seed] = build_script(oracle, seed)
        _stats[seed] = _script[seed]["stats"]
    return _script[seed]


def assert_outputs(eng, want, where):
    assert eng.arrival_bands_count() == want["count"], where
    got, captures = eng.fetch_arrival_bands()
    assert captures == want["count"][0], where
    for name in A.KEYS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape, where)
        assert got[name].tobytes() == want[name].tobytes(), (name, where)


def replay(eng, script):
    log = []
    for op in script["ops"]:
        name = op["op"]
        log.append(name)
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
        elif name == "memories":
            if op["data"] is not None:
                eng.write_boundary_data(op["d"], op["data"])
        elif name == "plan":
            if op["want"] is not None:
                assert_outputs(eng, op["want"], where)
            plan = op["plan"]
            shape = eng.set_arrival_bands(plan["edges"], plan["bands"], plan["threshold"], tail=plan["tail"], lag=plan["lag"], box=plan["box"],
                                          stride=plan["stride"], first_step=plan["first_step"], period=plan["period"], threshold_map=plan["threshold_map"])
            assert tuple(shape) == (plan["bands"].shape[0], len(plan["edges"]) + (plan["tail"][0] if plan["tail"] else 0)) + P.taken(plan)[::-1]
        elif name == "fetch":
            assert_outputs(eng, op["want"], where)
        elif name == "stop":
            assert_outputs(eng, op["want"], where)
            eng.set_arrival_bands(None, None)
        elif name == "checkpoint":
            eng.checkpoint()
        else:
            eng.rollback()
        assert eng.read_field(E.BUF_CURRENT).tobytes() == op["cur"].tobytes(), where
        assert eng.read_field(E.BUF_PREVIOUS).tobytes() == op["prev"].tobytes(), where
    final = script["final"]
    where = (script["room"], script["mesh"].dims, script["tag"], log, "the end")
    assert eng.step_count() == final["step_no"], where
    if final["want"] is not None:
        assert_outputs(eng, final["want"], where)
    for d in (1, 2, 3):
        assert eng.read_boundary_data(d)["filter_memory"].tobytes() == final["memories"][d - 1].tobytes(), where


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_banded_arrival_sequence(oracle, built_library, seed, mode):
    script = script_of(oracle, seed)
    set_tuning(**MODES[mode])
    eng = E.Engine(script["mesh"], precision=script["tag"], all_tiles=False)
    try:
        replay(eng, script)
    finally:
        eng.close()


def test_the_scripts_held_what_the_comparison_needs():
    """Over the seeds that ran in this process, and only if all of them did: the four kinds of room, both precisions, captures in every
    script and more than one stage holds in three of them at the least, outputs with onsets and without, bins and pre in five scripts of
    eight at the least, a tail bin that took energy in two, a plan stopped or replaced mid-sequence in three and a rollback across
    captures in two at the least."""
    if len(_stats) < SEEDS:
        return
    assert {s["room"] for s in _stats.values()} == {"box", "L", "blob", "sphere"}
    assert {P.precision_of(seed)[0] for seed in _stats} == {"f32", "f64"}
    assert sum(1 for s in _stats.values() if s["fetched_something"]) >= 5 and sum(1 for s in _stats.values() if s["tails"]) >= 2
    assert sum(1 for s in _stats.values() if s["stopped"]) >= 2 and sum(1 for s in _stats.values() if s["replaced"] or s["stopped"]) >= 3 and sum(1 for s in _stats.values() if s["rolled_across"]) >= 2
    assert all(s["captures"] > 0 for s in _stats.values()) and sum(1 for s in _stats.values() if s["captures"] > 16) >= 3

"""Modulation plans through random rooms and random sequences of API calls, against the oracle: tests/plan_twin.py's PlanTwin with the
modulation plan's outputs on top (ModulationTwin overrides `expected`; plan_twin.py itself is untouched), its rooms, boxes and bands,
and a generator in build_script's style whose every plan is a modulation plan: runs of random lengths, steps driven from outside,
values / fields / filter memories written between them, the plan replaced by another modulation plan mid-sequence, outputs fetched
mid-way, checkpoints and rollbacks.  After every call both fields, at every fetch and at the end the plan's count, energies and sums
must be the twin's BYTEWISE.  Ten seeds, the engine's own stepping form and two forced ones."""
import numpy as np
import pytest

import plan_twin as P
from helpers import set_tuning
from test_gpu_snapshots import subsample
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd import modulation as MOD

pytestmark = pytest.mark.gpu

SEEDS = 10
MODES = {"default": {}, "three-step-passes": dict(pair=1, triple=1), "single-steps": dict(pair=0)}
# (chosen so that the counts the last test asserts hold with room to spare: the bounds are fixed, these are not)
WEIGHTS = dict(run=18, outside=1.5, value=1, field=2, memories=1, plan=2, fetch=6, checkpoint=4, rollback=8)

_script = {}
_stats = {}


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


class ModulationTwin(P.PlanTwin):
    def expected(self):
        p = self.plan
        if p["kind"] != "modulation":
            return super().expected()
        n = len(self.log)
        steps = np.array([s for s, _ in self.log], dtype=np.uint64)
        shape = tuple(self.log[0][1].shape) if n else subsample(np.zeros(self.mesh.dims[::-1], np.float32), p, self.mesh.dims).shape
        snaps = np.stack([a for _, a in self.log]) if n else np.zeros((0,) + shape, np.float32)
        energy, sums = MOD.modulation_fold(snaps, steps, p["freqs"], p["bands"])
        return dict(count=(n, int(steps[-1]) if n else 0), energy=energy, sums=sums)


def random_modulation_plan(rng, mesh, step_no, live):
    origin, extent = P.random_box(rng, mesh.dims, live)
    m = int(rng.choice([1, 3, 4, 5, 14, 16]))
    freqs = [float(f) for f in rng.uniform(0.0, 0.5, m)]
    if m >= 3:
        freqs[0], freqs[1] = 0.0, 0.5
    return dict(kind="modulation", box=(origin, extent), stride=tuple(int(s) for s in rng.integers(1, 4, 3)), period=int(rng.integers(1, 8)),
                first_step=max(0, step_no - int(rng.integers(0, 6))), freqs=freqs, bands=P.random_bands(rng))


def build_script(oracle, seed):
    """plan_twin.build_script's scheme with one kind of plan: the room, the calls and what the engine must show after each of them."""
    rng = np.random.default_rng(16000 + seed)
    room, mesh = P.random_plan_room(rng, seed, oracle.classify)
    tag, dtype = P.precision_of(seed)
    t = mesh.nodes["boundary_type"]
    live = np.nonzero(t != 0)[0]
    inside = np.nonzero(t & M.ID_INSIDE)[0]
    twin = ModulationTwin(oracle, mesh, dtype)
    stats = dict(room=room, fetched_something=False, captures=0, rolled_across=False, replaced=0, steps=0)
    can_roll_back = False

    def fetched():
        want = twin.expected()
        if np.any(want["energy"]) and np.any(want["sums"]):
            stats["fetched_something"] = True
        return want

    ops = []
    for i in range(int(rng.integers(14, 25))):
        names = [k for k in WEIGHTS if k != "rollback" or can_roll_back]
        w = np.array([WEIGHTS[k] for k in names], dtype=np.float64)
        name = "source" if i == 0 else "plan" if i == 1 else str(rng.choice(names, p=w / w.sum()))
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
            op["plan"] = random_modulation_plan(rng, mesh, twin.step_no, live)
            twin.set_plan(op["plan"])
            can_roll_back = False          # (a plan set after the checkpoint: wv_rollback refuses, tests/test_gpu_modulation.py pins that)
        elif name == "fetch":
            op["want"] = fetched()
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
    final = dict(want=fetched(), step_no=twin.step_no, memories=[b["filter_memory"].copy() for b in twin.bd])
    return dict(room=room, mesh=mesh, tag=tag, dtype=dtype, ops=ops, final=final, stats=stats)


def script_of(oracle, seed):
    if seed not in _script:
        _script.clear()
        _script[seed] = build_script(oracle, seed)
        _stats[seed] = _script[seed]["stats"]
    return _script[seed]


def assert_outputs(eng, want, where):
    assert eng.modulation_count() == want["count"], where
    energy, sums = eng.fetch_modulation()
    for got, name in ((energy, "energy"), (sums, "sums")):
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, (name, got.shape, want[name].shape, where)
        assert got.tobytes() == want[name].tobytes(), (name, where)


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
            shape = eng.set_modulation(plan["freqs"], plan["bands"], box=plan["box"], stride=plan["stride"], first_step=plan["first_step"], period=plan["period"])
            assert tuple(shape) == (plan["bands"].shape[0], len(plan["freqs"])) + P.taken(plan)[::-1]
        elif name == "fetch":
            assert_outputs(eng, op["want"], where)
        elif name == "checkpoint":
            eng.checkpoint()
        else:
            eng.rollback()
        assert eng.read_field(E.BUF_CURRENT).tobytes() == op["cur"].tobytes(), where
        assert eng.read_field(E.BUF_PREVIOUS).tobytes() == op["prev"].tobytes(), where
    final = script["final"]
    where = (script["room"], script["mesh"].dims, script["tag"], log, "the end")
    assert eng.step_count() == final["step_no"], where
    assert_outputs(eng, final["want"], where)
    for d in (1, 2, 3):
        assert eng.read_boundary_data(d)["filter_memory"].tobytes() == final["memories"][d - 1].tobytes(), where


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_modulation_sequence(oracle, built_library, seed, mode):
    script = script_of(oracle, seed)
    set_tuning(**MODES[mode])
    eng = E.Engine(script["mesh"], precision=script["tag"], all_tiles=False)
    try:
        replay(eng, script)
    finally:
        eng.close()


def test_the_scripts_held_what_the_comparison_needs():
    """Over the seeds that ran in this process, and only if all of them did: the four kinds of room, both precisions, captures in every
    script and more than one stage holds in half of them, sums that were not zeros in seven scripts of ten at the least, a plan replaced
    mid-sequence and a rollback across captures in three each at the least."""
    if len(_stats) < SEEDS:
        return
    assert {s["room"] for s in _stats.values()} == {"box", "L", "blob", "sphere"}
    assert {P.precision_of(seed)[0] for seed in _stats} == {"f32", "f64"}
    assert sum(1 for s in _stats.values() if s["fetched_something"]) >= 7
    assert sum(1 for s in _stats.values() if s["replaced"]) >= 3 and sum(1 for s in _stats.values() if s["rolled_across"]) >= 3
    assert all(s["captures"] > 0 for s in _stats.values()) and sum(1 for s in _stats.values() if s["captures"] > 16) >= 5

"""The reference of tests/test_gpu_all_plan_sequences.py, with no GPU in it: tests/plan_twin.py's PlanTwin taught the two kinds of plan
that came after it (AllPlansTwin: lateral and modulation plans beside the six of plan_twin.KINDS, which go through PlanTwin
unchanged), and a generator in plan_twin.build_script's scheme that draws all eight kinds into one sequence and adds four calls the
older generator never makes: a plan replaced by one of its OWN kind with no stop in between, a setter of another kind that must be
refused, a rollback that must be refused, and a plan stopped with calls going on before the next one is set.  A script is the list
of calls with everything the engine must show after each of them; tests/test_all_plans_twin.py checks on the CPU that the scripts
hold what the comparison on the GPU needs before it means anything.  plan_twin.py itself is untouched: its seeds give what they gave.

What the header (include/wayverb_amd.h) and the engine's life cycle (csrc/engine_staged.hip.h, engine_io.hip.h) say of the new calls:
  - "setting a plan again replaces it": the new plan starts from nothing -- count 0, `next` from the step it is set at
  - while a plan is active every other kind's setter answers WV_E_STATE with plan_refused's sentence naming the active plan, and
    changes nothing
  - wv_rollback answers WV_E_STATE when the source or the receivers were set after the checkpoint, whatever was set and however many
    steps have run since ("must be the ones in place at the checkpoint"), and when the ACTIVE plan accumulates on the device (every
    kind but snapshots) and was set or replaced after it.  `refused-rollback` is drawn wherever one of the three holds.  A snapshot
    plan set after the checkpoint is rolled back (engine_snapshot.hip.h: snapshot_rollback), and so is a run whose plan was stopped
  - a setter given NULL stops its plan and forgets its state; with no plan active a rollback goes through"""
import numpy as np

import plan_twin as P
from test_gpu_modulation_sequences import random_modulation_plan
from test_gpu_snapshots import subsample
from wayverb_amd import engine as E
from wayverb_amd import intensity as I
from wayverb_amd import lateral as L
from wayverb_amd import mesh as M
from wayverb_amd import modulation as MOD

KINDS8 = P.KINDS + ("lateral", "modulation")
SEEDS = 32

TAIL = "; the plans exclude each other"
# the words of plan_refused's sentence (csrc/engine_staged.hip.h) that tell the active plan from every other
ACTIVE = {
    "snapshots": "a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)",
    "spectrum": "a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)",
    "decay": "a decay plan is active (wv_set_decay(e, NULL) stops it)",
    "banded": "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)",
    "intensity": "an intensity plan is active (wv_set_intensity(e, NULL) stops it)",
    "arrival": "an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it)",
    "lateral": "a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it)",
    "modulation": "a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it)",
}
SETTER = {"snapshots": "wv_set_snapshots", "spectrum": "wv_set_spectrum", "decay": "wv_set_decay", "banded": "wv_set_decay_bands",
          "intensity": "wv_set_intensity", "arrival": "wv_set_arrival", "lateral": "wv_set_lateral", "modulation": "wv_set_modulation"}


def refusal_words(active, setter):
    """What the setter of kind `setter` says under an active plan of kind `active`, behind "error -6: "."""
    if (active, setter) == ("decay", "banded"):      # (engine_decay.hip.h: the banded setter names the plain plan as such)
        return "wv_set_decay_bands: a plain decay plan is active (wv_set_decay(e, NULL) stops it)" + TAIL
    return SETTER[setter] + ": " + ACTIVE[active] + TAIL


def capture_box(plan):
    """plan_twin.capture_box, which knows the hull of an intensity plan only: a lateral plan captures its box's hull at stride 1 too."""
    if plan["kind"] != "lateral":
        return P.capture_box(plan)
    hull, _ = I.hull_box((plan["box"][0], P.taken(plan)), plan["stride"])
    return dict(box=hull, stride=(1, 1, 1))


class AllPlansTwin(P.PlanTwin):
    """PlanTwin with all eight kinds of plan."""

    def capture(self):
        if self.plan["kind"] != "lateral":
            return super().capture()
        nx, ny, nz = self.mesh.dims
        planes = self.cur.reshape(nz, ny, nx)
        self.log.append((self.step_no, np.ascontiguousarray(subsample(planes, capture_box(self.plan), self.mesh.dims)).astype(np.float32)))
        self.next = self.step_no + self.plan["period"]
        if self.on_capture:
            self.on_capture()

    def expected(self):
        p, n = self.plan, len(self.log)
        if p["kind"] not in ("lateral", "modulation"):
            return super().expected()
        steps = np.array([s for s, _ in self.log], dtype=np.uint64)
        last = int(steps[-1]) if n else 0
        shape = tuple(self.log[0][1].shape) if n else subsample(np.zeros(self.mesh.dims[::-1], np.float32), capture_box(p), self.mesh.dims).shape
        snaps = np.stack([a for _, a in self.log]) if n else np.zeros((0,) + shape, np.float32)
        if p["kind"] == "modulation":
            energy, sums = MOD.modulation_fold(snaps, steps, p["freqs"], p["bands"])
            return dict(count=(n, last), energy=energy, sums=sums)
        _, box_in_hull = I.hull_box((p["box"][0], P.taken(p)), p["stride"])
        c = P.intensity_constants(p)
        thr = p["threshold_map"] if p["threshold_map"] is not None else p["threshold"]
        out = L.lateral_fold(snaps, box_in_hull, thr, p["edges"], c["spacing"], c["sample_rate"], c["ambient_density"])
        return dict(count=(n, last), captures=n, **out)


def main_output(kind, want):
    return want["sums"] if kind == "modulation" else P.main_output(kind, want)


# ---- the generator ------------------------------------------------------------------------------------------------------------

def random_plan(rng, mesh, step_no, live, kind):
    """plan_twin.random_plan for its six kinds; a lateral plan's box, stride, period and first_step as it draws an intensity plan's
    (the hull inside the mesh), 1-8 edges, a threshold and, in 4 plans of 10, a per-node map as an arrival plan's; a modulation plan as
    tests/test_gpu_modulation_sequences.py draws it."""
    if kind == "modulation":
        return random_modulation_plan(rng, mesh, step_no, live)
    if kind != "lateral":
        return P.random_plan(rng, mesh, step_no, live, kind)
    drawn = P.random_plan(rng, mesh, step_no, live, "intensity")
    plan = dict(kind="lateral", box=drawn["box"], stride=drawn["stride"], period=drawn["period"], first_step=drawn["first_step"])
    n_edges = int(rng.integers(1, 9))
    widest = 3 if rng.random() < 0.5 else 5          # gaps of 1-2 captures in half the plans: more bins are reached in a short script
    plan["edges"] = [0] + [int(e) for e in np.cumsum(rng.integers(1, widest, n_edges - 1))]
    plan["threshold"] = float(np.float32(rng.uniform(0.02, 0.2)))
    plan["threshold_map"] = None
    if rng.random() < 0.4:
        plan["threshold_map"] = (plan["threshold"] * 10.0 ** rng.uniform(-1, 1, P.taken(plan)[::-1])).astype(np.float32)
    return plan


# The bounds tests/test_all_plans_twin.py asserts are fixed, these weights are not: they were chosen, by a search over a few dozen
# sets, so that every count holds with room to spare.  Against plan_twin.WEIGHTS: many more plans (eight kinds have 56 handovers, six
# have 30), more whole fields written (they bring the nodes of a lateral plan over their thresholds, and its state worth fuzzing lies
# behind the onset), and the four new calls.
WEIGHTS = dict(run=18, outside=1.5, value=1.5, field=5, source=0.5, receivers=0.5, memories=1.5, plan=9, fetch=8, checkpoint=6, rollback=14)
WEIGHTS.update({"same": 1, "refused-plan": 2, "refused-rollback": 3, "stop": 1})
NEED_A_PLAN = ("fetch", "same", "refused-plan", "stop")


def build_script(oracle, seed):
    """The room, the sequence of calls and what the engine must show after each of them, from the twin alone.  dict(room, mesh, tag,
    dtype, ops, final, stats); an op is a dict with its name under "op", its arguments, the two fields behind it ("cur", "prev") and,
    wherever a plan's outputs are compared, its kind under "stop" / "kind" and the expected outputs under "want"."""
    rng = np.random.default_rng(17000 + seed)
    room, mesh = P.random_plan_room(rng, seed, oracle.classify)
    tag, dtype = P.precision_of(seed)
    t = mesh.nodes["boundary_type"]
    live = np.nonzero(t != 0)[0]
    inside = np.nonzero(t & M.ID_INSIDE)[0]
    twin = AllPlansTwin(oracle, mesh, dtype)
    stats = dict(room=room, first=None, fetched=set(), pairs=set(), pairs_over_a_stop=set(), captures=0, most_under_one_plan=0, rolled_across=False,
                 same=0, refused_plans=0, refused_rollbacks=0, refused_for=set(), stop_run_plan=False, onsets=set(), with_onset=0, without_onset=0,
                 lateral_bins=0, steps=0)
    state = dict(checkpoint=False, plan_since=False, source_since=False, receivers_since=False, stopped=None, ran_since_stop=False)

    def on_capture():
        stats["most_under_one_plan"] = max(stats["most_under_one_plan"], len(twin.log))
    twin.on_capture = on_capture

    def can_roll_back():
        return state["checkpoint"] and not state["source_since"] and not state["receivers_since"] and not (twin.plan is not None and state["plan_since"])

    def rollback_is_refused():
        return state["checkpoint"] and (state["source_since"] or state["receivers_since"]
                                        or (twin.plan is not None and twin.plan["kind"] != "snapshots" and state["plan_since"]))

    def fetched():
        want = twin.expected()
        kind = twin.plan["kind"]
        if kind == "modulation":
            if np.any(want["energy"]) and np.any(want["sums"]):
                stats["fetched"].add(kind)
        elif np.any(main_output(kind, want)) or (kind in ("arrival", "lateral") and np.any(want["pre"])):
            stats["fetched"].add(kind)
        if kind == "lateral":
            stats["onsets"] |= set(int(v) for v in np.unique(want["onset"]) if v != L.NONE)
            stats["with_onset"] += int((want["onset"] != L.NONE).sum())
            stats["without_onset"] += int((want["onset"] == L.NONE).sum())
            energy = want["bins"][0]
            stats["lateral_bins"] = max(stats["lateral_bins"], int((energy.reshape(energy.shape[0], -1) != 0).any(axis=1).sum()))
        return want

    def leaves():
        """The active plan goes: its captures are counted, its outputs are what the engine must still show."""
        stats["captures"] += len(twin.log)
        return twin.plan["kind"], fetched()

    ops = []
    n_ops = int(rng.integers(20, 34))
    for i in range(n_ops):
        names = [k for k in WEIGHTS
                 if (k != "rollback" or can_roll_back()) and (k != "refused-rollback" or rollback_is_refused())
                 and (k not in NEED_A_PLAN or twin.plan is not None)
                 and (k != "plan" or not (ops and ops[-1]["op"] == "stop"))        # (a stop is followed by a call with no plan active)
                 and (k != "stop" or i < n_ops - 3)]
        w = np.array([WEIGHTS[k] for k in names], dtype=np.float64)
        name = "source" if i == 0 else "plan" if i == 1 or (i == n_ops - 1 and twin.plan is None) else str(rng.choice(names, p=w / w.sum()))
        op = dict(op=name)
        if name == "run":
            op["n"] = int(rng.integers(1, 12)) if rng.random() < 0.7 else int(rng.integers(16, 40))
            op["done"] = twin.run(op["n"])
            stats["steps"] += op["done"]
            if twin.plan is None and op["done"]:
                state["ran_since_stop"] = True
        elif name == "outside":
            op["n"] = int(rng.integers(1, 4))
            for _ in range(op["n"]):
                twin.outside_step()
        elif name == "value":
            op["node"] = int(rng.integers(0, mesh.num_nodes)) if rng.random() < 0.4 else int(rng.choice(live))
            op["value"] = dtype(rng.uniform(-0.5, 0.5))
            op["which"] = E.BUF_CURRENT if rng.random() < 0.7 else E.BUF_PREVIOUS
            (twin.cur if op["which"] == E.BUF_CURRENT else twin.prev)[op["node"]] = op["value"]
        elif name == "field":
            everywhere = rng.random() < 0.3                              # noise in the outside nodes too
            op["field"] = np.where((t != 0) | everywhere, rng.uniform(-0.25, 0.25, mesh.num_nodes), 0.0).astype(dtype)
            op["which"] = E.BUF_CURRENT if rng.random() < 0.5 else E.BUF_PREVIOUS
            if op["which"] == E.BUF_CURRENT:
                twin.cur = op["field"].copy()
            else:
                twin.prev = op["field"].copy()
        elif name == "source":
            kind = int(rng.choice([E.SOURCE_NONE, E.SOURCE_HARD, E.SOURCE_SOFT], p=[0.0, 0.45, 0.55] if i == 0 else [0.15, 0.4, 0.45]))
            node = int(rng.choice(inside)) if rng.random() < 0.7 else int(rng.choice(live))
            sig = rng.uniform(-0.3, 0.3, int(rng.integers(250, 401)))
            op.update(kind=kind, node=node, signal=sig)
            twin.kind, twin.node, twin.signal, twin.pos = kind, node, sig, 0
            state["source_since"] = True
        elif name == "receivers":
            op["recv"] = [int(rng.choice(inside)) if rng.random() < 0.6 else int(rng.integers(0, mesh.num_nodes))
                          for _ in range(int(rng.integers(0, 5)))]
            twin.recv, twin.rows, twin.recv_from = op["recv"], [], twin.step_no
            state["receivers_since"] = True
        elif name == "memories":
            op["d"] = int(rng.integers(1, 4))
            op["data"] = None
            if len(twin.bd[op["d"] - 1]):
                twin.bd[op["d"] - 1]["filter_memory"] = rng.uniform(-1e-3, 1e-3, twin.bd[op["d"] - 1]["filter_memory"].shape)
                op["data"] = twin.bd[op["d"] - 1].copy()
        elif name in ("plan", "same"):
            op["stop"], op["want"] = None, None
            if twin.plan is not None:      # (no plan leaves unseen: its outputs are compared before another takes its place)
                op["stop"], op["want"] = leaves()
            if name == "same":
                kind = twin.plan["kind"]
                stats["same"] += 1
            elif stats["first"] is None:
                # the first plan's kind goes round the eight with the seed: seed % 4 picks the room, so every kind meets every room,
                # and with precision_of every kind is first once in f32
                kind = stats["first"] = KINDS8[(seed // 4) % 8]
            else:
                kind = str(rng.choice([k for k in KINDS8 if twin.plan is None or k != twin.plan["kind"]]))
                if twin.plan is not None:
                    stats["pairs"].add((twin.plan["kind"], kind))
                elif state["stopped"] != kind:
                    stats["pairs_over_a_stop"].add((state["stopped"], kind))
                if twin.plan is None and state["ran_since_stop"]:
                    stats["stop_run_plan"] = True
            op["plan"] = random_plan(rng, mesh, twin.step_no, live, kind)
            twin.set_plan(op["plan"])
            state["plan_since"] = True
            op["rollback_refused"] = rollback_is_refused()     # (asserted on the spot: a refused rollback changes nothing)
        elif name == "fetch":
            op["kind"], op["want"] = twin.plan["kind"], fetched()
        elif name == "refused-plan":
            kind = str(rng.choice([k for k in KINDS8 if k != twin.plan["kind"]]))
            op["plan"] = random_plan(rng, mesh, twin.step_no, live, kind)
            op["words"] = refusal_words(twin.plan["kind"], kind)
            stats["refused_plans"] += 1
        elif name == "refused-rollback":
            # (engine_io.hip.h asks in this order, and says the first that holds)
            op["words"] = ("the receivers were changed after the checkpoint" if state["receivers_since"]
                           else "the source was changed after the checkpoint" if state["source_since"]
                           else "plan was set after the checkpoint")
            stats["refused_rollbacks"] += 1
            stats["refused_for"].add("receivers" if state["receivers_since"] else "source" if state["source_since"] else "plan")
        elif name == "stop":
            op["stop"], op["want"] = leaves()
            twin.set_plan(None)
            state["stopped"], state["ran_since_stop"] = op["stop"], False
        elif name == "checkpoint":
            twin.checkpoint()
            state.update(checkpoint=True, plan_since=False, source_since=False, receivers_since=False)
        else:
            if twin.plan is not None and len(twin.log) > len(twin.saved["log"]):
                stats["rolled_across"] = True
            twin.rollback()
        op["cur"], op["prev"] = twin.cur.copy(), twin.prev.copy()
        ops.append(op)
    stats["captures"] += len(twin.log)
    stats["cut_segment"] = twin.cut_segment
    final = dict(want=fetched(), step_no=twin.step_no, memories=[b["filter_memory"].copy() for b in twin.bd], recv=list(twin.recv),
                 rows=[list(r) for r in twin.rows], recv_from=twin.recv_from, plan=twin.plan)
    return dict(room=room, mesh=mesh, tag=tag, dtype=dtype, ops=ops, final=final, stats=stats)

"""The reference of tests/test_gpu_plan_sequences.py, with no GPU in it: the oracle `Twin` of tests/test_gpu_api_sequences.py with a
capture plan on top (PlanTwin), and the generator of random rooms and API sequences that drives it (build_script).  A script is the
list of calls with everything the engine must show after each of them; tests/test_plan_twin.py checks on the CPU that the scripts
hold what the comparison on the GPU needs before it means anything.

The capture rule is the one include/wayverb_amd.h documents ("field snapshots while a run keeps going") and engine_snapshot.hip.h
(snapshot_begin_run) / capture_stage.h (begin_run) implement, restated in plain Python:
  - at `set`, `next` is the first plan step at or after step_no
  - at the start of every run, if outside steps have passed `next`, it moves to the first plan step at or after step_no
  - if next == step_no the run captures before it steps; after every completed step with step_no == next it captures and advances
    `next` by the period
  - outside steps never capture; a run that stops because the signal ran out captures the steps it completed and no other
A capture is the twin's `current` as [nz, ny, nx], cut to the box and strides, as float32 (the hull of the box for an intensity
plan); the expected outputs are the definitions the project ships, folded over the captures in order."""
import copy

import numpy as np

from test_gpu_api_sequences import Twin
from test_gpu_decay import numpy_bins
from test_gpu_snapshots import subsample
from test_gpu_spectrum import numpy_fold
from test_receiver_arrays_host import canonical_parameters
from wayverb_amd import arrival as A
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import intensity as I
from wayverb_amd import mesh as M

KINDS = ("snapshots", "spectrum", "decay", "banded", "intensity", "arrival")
SEEDS = 40
SPACING, RATE, DENSITY = canonical_parameters()


def next_plan_step(plan, at):
    """The first step first_step + j * period that is >= at."""
    first, period = plan["first_step"], plan["period"]
    return first if at <= first else first + -(-(at - first) // period) * period


def taken(plan):
    """Nodes taken along (x, y, z)."""
    return tuple((e + s - 1) // s for e, s in zip(plan["box"][1], plan["stride"]))


def capture_box(plan):
    """What a capture cuts out of the field: the plan itself, or the hull of its box at stride 1 for an intensity plan."""
    if plan["kind"] != "intensity":
        return plan
    hull, _ = I.hull_box((plan["box"][0], taken(plan)), plan["stride"])
    return dict(box=hull, stride=(1, 1, 1))


def intensity_constants(plan):
    """The integrator sees a series sampled every `period` steps: that rate."""
    return dict(spacing=SPACING, sample_rate=RATE / plan["period"], ambient_density=DENSITY)


class PlanTwin(Twin):
    """The oracle kept in step with an engine, with the active capture plan and the log of its captures."""

    def __init__(self, oracle, mesh, dtype):
        super().__init__(oracle, mesh, dtype)
        self.plan, self.log, self.next = None, [], None
        self.saved = None
        self.cut_segment = False      # a capture strictly inside a run of six steps or more
        self.on_capture = None

    def set_plan(self, plan):
        self.plan, self.log = plan, []
        self.next = None if plan is None else next_plan_step(plan, self.step_no)

    def capture(self):
        nx, ny, nz = self.mesh.dims
        planes = self.cur.reshape(nz, ny, nx)
        self.log.append((self.step_no, np.ascontiguousarray(subsample(planes, capture_box(self.plan), self.mesh.dims)).astype(np.float32)))
        self.next = self.step_no + self.plan["period"]
        if self.on_capture:
            self.on_capture()

    def run(self, n):
        if self.plan is not None:
            if self.next < self.step_no:
                self.next = next_plan_step(self.plan, self.step_no)
            if self.next == self.step_no:
                self.capture()
        done, inside = 0, []
        for _ in range(n):
            if super().run(1) == 0:
                break
            done += 1
            if self.plan is not None and self.step_no == self.next:
                self.capture()
                inside.append(done)
        if done >= 6 and any(0 < i < done for i in inside):
            self.cut_segment = True
        return done

    STATE = ("prev", "cur", "bd", "kind", "node", "signal", "pos", "recv", "rows", "recv_from", "step_no", "log", "next")

    def checkpoint(self):
        self.saved = copy.deepcopy({k: getattr(self, k) for k in self.STATE})

    def rollback(self):
        for k, v in copy.deepcopy(self.saved).items():
            setattr(self, k, v)

    def expected(self):
        """Every output of the active plan, by the shipped definitions over the captures so far."""
        p, n = self.plan, len(self.log)
        steps = np.array([s for s, _ in self.log], dtype=np.uint64)
        last = int(steps[-1]) if n else 0
        shape = tuple(self.log[0][1].shape) if n else subsample(np.zeros(self.mesh.dims[::-1], np.float32), capture_box(p), self.mesh.dims).shape
        snaps = np.stack([a for _, a in self.log]) if n else np.zeros((0,) + shape, np.float32)
        if p["kind"] == "snapshots":
            return dict(count=(n, 0), steps=steps, snapshots=snaps)
        if p["kind"] == "spectrum":
            return dict(count=(n, last), captures=n, spectrum=numpy_fold(snaps, steps, p["freqs"]))
        if p["kind"] == "decay":
            return dict(count=(n, last), captures=n, bins=numpy_bins(snaps, p["n_bins"], p["bin_captures"]))
        if p["kind"] == "banded":
            return dict(count=(n, last), captures=n, bins=D.banded_bins(snaps, p["bands"], p["n_bins"], p["bin_captures"]))
        if p["kind"] == "intensity":
            _, box_in_hull = I.hull_box((p["box"][0], taken(p)), p["stride"])
            c = intensity_constants(p)
            bins, v = I.intensity_bins(snaps, box_in_hull, c["spacing"], c["sample_rate"], c["ambient_density"], p["n_bins"], p["bin_captures"],
                                       return_velocity=True) if n else (np.zeros((4, p["n_bins"]) + taken(p)[::-1]), np.zeros((3,) + taken(p)[::-1]))
            return dict(count=(n, last), captures=n, bins=bins, velocity=v)
        thr = p["threshold_map"] if p["threshold_map"] is not None else p["threshold"]
        out = A.arrival_fold(snaps, thr, p["edges"])
        return dict(count=(n, last), captures=n, **out)


def main_output(kind, want):
    return want[{"snapshots": "snapshots", "spectrum": "spectrum"}.get(kind, "bins")]


# ---- the generator ------------------------------------------------------------------------------------------------------------

def random_plan_room(rng, seed, classify):
    """The rooms of random_room in tests/test_gpu_api_sequences.py (box, L, blob; nx 9-35 or 126-149) and the sphere, one of the four
    per seed.  That function classifies its nodes on the device; here `classify` does (the oracle's restatement, which
    tests/test_mesh_setup.py holds equal to the device's node for node), so that the same room comes out with no GPU."""
    room = ["box", "L", "blob", "sphere"][seed % 4]
    nx = int(rng.choice([rng.integers(9, 36), rng.integers(126, 150)], p=[0.75, 0.25]))
    ny, nz = int(rng.integers(9, 26)), int(rng.integers(9, 26))
    if room != "box":
        nx, ny, nz = max(nx, 14), max(ny, 14), max(nz, 14)
    coeffs = np.concatenate([M.passive_peak_filter_coefficients(rng, 2),
                             np.array([M.flat_coefficients(0.3), M.rigid_coefficients()], dtype=M.coefficients_dtype)])
    surfaces = [int(s) for s in rng.integers(0, len(coeffs), 6)]
    if room == "box":
        return room, M.box_mesh(nx, ny, nz, coefficients=coeffs, surface_of_face=surfaces)
    nodes, counts = classify(M.room_mask((nz, ny, nx), room, seed=seed))
    return room, M.mesh_from_nodes((nx, ny, nz), nodes, counts, coeffs, surface_of_port=surfaces)


def precision_of(seed):
    """f32 for one seed in four, and for every kind of room in turn."""
    return ("f32", np.float32) if seed % 4 == (seed // 4) % 4 else ("f64", np.float64)


def random_box(rng, dims, live):
    nx, ny, nz = dims
    names = ["mesh", "z-plane", "sub-box", "far-corner", "one-node"] + (["across-lanes"] if nx > 130 else [])
    w = np.array([3, 3, 3, 1, 1, 3][:len(names)], dtype=np.float64)       # (the two smallest boxes seldom hold anything but zeros)
    name = str(rng.choice(names, p=w / w.sum()))
    if name == "mesh":
        return (0, 0, 0), (nx, ny, nz)
    if name == "z-plane":         # (the outermost planes are the dead shell of a box and outside in every other room: seldom those)
        return (0, 0, int(rng.integers(0, nz)) if rng.random() < 0.15 else int(rng.integers(2, nz - 2))), (nx, ny, 1)
    if name == "sub-box":         # rows that begin and end off every 16-byte boundary: an odd first node, an odd node behind the last
        x0 = 1 + 2 * int(rng.integers(0, (nx - 3) // 2))
        x1 = x0 + 2 * int(rng.integers(1, (nx - x0) // 2 + 1))
        y0, z0 = int(rng.integers(0, ny - 2)), int(rng.integers(0, nz - 2))
        return (x0, y0, z0), (x1 - x0, int(rng.integers(1, ny - y0 + 1)), int(rng.integers(1, nz - z0 + 1)))
    if name == "far-corner":      # the last two nodes of every axis
        return (nx - 2, ny - 2, nz - 2), (2, 2, 2)
    if name == "one-node":
        i = int(rng.choice(live))
        return (i % nx, i // nx % ny, i // (nx * ny)), (1, 1, 1)
    x0, x1 = int(rng.integers(40, 64)), int(rng.integers(130, nx + 1))       # across lane 64 and lane 128 of a row
    y0, z0 = int(rng.integers(0, ny - 3)), int(rng.integers(0, nz - 3))
    return (x0, y0, z0), (x1 - x0, int(rng.integers(2, ny - y0 + 1)), int(rng.integers(2, nz - z0 + 1)))


def random_bands(rng):
    """1-3 octave bands of 1-2 sections, designed at the rate of the captured series (1 per capture), the highest band's upper edge
    below its Nyquist frequency: S = 1 the reference's band-pass biquad, S = 2 the low-pass half of its Butterworth band-pass."""
    k_bands, n_sections = int(rng.integers(1, 4)), int(rng.integers(1, 3))
    top = float(rng.uniform(0.1, 0.3))
    edges = D.octave_band_edges([top / 2 ** k for k in range(k_bands)])
    if n_sections == 1:
        return np.stack([D.bandpass_biquad(lo, hi, 1.0) for lo, hi in edges])
    return np.stack([D.butterworth_bandpass(lo, hi, 1.0)[2:] for lo, hi in edges])


def random_plan(rng, mesh, step_no, live, kind):
    dims = mesh.dims
    origin, extent = random_box(rng, dims, live)
    stride = tuple(int(s) for s in rng.integers(1, 4, 3))
    if kind == "intensity":       # every taken node with its six neighbours on the grid: the hull inside the mesh
        lo = [min(max(o, 1), d - 2) for o, d in zip(origin, dims)]
        hi = [max(min(o + e, d - 1), l + 1) for o, e, d, l in zip(origin, extent, dims, lo)]
        origin, extent = tuple(lo), tuple(h - l for h, l in zip(hi, lo))
    plan = dict(kind=kind, box=(origin, extent), stride=stride, period=int(rng.integers(1, 8)),
                first_step=max(0, step_no - int(rng.integers(0, 6))))
    if kind == "spectrum":
        k = int(rng.integers(1, 7))
        freqs = [float(f) for f in rng.uniform(0.0, 0.5, k)]
        if k >= 3:
            freqs[0], freqs[1] = 0.0, 0.5
        plan["freqs"] = freqs
    elif kind in ("decay", "banded", "intensity"):
        plan["n_bins"], plan["bin_captures"] = int(rng.integers(1, 7)), int(rng.integers(1, 6))
        if kind == "banded":
            plan["bands"] = random_bands(rng)
    elif kind == "arrival":
        n_edges = int(rng.integers(1, 7))
        plan["edges"] = [0] + [int(e) for e in np.cumsum(rng.integers(1, 5, n_edges - 1))]
        plan["threshold"] = float(np.float32(rng.uniform(0.02, 0.2)))
        plan["threshold_map"] = None
        if rng.random() < 0.4:
            plan["threshold_map"] = (plan["threshold"] * 10.0 ** rng.uniform(-1, 1, taken(plan)[::-1])).astype(np.float32)
    return plan


# Chosen so that the counts tests/test_plan_twin.py asserts hold with room to spare (the bounds are fixed, these are not): a source or
# receivers call ends the chance of a rollback (wayverb_amd.h: they "must be the ones in place at the checkpoint"), so they are rare.
SHORT_SIGNAL = 0.15     # share of the signals that are 3-39 samples long, so that runs end because the signal ran out; the others 40-119
WEIGHTS = dict(run=15, outside=1.5, value=1.5, field=3, source=0.5, receivers=0.5, memories=1.5, plan=2.5, fetch=7, checkpoint=5, rollback=14)


def build_script(oracle, seed):
    """The room, the sequence of calls and what the engine must show after each of them, from the twin alone.  dict(room, mesh, tag,
    dtype, ops, final, stats); an op is a dict with its name under "op", its arguments, the two fields behind it ("cur", "prev") and,
    for a fetch, the plan's expected outputs under "want"."""
    rng = np.random.default_rng(7000 + seed)
    room, mesh = random_plan_room(rng, seed, oracle.classify)
    tag, dtype = precision_of(seed)
    t = mesh.nodes["boundary_type"]
    live = np.nonzero(t != 0)[0]
    inside = np.nonzero(t & M.ID_INSIDE)[0]
    outside_planes = (t == 0).reshape(mesh.dims[::-1])
    twin = PlanTwin(oracle, mesh, dtype)
    stats = dict(room=room, fetched=set(), captures=0, rolled_across=False, write_between=False, outside_in_box=False,
                 onsets=set(), with_onset=0, without_onset=0, steps=0)
    state = dict(can_roll_back=False, written=False, plan_has_outside=False)

    def on_capture():
        if state["written"]:
            stats["write_between"] = True
        if state["plan_has_outside"]:
            stats["outside_in_box"] = True
    twin.on_capture = on_capture

    def fetched():
        want = twin.expected()
        kind = twin.plan["kind"]
        if np.any(main_output(kind, want)) or (kind == "arrival" and np.any(want["pre"])):
            stats["fetched"].add(kind)
        if kind == "arrival":
            stats["onsets"] |= set(int(v) for v in np.unique(want["onset"]) if v != A.NONE)
            stats["with_onset"] += int((want["onset"] != A.NONE).sum())
            stats["without_onset"] += int((want["onset"] == A.NONE).sum())
        return want

    ops = []
    for i in range(int(rng.integers(10, 19))):
        names = [k for k in WEIGHTS if k != "rollback" or state["can_roll_back"]]
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
            # (the first call puts a signal in: a sequence without any would capture zeros throughout)
            kind = int(rng.choice([E.SOURCE_NONE, E.SOURCE_HARD, E.SOURCE_SOFT], p=[0.0, 0.45, 0.55] if i == 0 else [0.15, 0.4, 0.45]))
            node = int(rng.choice(inside)) if rng.random() < 0.7 else int(rng.choice(live))
            sig = rng.uniform(-0.3, 0.3, int(rng.integers(3, 40)) if rng.random() < SHORT_SIGNAL else int(rng.integers(40, 120)))
            op.update(kind=kind, node=node, signal=sig)
            twin.kind, twin.node, twin.signal, twin.pos = kind, node, sig, 0
            state["can_roll_back"] = False     # wayverb_amd.h: "The source and the receivers must be the ones in place at the checkpoint"
        elif name == "receivers":
            op["recv"] = [int(rng.choice(inside)) if rng.random() < 0.6 else int(rng.integers(0, mesh.num_nodes))
                          for _ in range(int(rng.integers(0, 5)))]
            twin.recv, twin.rows, twin.recv_from = op["recv"], [], twin.step_no
            state["can_roll_back"] = False
        elif name == "memories":
            op["d"] = int(rng.integers(1, 4))
            op["data"] = None
            if len(twin.bd[op["d"] - 1]):
                twin.bd[op["d"] - 1]["filter_memory"] = rng.uniform(-1e-3, 1e-3, twin.bd[op["d"] - 1]["filter_memory"].shape)
                op["data"] = twin.bd[op["d"] - 1].copy()
        elif name == "plan":
            op["stop"], op["want"] = None, None
            if twin.plan is not None:      # (no plan leaves unseen: its outputs are fetched and compared before it is stopped)
                stats["captures"] += len(twin.log)
                op["stop"], op["want"] = twin.plan["kind"], fetched()
            # the first plan's kind goes round the six with the seed, so that every kind meets every room and precision (seed % 4 picks
            # the room); every later one is random, of another kind than the one it replaces
            kind = KINDS[(seed + seed // 4) % 6] if twin.plan is None else str(rng.choice([k for k in KINDS if k != twin.plan["kind"]]))
            op["plan"] = random_plan(rng, mesh, twin.step_no, live, kind)
            twin.set_plan(op["plan"])
            state["can_roll_back"] = False     # (a plan set after the checkpoint: wv_rollback refuses, and the plans' own tests pin that)
            state["plan_has_outside"] = bool(subsample(outside_planes, capture_box(op["plan"]), mesh.dims).any())
        elif name == "fetch":
            op["want"] = fetched()
        elif name == "checkpoint":
            twin.checkpoint()
            state["can_roll_back"] = True
        else:
            if len(twin.log) > len(twin.saved["log"]):
                stats["rolled_across"] = True
            twin.rollback()
        if name in ("value", "field", "memories") and twin.plan is not None and twin.log:
            state["written"] = True
        if name == "plan":
            state["written"] = False
        op["cur"], op["prev"] = twin.cur.copy(), twin.prev.copy()
        ops.append(op)
    stats["captures"] += len(twin.log)
    stats["cut_segment"] = twin.cut_segment
    final = dict(want=fetched(), step_no=twin.step_no, memories=[b["filter_memory"].copy() for b in twin.bd], recv=list(twin.recv),
                 rows=[list(r) for r in twin.rows], recv_from=twin.recv_from, plan=twin.plan)
    return dict(room=room, mesh=mesh, tag=tag, dtype=dtype, ops=ops, final=final, stats=stats)

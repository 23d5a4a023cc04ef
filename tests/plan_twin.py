"""The reference of tests/test_gpu_plan_sequences.py, with no GPU in it: the oracle kept in step with an engine (Twin), the capture
plan on top of it (PlanTwin), the table of the nine kinds of plan (KINDS), the generator of random rooms and API sequences
(build_script), the replay of a script on an engine (replay) and the digest that pins a script (digest).  A script is the list of
calls with everything the engine must show after each of them; tests/test_plan_twin.py and tests/test_all_plans_twin.py check on the
CPU that the scripts hold what the comparison on the GPU needs before it means anything.

A new kind of plan is one entry of KINDS, plus a family of its own in FAMILIES or a place in the `kinds` of one.

The capture rule is the one include/wayverb_amd.h documents ("field snapshots while a run keeps going") and engine_snapshot.hip.h
(snapshot_begin_run) / capture_stage.h (begin_run) implement, restated in plain Python:
  - at `set`, `next` is the first plan step at or after step_no
  - at the start of every run, if outside steps have passed `next`, it moves to the first plan step at or after step_no
  - if next == step_no the run captures before it steps; after every completed step with step_no == next it captures and advances
    `next` by the period
  - outside steps never capture; a run that stops because the signal ran out captures the steps it completed and no other
A capture is the twin's `current` as [nz, ny, nx], cut to the box and strides, as float32 (the hull of the box for an intensity or
a lateral plan); the expected outputs are the definitions the project ships, folded over the captures in order.

What the header and the engine's life cycle (csrc/engine_staged.hip.h, engine_io.hip.h) say of the calls only `all-plans` draws:
  - "setting a plan again replaces it": the new plan starts from nothing -- count 0, `next` from the step it is set at
  - while a plan is active every other kind's setter answers WV_E_STATE with plan_refused's sentence naming the active plan, and
    changes nothing
  - wv_rollback answers WV_E_STATE when the source or the receivers were set after the checkpoint, whatever was set and however many
    steps have run since ("must be the ones in place at the checkpoint"), and when the ACTIVE plan accumulates on the device (every
    kind but snapshots) and was set or replaced after it.  `refused-rollback` is drawn wherever one of the three holds.  A snapshot
    plan set after the checkpoint is rolled back (engine_snapshot.hip.h: snapshot_rollback), and so is a run whose plan was stopped
  - a setter given NULL stops its plan and forgets its state; with no plan active a rollback goes through"""
import copy
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import canonical_parameters, numpy_bins, numpy_fold, subsample
from wayverb_amd import arrival as A
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import intensity as I
from wayverb_amd import lateral as L
from wayverb_amd import mesh as M
from wayverb_amd import modulation as MOD

SPACING, RATE, DENSITY = canonical_parameters()


class Twin:
    """The oracle kept in step with an engine."""

    def __init__(self, oracle, mesh, dtype):
        self.oracle, self.mesh, self.dtype = oracle, mesh, dtype
        self.prev = np.zeros(mesh.num_nodes, dtype=dtype)
        self.cur = np.zeros(mesh.num_nodes, dtype=dtype)
        self.bd = [mesh.boundary_data(d) for d in (1, 2, 3)]
        self.kind, self.node, self.signal, self.pos = E.SOURCE_NONE, 0, None, 0
        self.recv, self.rows, self.step_no, self.recv_from = [], [], 0, 0

    def plain_step(self):
        assert self.oracle.step(self.prev, self.cur, self.mesh, self.bd) == 0
        self.prev, self.cur = self.cur, self.prev
        self.step_no += 1

    def run(self, n):
        done = 0
        for _ in range(n):
            if self.kind != E.SOURCE_NONE:
                if self.pos >= len(self.signal):
                    break                                            # hard_source.h:18-20: `pre` returns false
                s = self.dtype(self.signal[self.pos])
                self.cur[self.node] = s if self.kind == E.SOURCE_HARD else self.dtype(self.cur[self.node] + s)
                self.pos += 1
            self.rows.append([float(self.cur[r]) for r in self.recv])
            self.plain_step()
            done += 1
        return done

    def outside_step(self):
        self.rows.append([float("nan")] * len(self.recv))
        self.plain_step()


def next_plan_step(plan, at):
    """The first step first_step + j * period that is >= at."""
    first, period = plan["first_step"], plan["period"]
    return first if at <= first else first + -(-(at - first) // period) * period


def taken(plan):
    """Nodes taken along (x, y, z)."""
    return tuple((e + s - 1) // s for e, s in zip(plan["box"][1], plan["stride"]))


def hull_of(plan):
    """(the hull of the plan's box: every taken node with its six neighbours; the box inside it)."""
    return I.hull_box((plan["box"][0], taken(plan)), plan["stride"])


def capture_box(plan):
    """What a capture cuts out of the field: the plan itself, or the hull of its box at stride 1."""
    return dict(box=hull_of(plan)[0], stride=(1, 1, 1)) if KINDS[plan["kind"]].hull else plan


def intensity_constants(plan):
    """The integrator sees a series sampled every `period` steps: that rate."""
    return dict(spacing=SPACING, sample_rate=RATE / plan["period"], ambient_density=DENSITY)


def threshold_of(plan):
    return plan["threshold_map"] if plan["threshold_map"] is not None else plan["threshold"]


# ---- how a random plan of each kind is drawn --------------------------------------------------------------------------------------

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


def random_cadence(rng, mesh, step_no, live, kind, hull=False):
    """A box, strides, a period and a first step at or a little before the step the plan is set at."""
    dims = mesh.dims
    origin, extent = random_box(rng, dims, live)
    stride = tuple(int(s) for s in rng.integers(1, 4, 3))
    if hull:       # every taken node with its six neighbours on the grid: the hull inside the mesh
        lo = [min(max(o, 1), d - 2) for o, d in zip(origin, dims)]
        hi = [max(min(o + e, d - 1), l + 1) for o, e, d, l in zip(origin, extent, dims, lo)]
        origin, extent = tuple(lo), tuple(h - l for h, l in zip(hi, lo))
    return dict(kind=kind, box=(origin, extent), stride=stride, period=int(rng.integers(1, 8)),
                first_step=max(0, step_no - int(rng.integers(0, 6))))


def random_spectrum_plan(rng, mesh, step_no, live):
    plan = random_cadence(rng, mesh, step_no, live, "spectrum")
    k = int(rng.integers(1, 7))
    freqs = [float(f) for f in rng.uniform(0.0, 0.5, k)]
    if k >= 3:
        freqs[0], freqs[1] = 0.0, 0.5
    plan["freqs"] = freqs
    return plan


def random_binned_plan(rng, mesh, step_no, live, kind, hull=False):
    plan = random_cadence(rng, mesh, step_no, live, kind, hull)
    plan["n_bins"], plan["bin_captures"] = int(rng.integers(1, 7)), int(rng.integers(1, 6))
    return plan


def random_banded_plan(rng, mesh, step_no, live):
    plan = random_binned_plan(rng, mesh, step_no, live, "banded")
    plan["bands"] = random_bands(rng)
    return plan


def with_threshold(rng, plan):
    """A threshold and, in 4 plans of 10, a per-node map a decade either side of it."""
    plan["threshold"] = float(np.float32(rng.uniform(0.02, 0.2)))
    plan["threshold_map"] = None
    if rng.random() < 0.4:
        plan["threshold_map"] = (plan["threshold"] * 10.0 ** rng.uniform(-1, 1, taken(plan)[::-1])).astype(np.float32)
    return plan


def random_arrival_plan(rng, mesh, step_no, live, kind="arrival"):
    plan = random_cadence(rng, mesh, step_no, live, kind)
    n_edges = int(rng.integers(1, 7))
    plan["edges"] = [0] + [int(e) for e in np.cumsum(rng.integers(1, 5, n_edges - 1))]
    return with_threshold(rng, plan)


def random_lateral_plan(rng, mesh, step_no, live):
    """An intensity plan's box (the hull inside the mesh) and 1-8 edges."""
    plan = random_cadence(rng, mesh, step_no, live, "lateral", hull=True)
    rng.integers(1, 7), rng.integers(1, 6)           # (the two draws of an intensity plan's bins: the scripts are pinned draw by draw)
    n_edges = int(rng.integers(1, 9))
    widest = 3 if rng.random() < 0.5 else 5          # gaps of 1-2 captures in half the plans: more bins are reached in a short script
    plan["edges"] = [0] + [int(e) for e in np.cumsum(rng.integers(1, widest, n_edges - 1))]
    return with_threshold(rng, plan)


def random_modulation_plan(rng, mesh, step_no, live):
    origin, extent = random_box(rng, mesh.dims, live)
    m = int(rng.choice([1, 3, 4, 5, 14, 16]))
    freqs = [float(f) for f in rng.uniform(0.0, 0.5, m)]
    if m >= 3:
        freqs[0], freqs[1] = 0.0, 0.5
    return dict(kind="modulation", box=(origin, extent), stride=tuple(int(s) for s in rng.integers(1, 4, 3)), period=int(rng.integers(1, 8)),
                first_step=max(0, step_no - int(rng.integers(0, 6))), freqs=freqs, bands=random_bands(rng))


def random_arrival_bands_plan(rng, mesh, step_no, live):
    """An arrival plan with random_bands' 1-3 bands of 1-2 sections, a lag of 0-5 captures per band and, in 8 plans of 10, a tail of
    1-6 bins of 1-4 captures that begins 1-3 captures behind the last of then 3 edges at the most."""
    plan = random_arrival_plan(rng, mesh, step_no, live, "arrival_bands")
    plan["bands"] = random_bands(rng)
    plan["lag"] = [int(v) for v in rng.integers(0, 6, plan["bands"].shape[0])]
    plan["tail"] = None
    if rng.random() < 0.8:
        plan["edges"] = plan["edges"][:3]      # (so that runs of a few dozen captures reach the tail)
        plan["tail"] = (int(rng.integers(1, 7)), plan["edges"][-1] + int(rng.integers(1, 4)), int(rng.integers(1, 5)))
    return plan


# ---- what a plan of each kind must show after its captures, by the shipped definitions -------------------------------------------------

def expect_intensity(p, snaps, steps):
    if not len(snaps):
        return dict(captures=0, bins=np.zeros((4, p["n_bins"]) + taken(p)[::-1]), velocity=np.zeros((3,) + taken(p)[::-1]))
    c = intensity_constants(p)
    bins, v = I.intensity_bins(snaps, hull_of(p)[1], c["spacing"], c["sample_rate"], c["ambient_density"], p["n_bins"], p["bin_captures"],
                               return_velocity=True)
    return dict(captures=len(snaps), bins=bins, velocity=v)


def expect_lateral(p, snaps, steps):
    c = intensity_constants(p)
    return dict(captures=len(snaps), **L.lateral_fold(snaps, hull_of(p)[1], threshold_of(p), p["edges"], c["spacing"], c["sample_rate"],
                                                      c["ambient_density"]))


def expect_modulation(p, snaps, steps):
    energy, sums = MOD.modulation_fold(snaps, steps, p["freqs"], p["bands"])
    return dict(energy=energy, sums=sums)


def heard_and_unheard(want, plan):
    heard = want["onset"] != A.NONE
    return bool(heard.any() and (~heard).any() and np.any(want["bins"]) and np.any(want["pre"]))


# ---- the Engine calls of each kind --------------------------------------------------------------------------------------------------

def behind(shape, lead):
    """The node axes of a setter's shape, behind leading axes that are `lead`."""
    assert tuple(shape[:len(lead)]) == tuple(lead), (shape, lead)
    return shape[len(lead):]


def fetch_snapshots(eng):
    snaps, steps = eng.fetch_snapshots()
    return dict(steps=steps, snapshots=snaps)


def fetch_with_captures(fetch, name):
    main, captures = fetch()
    return {"captures": captures, name: main}


def fetch_keyed(fetch, keys):
    out, captures = fetch()
    assert sorted(out) == sorted(keys)
    return dict(captures=captures, **out)


def fetch_modulation(eng):
    energy, sums = eng.fetch_modulation()
    return dict(energy=energy, sums=sums)


def fetch_arrival_bands(eng):
    out, captures = eng.fetch_arrival_bands()
    assert sorted(out) == sorted(A.KEYS) and captures == eng.arrival_bands_count()[0]
    return out


# ---- the nine kinds ----------------------------------------------------------------------------------------------------------------
# draw(rng, mesh, step_no, live): a random plan.  hull: a capture cuts the hull of the box at stride 1, not the box.
# expect(plan, snaps, steps): the outputs over the captures float32[n, ...] taken at `steps`, by the shipped definition; the twin adds
# count = (n, the last capture's step).  something(want, plan): "fetched with something in it".  set(eng, plan, common): the setter,
# which returns the node axes of the shape it answers; stop / count / fetch(eng): the plan stopped through its own setter, its count,
# every output under expect's names.  setter: the C setter's name; active: plan_refused's words (csrc/engine_staged.hip.h) that tell
# this kind's active plan from every other.

def kind_entry(**fields):
    return SimpleNamespace(**dict(dict(hull=False), **fields))


KINDS = {
    "snapshots": kind_entry(
        draw=lambda rng, mesh, step_no, live: random_cadence(rng, mesh, step_no, live, "snapshots"),
        expect=lambda p, snaps, steps: dict(count=(len(snaps), 0), steps=steps, snapshots=snaps),      # (its count's second word: the oldest held)
        something=lambda want, p: bool(np.any(want["snapshots"])),
        set=lambda eng, p, c: eng.set_snapshots(**c), stop=lambda eng: eng.set_snapshots(None),
        count=lambda eng: eng.snapshot_count(), fetch=fetch_snapshots,
        setter="wv_set_snapshots", active="a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)"),
    "spectrum": kind_entry(
        draw=random_spectrum_plan,
        expect=lambda p, snaps, steps: dict(captures=len(snaps), spectrum=numpy_fold(snaps, steps, p["freqs"])),
        something=lambda want, p: bool(np.any(want["spectrum"])),
        set=lambda eng, p, c: eng.set_spectrum(p["freqs"], **c)[1:], stop=lambda eng: eng.set_spectrum(None),
        count=lambda eng: eng.spectrum_count(), fetch=lambda eng: fetch_with_captures(eng.fetch_spectrum, "spectrum"),
        setter="wv_set_spectrum", active="a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)"),
    "decay": kind_entry(
        draw=lambda rng, mesh, step_no, live: random_binned_plan(rng, mesh, step_no, live, "decay"),
        expect=lambda p, snaps, steps: dict(captures=len(snaps), bins=numpy_bins(snaps, p["n_bins"], p["bin_captures"])),
        something=lambda want, p: bool(np.any(want["bins"])),
        set=lambda eng, p, c: eng.set_decay(p["n_bins"], p["bin_captures"], **c)[1:], stop=lambda eng: eng.set_decay(None),
        count=lambda eng: eng.decay_count(), fetch=lambda eng: fetch_with_captures(eng.fetch_decay, "bins"),
        setter="wv_set_decay", active="a decay plan is active (wv_set_decay(e, NULL) stops it)"),
    "banded": kind_entry(
        draw=random_banded_plan,
        expect=lambda p, snaps, steps: dict(captures=len(snaps), bins=D.banded_bins(snaps, p["bands"], p["n_bins"], p["bin_captures"])),
        something=lambda want, p: bool(np.any(want["bins"])),
        set=lambda eng, p, c: eng.set_decay(p["n_bins"], p["bin_captures"], bands=p["bands"], **c)[2:], stop=lambda eng: eng.set_decay(None),
        count=lambda eng: eng.decay_count(), fetch=lambda eng: fetch_with_captures(eng.fetch_decay, "bins"),
        setter="wv_set_decay_bands", active="a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)"),
    "intensity": kind_entry(
        draw=lambda rng, mesh, step_no, live: random_binned_plan(rng, mesh, step_no, live, "intensity", hull=True), hull=True,
        expect=expect_intensity,
        something=lambda want, p: bool(np.any(want["bins"])),
        set=lambda eng, p, c: eng.set_intensity(p["n_bins"], p["bin_captures"], **c, **intensity_constants(p))[2:],
        stop=lambda eng: eng.set_intensity(None), count=lambda eng: eng.intensity_count(),
        fetch=lambda eng: dict(fetch_with_captures(eng.fetch_intensity, "bins"), velocity=eng.fetch_intensity_velocity()),
        setter="wv_set_intensity", active="an intensity plan is active (wv_set_intensity(e, NULL) stops it)"),
    "arrival": kind_entry(
        draw=random_arrival_plan,
        expect=lambda p, snaps, steps: dict(captures=len(snaps), **A.arrival_fold(snaps, threshold_of(p), p["edges"])),
        something=lambda want, p: bool(np.any(want["bins"]) or np.any(want["pre"])),
        set=lambda eng, p, c: eng.set_arrival(p["edges"], p["threshold"], threshold_map=p["threshold_map"], **c)[1:],
        stop=lambda eng: eng.set_arrival(None), count=lambda eng: eng.arrival_count(),
        fetch=lambda eng: fetch_keyed(eng.fetch_arrival, A.KEYS),
        setter="wv_set_arrival", active="an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it)"),
    "lateral": kind_entry(
        draw=random_lateral_plan, hull=True,
        expect=expect_lateral,
        something=lambda want, p: bool(np.any(want["bins"]) or np.any(want["pre"])),
        set=lambda eng, p, c: behind(eng.set_lateral(p["edges"], p["threshold"], threshold_map=p["threshold_map"], **c, **intensity_constants(p)),
                                     (10, len(p["edges"]))),
        stop=lambda eng: eng.set_lateral(None), count=lambda eng: eng.lateral_count(),
        fetch=lambda eng: fetch_keyed(eng.fetch_lateral, L.KEYS),
        setter="wv_set_lateral", active="a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it)"),
    "modulation": kind_entry(
        draw=random_modulation_plan,
        expect=expect_modulation,
        something=lambda want, p: bool(np.any(want["energy"]) and np.any(want["sums"])),
        set=lambda eng, p, c: behind(eng.set_modulation(p["freqs"], p["bands"], **c), (p["bands"].shape[0], len(p["freqs"]))),
        stop=lambda eng: eng.set_modulation(None, None), count=lambda eng: eng.modulation_count(), fetch=fetch_modulation,
        setter="wv_set_modulation", active="a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it)"),
    "arrival_bands": kind_entry(
        draw=random_arrival_bands_plan,
        expect=lambda p, snaps, steps: A.banded_arrival_fold(snaps, threshold_of(p), p["edges"], p["bands"], tail=p["tail"], lag=p["lag"]),
        something=heard_and_unheard,
        set=lambda eng, p, c: behind(eng.set_arrival_bands(p["edges"], p["bands"], p["threshold"], tail=p["tail"], lag=p["lag"],
                                                           threshold_map=p["threshold_map"], **c),
                                     (p["bands"].shape[0], len(p["edges"]) + (p["tail"][0] if p["tail"] else 0))),
        stop=lambda eng: eng.set_arrival_bands(None, None), count=lambda eng: eng.arrival_bands_count(), fetch=fetch_arrival_bands,
        setter="wv_set_arrival_bands", active="a banded arrival plan is active (wv_set_arrival_bands(e, NULL, NULL, NULL, 0, 0) stops it)"),
}
KINDS6 = ("snapshots", "spectrum", "decay", "banded", "intensity", "arrival")
KINDS8 = KINDS6 + ("lateral", "modulation")
TAIL = "; the plans exclude each other"


def refusal_words(active, setter):
    """What the setter of kind `setter` says under an active plan of kind `active`, behind "error -6: "."""
    if (active, setter) == ("decay", "banded"):      # (engine_decay.hip.h: the banded setter names the plain plan as such)
        return "wv_set_decay_bands: a plain decay plan is active (wv_set_decay(e, NULL) stops it)" + TAIL
    return KINDS[setter].setter + ": " + KINDS[active].active + TAIL


def set_plan(eng, plan):
    common = dict(box=plan["box"], stride=plan["stride"], first_step=plan["first_step"], period=plan["period"])
    assert tuple(KINDS[plan["kind"]].set(eng, plan, common)) == taken(plan)[::-1]


def stop_plan(eng, kind):
    """Through the plan's own setter; its count then says that no plan is set."""
    KINDS[kind].stop(eng)
    with pytest.raises(E.WaveguideError, match="error -6: .* plan is set"):
        KINDS[kind].count(eng)


def assert_same(got, want, where=None):
    """Two sets of outputs under the same names: dtype, shape, then bytes."""
    assert sorted(got) == sorted(want), where
    for name in sorted(want):
        if isinstance(want[name], np.ndarray):
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape, where)
            assert got[name].tobytes() == want[name].tobytes(), (name, where)
        else:
            assert got[name] == want[name], (name, got[name], want[name], where)


def assert_outputs(eng, kind, want, where):
    """Every output of the active plan, under the names of PlanTwin.expected: dtype, shape, then bytes."""
    assert_same(dict(count=KINDS[kind].count(eng), **KINDS[kind].fetch(eng)), want, where)


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
        shape = tuple(self.log[0][1].shape) if n else subsample(np.zeros(self.mesh.dims[::-1], np.float32), capture_box(p), self.mesh.dims).shape
        snaps = np.stack([a for _, a in self.log]) if n else np.zeros((0,) + shape, np.float32)
        return {"count": (n, int(steps[-1]) if n else 0), **KINDS[p["kind"]].expect(p, snaps, steps)}


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


# The four families of scripts.  What differs between them, and nothing else:
#   seeds, rng_base, calls: how many scripts, the seed of script 0's generator, the range the number of calls is drawn from
#   kinds, first: the kinds of plan drawn, and the first plan's kind by the seed.  A family of one kind never draws a kind, writes no
#       kind's name into its calls, has no receivers at the end, and sets a plan wherever it has none after a stop
#   value_anywhere: a written value lands on any node of the mesh with probability 0.4, otherwise on a live one
#   noise_everywhere: a written field has noise in the outside nodes too with probability 0.3
#   source_anywhere: NONE / HARD / SOFT with the probabilities below (the first call: never NONE) at an inside node with probability
#       0.7, otherwise a live one; if not, HARD or SOFT at an inside node
#   signal_length(rng): how long a source's signal is
#   late_stops: the last calls that are never a `stop`
#   onsets_of: the kind whose fetches the onset statistics are taken from
#   weights: the calls and how often each is drawn (`receivers`, `same`, `refused-plan`, `refused-rollback` and `stop` are drawn only
#       where they have a weight).  The weights were chosen, the bounds the CPU tests assert were not: a source or receivers call ends
#       the chance of a rollback (wayverb_amd.h: they "must be the ones in place at the checkpoint"), so they are rare; `all-plans` has
#       many more plans (eight kinds have 56 handovers, six have 30) and more whole fields (they bring the nodes of a lateral plan over
#       their thresholds, and its state worth fuzzing lies behind the onset).  A family that draws refusals also writes into its calls
#       the kind a fetch must find active and whether a rollback must be refused behind a plan
#   stats: the statistics a script reports
SHORT_SIGNAL = 0.15     # share of `plans`' signals that are 3-39 samples long, so that runs end because the signal ran out; the others 40-119
COMMON_STATS = ("room", "captures", "rolled_across", "steps")
FAMILIES = {
    "plans": SimpleNamespace(
        seeds=40, rng_base=7000, calls=(10, 19), kinds=KINDS6, first=lambda seed: KINDS6[(seed + seed // 4) % 6],
        value_anywhere=True, noise_everywhere=True, source_anywhere=True,
        signal_length=lambda rng: int(rng.integers(3, 40)) if rng.random() < SHORT_SIGNAL else int(rng.integers(40, 120)),
        late_stops=0, onsets_of="arrival",
        weights=dict(run=15, outside=1.5, value=1.5, field=3, source=0.5, receivers=0.5, memories=1.5, plan=2.5, fetch=7, checkpoint=5, rollback=14),
        stats=COMMON_STATS + ("fetched", "write_between", "outside_in_box", "onsets", "with_onset", "without_onset", "cut_segment")),
    "all-plans": SimpleNamespace(
        seeds=32, rng_base=17000, calls=(20, 34), kinds=KINDS8, first=lambda seed: KINDS8[(seed // 4) % 8],
        value_anywhere=True, noise_everywhere=True, source_anywhere=True, signal_length=lambda rng: int(rng.integers(250, 401)),
        late_stops=3, onsets_of="lateral",
        weights={"run": 18, "outside": 1.5, "value": 1.5, "field": 5, "source": 0.5, "receivers": 0.5, "memories": 1.5, "plan": 9, "fetch": 8,
                 "checkpoint": 6, "rollback": 14, "same": 1, "refused-plan": 2, "refused-rollback": 3, "stop": 1},
        stats=COMMON_STATS + ("first", "fetched", "pairs", "pairs_over_a_stop", "most_under_one_plan", "same", "refused_plans", "refused_rollbacks",
                              "refused_for", "stop_run_plan", "onsets", "with_onset", "without_onset", "lateral_bins", "cut_segment")),
    "modulation": SimpleNamespace(
        seeds=10, rng_base=16000, calls=(14, 25), kinds=("modulation",), first=lambda seed: "modulation",
        value_anywhere=False, noise_everywhere=False, source_anywhere=False, signal_length=lambda rng: int(rng.integers(250, 400)),
        late_stops=0, onsets_of=None,
        weights=dict(run=18, outside=1.5, value=1, field=2, memories=1, plan=2, fetch=6, checkpoint=4, rollback=8),
        stats=COMMON_STATS + ("fetched_something", "replaced")),
    "arrival-bands": SimpleNamespace(
        seeds=8, rng_base=19000, calls=(14, 25), kinds=("arrival_bands",), first=lambda seed: "arrival_bands",
        value_anywhere=False, noise_everywhere=False, source_anywhere=False, signal_length=lambda rng: int(rng.integers(250, 400)),
        late_stops=0, onsets_of=None,
        weights=dict(run=18, outside=1.5, value=1, field=2, memories=1, plan=2, stop=2, fetch=6, checkpoint=5, rollback=12),
        stats=COMMON_STATS + ("fetched_something", "replaced", "stopped", "tails")),
}
def can_roll_back(g):
    s = g.state
    return s["checkpoint"] and not s["source_since"] and not s["receivers_since"] and not (g.twin.plan is not None and s["plan_since"])


def rollback_is_refused(g):
    s = g.state
    return s["checkpoint"] and (s["source_since"] or s["receivers_since"]
                                or (g.twin.plan is not None and g.twin.plan["kind"] != "snapshots" and s["plan_since"]))


def fetched(g):
    """The active plan's expected outputs, and what they add to the statistics."""
    want = g.twin.expected()
    plan, kind, stats = g.twin.plan, g.twin.plan["kind"], g.stats
    if KINDS[kind].something(want, plan):
        stats["fetched"].add(kind)
    if kind == g.fam.onsets_of:
        stats["onsets"] |= set(int(v) for v in np.unique(want["onset"]) if v != A.NONE)
        stats["with_onset"] += int((want["onset"] != A.NONE).sum())
        stats["without_onset"] += int((want["onset"] == A.NONE).sum())
    if "lateral_bins" in g.fam.stats and kind == g.fam.onsets_of:
        energy = want["bins"][0]
        stats["lateral_bins"] = max(stats["lateral_bins"], int((energy.reshape(energy.shape[0], -1) != 0).any(axis=1).sum()))
    if "tails" in g.fam.stats and want["bins"].shape[1] > len(plan["edges"]) and np.any(want["bins"][:, len(plan["edges"]):]):
        stats["tails"] += 1
    return want


def leaves(g, op):
    """The active plan goes: its captures are counted, its outputs are what the engine must still show."""
    g.stats["captures"] += len(g.twin.log)
    kind, want = g.twin.plan["kind"], fetched(g)
    op.update(dict(stop=kind, want=want) if g.several else dict(want=want))
    return kind


def call_run(g, op):
    op["n"] = int(g.rng.integers(1, 12)) if g.rng.random() < 0.7 else int(g.rng.integers(16, 40))
    op["done"] = g.twin.run(op["n"])
    g.stats["steps"] += op["done"]
    if g.twin.plan is None and op["done"]:
        g.state["ran_since_stop"] = True


def call_outside(g, op):
    op["n"] = int(g.rng.integers(1, 4))
    for _ in range(op["n"]):
        g.twin.outside_step()


def call_value(g, op):
    rng = g.rng
    op["node"] = int(rng.integers(0, g.mesh.num_nodes)) if g.fam.value_anywhere and rng.random() < 0.4 else int(rng.choice(g.live))
    op["value"] = g.twin.dtype(rng.uniform(-0.5, 0.5))
    op["which"] = E.BUF_CURRENT if rng.random() < 0.7 else E.BUF_PREVIOUS
    (g.twin.cur if op["which"] == E.BUF_CURRENT else g.twin.prev)[op["node"]] = op["value"]


def call_field(g, op):
    rng = g.rng
    everywhere = g.fam.noise_everywhere and rng.random() < 0.3
    op["field"] = np.where(g.is_live | everywhere, rng.uniform(-0.25, 0.25, g.mesh.num_nodes), 0.0).astype(g.twin.dtype)
    op["which"] = E.BUF_CURRENT if rng.random() < 0.5 else E.BUF_PREVIOUS
    if op["which"] == E.BUF_CURRENT:
        g.twin.cur = op["field"].copy()
    else:
        g.twin.prev = op["field"].copy()


def call_source(g, op):
    rng, twin = g.rng, g.twin
    if g.fam.source_anywhere:
        kind = int(rng.choice([E.SOURCE_NONE, E.SOURCE_HARD, E.SOURCE_SOFT], p=[0.15, 0.4, 0.45] if g.ops else [0.0, 0.45, 0.55]))
        node = int(rng.choice(g.inside)) if rng.random() < 0.7 else int(rng.choice(g.live))
    else:
        kind, node = int(rng.choice([E.SOURCE_HARD, E.SOURCE_SOFT])), int(rng.choice(g.inside))
    sig = rng.uniform(-0.3, 0.3, g.fam.signal_length(rng))
    op.update(kind=kind, node=node, signal=sig)
    twin.kind, twin.node, twin.signal, twin.pos = kind, node, sig, 0
    g.state["source_since"] = True       # wayverb_amd.h: "The source and the receivers must be the ones in place at the checkpoint"


def call_receivers(g, op):
    rng, twin = g.rng, g.twin
    op["recv"] = [int(rng.choice(g.inside)) if rng.random() < 0.6 else int(rng.integers(0, g.mesh.num_nodes))
                  for _ in range(int(rng.integers(0, 5)))]
    twin.recv, twin.rows, twin.recv_from = op["recv"], [], twin.step_no
    g.state["receivers_since"] = True


def call_memories(g, op):
    op["d"] = int(g.rng.integers(1, 4))
    op["data"] = None
    bd = g.twin.bd[op["d"] - 1]
    if len(bd):
        bd["filter_memory"] = g.rng.uniform(-1e-3, 1e-3, bd["filter_memory"].shape)
        op["data"] = bd.copy()


def call_plan(g, op):
    """`plan`: a plan where there is none, or one that takes the active plan's place; `same`: one of the active plan's own kind."""
    twin, stats, state = g.twin, g.stats, g.state
    op.update(dict(stop=None, want=None) if g.several else dict(want=None))
    if twin.plan is not None:      # (no plan leaves unseen: its outputs are compared before another takes its place)
        leaves(g, op)
        stats["replaced"] += 1
    if op["op"] == "same":
        kind = twin.plan["kind"]
        stats["same"] += 1
    elif stats["first"] is None:
        # the first plan's kind goes round the family's with the seed: seed % 4 picks the room, so every kind meets every room (and,
        # of `all-plans`' eight, with precision_of every kind is first once in f32)
        kind = stats["first"] = g.fam.first(g.seed)
    elif not g.several:
        kind = g.fam.kinds[0]
    else:      # of another kind than the one it replaces
        kind = str(g.rng.choice([k for k in g.fam.kinds if twin.plan is None or k != twin.plan["kind"]]))
        if twin.plan is not None:
            stats["pairs"].add((twin.plan["kind"], kind))
        elif state["stopped"] != kind:
            stats["pairs_over_a_stop"].add((state["stopped"], kind))
        if twin.plan is None and state["ran_since_stop"]:
            stats["stop_run_plan"] = True
    op["plan"] = KINDS[kind].draw(g.rng, g.mesh, twin.step_no, g.live)
    twin.set_plan(op["plan"])
    state["plan_since"] = True         # (a plan set after the checkpoint: wv_rollback refuses, and the plans' own tests pin that)
    state["written"] = False
    state["plan_has_outside"] = bool(subsample(~g.is_live.reshape(g.mesh.dims[::-1]), capture_box(op["plan"]), g.mesh.dims).any())
    if g.refusals:
        op["rollback_refused"] = rollback_is_refused(g)     # (asserted on the spot: a refused rollback changes nothing)


def call_fetch(g, op):
    if g.refusals:
        op["kind"] = g.twin.plan["kind"]
    op["want"] = fetched(g)


def call_refused_plan(g, op):
    kind = str(g.rng.choice([k for k in g.fam.kinds if k != g.twin.plan["kind"]]))
    op["plan"] = KINDS[kind].draw(g.rng, g.mesh, g.twin.step_no, g.live)
    op["words"] = refusal_words(g.twin.plan["kind"], kind)
    g.stats["refused_plans"] += 1


def call_refused_rollback(g, op):
    # (engine_io.hip.h asks in this order, and says the first that holds)
    why = "receivers" if g.state["receivers_since"] else "source" if g.state["source_since"] else "plan"
    op["words"] = {"receivers": "the receivers were changed after the checkpoint", "source": "the source was changed after the checkpoint",
                   "plan": "plan was set after the checkpoint"}[why]
    g.stats["refused_rollbacks"] += 1
    g.stats["refused_for"].add(why)


def call_stop(g, op):
    """A NULL plan: compared, stopped, forgotten; runs go on without one until the next `plan`."""
    g.state["stopped"], g.state["ran_since_stop"] = leaves(g, op), False
    g.twin.set_plan(None)
    g.stats["stopped"] += 1


def call_checkpoint(g, op):
    g.twin.checkpoint()
    g.state.update(checkpoint=True, plan_since=False, source_since=False, receivers_since=False)


def call_rollback(g, op):
    if len(g.twin.log) > len(g.twin.saved["log"]):
        g.stats["rolled_across"] = True
    g.twin.rollback()


# one function per call: it draws the call's arguments, writes them into `op` and applies the call to the twin
CALLS = {"run": call_run, "outside": call_outside, "value": call_value, "field": call_field, "source": call_source, "receivers": call_receivers,
         "memories": call_memories, "plan": call_plan, "same": call_plan, "fetch": call_fetch, "refused-plan": call_refused_plan,
         "refused-rollback": call_refused_rollback, "stop": call_stop, "checkpoint": call_checkpoint, "rollback": call_rollback}
NEED_A_PLAN = ("fetch", "same", "refused-plan", "stop")


def build_script(oracle, family, seed):
    """The room, the sequence of calls and what the engine must show after each of them, from the twin alone.  dict(room, mesh, tag,
    dtype, ops, final, stats); an op is a dict with its name under "op", its arguments, the two fields behind it ("cur", "prev") and,
    wherever a plan's outputs are compared, the expected outputs under "want" (and, in a family of several kinds, the plan's kind
    under "stop" / "kind").  The order of the draws is pinned by tests/golden/plan_sequence_digests.json: a draw added, dropped or
    moved changes every script behind it."""
    fam = FAMILIES[family]
    rng = np.random.default_rng(fam.rng_base + seed)
    room, mesh = random_plan_room(rng, seed, oracle.classify)
    tag, dtype = precision_of(seed)
    t = mesh.nodes["boundary_type"]
    twin = PlanTwin(oracle, mesh, dtype)
    stats = dict(room=room, first=None, fetched=set(), pairs=set(), pairs_over_a_stop=set(), captures=0, most_under_one_plan=0, rolled_across=False,
                 write_between=False, outside_in_box=False, same=0, replaced=0, stopped=0, refused_plans=0, refused_rollbacks=0, refused_for=set(),
                 stop_run_plan=False, onsets=set(), with_onset=0, without_onset=0, lateral_bins=0, tails=0, steps=0)
    state = dict(checkpoint=False, plan_since=False, source_since=False, receivers_since=False, stopped=None, ran_since_stop=False,
                 written=False, plan_has_outside=False)
    ops = []
    g = SimpleNamespace(fam=fam, seed=seed, rng=rng, mesh=mesh, twin=twin, stats=stats, state=state, ops=ops, is_live=t != 0,
                        live=np.nonzero(t != 0)[0], inside=np.nonzero(t & M.ID_INSIDE)[0],
                        several=len(fam.kinds) > 1, refusals="refused-rollback" in fam.weights)

    def on_capture():
        stats["most_under_one_plan"] = max(stats["most_under_one_plan"], len(twin.log))
        if state["written"]:
            stats["write_between"] = True
        if state["plan_has_outside"]:
            stats["outside_in_box"] = True
    twin.on_capture = on_capture

    n_ops = int(rng.integers(*fam.calls))
    for i in range(n_ops):
        names = [k for k in fam.weights
                 if (k != "rollback" or can_roll_back(g)) and (k != "refused-rollback" or rollback_is_refused(g))
                 and (k not in NEED_A_PLAN or twin.plan is not None)
                 and (k != "plan" or not (ops and ops[-1]["op"] == "stop"))        # (a stop is followed by a call with no plan active)
                 and (k != "stop" or i < n_ops - fam.late_stops)]
        w = np.array([fam.weights[k] for k in names], dtype=np.float64)
        # forced: a source first (a sequence without a signal would capture zeros throughout), a plan second, a plan wherever a family
        # of one kind has none, and at the end if there is none
        name = ("source" if i == 0 else "plan" if i == 1 or (twin.plan is None and (not g.several or i == n_ops - 1))
                else str(rng.choice(names, p=w / w.sum())))
        op = dict(op=name)
        CALLS[name](g, op)
        if name in ("value", "field", "memories") and twin.plan is not None and twin.log:
            state["written"] = True
        op["cur"], op["prev"] = twin.cur.copy(), twin.prev.copy()
        ops.append(op)
    stats["captures"] += len(twin.log)
    final = dict(want=fetched(g) if twin.plan is not None else None, step_no=twin.step_no, memories=[b["filter_memory"].copy() for b in twin.bd])
    if g.several:
        final.update(recv=list(twin.recv), rows=[list(r) for r in twin.rows], recv_from=twin.recv_from, plan=twin.plan)
    stats.update(cut_segment=twin.cut_segment, fetched_something=bool(stats["fetched"]))
    return dict(room=room, mesh=mesh, tag=tag, dtype=dtype, ops=ops, final=final, stats={k: stats[k] for k in fam.stats})


# ---- the replay ---------------------------------------------------------------------------------------------------------------

def assert_rollback_refused(eng, words=""):
    with pytest.raises(E.WaveguideError, match="error -6: wv_rollback: .*%s" % (words or " after the checkpoint")):
        eng.rollback()


def replay(eng, script):
    """The script's calls on the engine, each followed by the comparison the script holds for it: after every call both fields, at
    every fetch, handover, stop and the end every output of the active plan, at the end the step count, the filter memories and the
    receiver rows, all BYTEWISE.  `kind` is the replay's own account of the active plan: what the script names must agree with it."""
    log = []
    kind = None
    for op in script["ops"]:
        name = op["op"]
        log.append("%s:%s" % (name, op["plan"]["kind"]) if "plan" in op else name)
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
            if op["want"] is not None:
                assert kind == op.get("stop", kind) and kind is not None, where
                assert_outputs(eng, kind, op["want"], where)
                if kind != op["plan"]["kind"]:         # (a setter replaces a plan of its own kind, no stop in between)
                    stop_plan(eng, kind)
            set_plan(eng, op["plan"])
            kind = op["plan"]["kind"]
            if op.get("rollback_refused"):
                assert_rollback_refused(eng)
        elif name == "fetch":
            assert kind == op.get("kind", kind), where
            assert_outputs(eng, kind, op["want"], where)
        elif name == "refused-plan":
            with pytest.raises(E.WaveguideError) as refusal:
                set_plan(eng, op["plan"])
            assert str(refusal.value).endswith("error -6: " + op["words"]), (str(refusal.value), where)
        elif name == "refused-rollback":
            assert_rollback_refused(eng, op["words"])
        elif name == "stop":
            assert kind == op.get("stop", kind), where
            assert_outputs(eng, kind, op["want"], where)
            stop_plan(eng, kind)
            kind = None
        elif name == "checkpoint":
            eng.checkpoint()
        else:
            assert name == "rollback", where
            eng.rollback()
        assert eng.read_field(E.BUF_CURRENT).tobytes() == op["cur"].tobytes(), where
        assert eng.read_field(E.BUF_PREVIOUS).tobytes() == op["prev"].tobytes(), where
    final = script["final"]
    where = (script["room"], script["mesh"].dims, script["tag"], log, "the end")
    assert eng.step_count() == final["step_no"], where
    assert (kind is None) == (final["want"] is None) and ("plan" not in final or kind == final["plan"]["kind"]), where
    if kind is not None:
        assert_outputs(eng, kind, final["want"], where)
    for d in (1, 2, 3):
        assert eng.read_boundary_data(d)["filter_memory"].tobytes() == final["memories"][d - 1].tobytes(), where
    if final.get("recv") and final["rows"]:
        got = eng.fetch_receivers(final["recv_from"], len(final["rows"]))
        want = np.array(final["rows"], dtype=np.float64).reshape(len(final["rows"]), len(final["recv"]))
        assert got.dtype == want.dtype and got.shape == want.shape, where
        # (a row of an outside step is NaN in every column, and so is the twin's: the payload of a NaN is nobody's contract)
        gaps = np.isnan(want)
        assert np.array_equal(np.isnan(got), gaps) and np.where(gaps, 0.0, got).tobytes() == np.where(gaps, 0.0, want).tobytes(), where


# ---- the digest ---------------------------------------------------------------------------------------------------------------

def digest(script):
    """SHA-256 over everything a script holds: the room, the mesh, the tag, every call with its arguments, fields and expected outputs,
    the end and the statistics.  Keys and sets go in sorted, arrays with dtype and shape, structured arrays field by field (their
    padding bytes are nobody's)."""
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, dict):
            h.update(b"{")
            for k in sorted(v):
                feed(k)
                feed(v[k])
            h.update(b"}")
        elif isinstance(v, (set, frozenset)):
            feed(sorted(v, key=repr))
        elif isinstance(v, (list, tuple)):
            h.update(b"[")
            for x in v:
                feed(x)
            h.update(b"]")
        elif isinstance(v, np.ndarray) and v.dtype.names:
            h.update(b"<")
            for field in v.dtype.names:
                feed(field)
                feed(v[field])
            h.update(b">")
        elif isinstance(v, (np.ndarray, np.generic)):
            v = np.asarray(v)
            h.update(("%s%s" % (v.dtype.str, v.shape)).encode())
            h.update(v.tobytes())
        else:
            assert v is None or isinstance(v, (bool, int, float, str)), type(v)
            h.update(("%s:%r;" % (type(v).__name__, v)).encode())

    mesh = script["mesh"]
    feed([script["room"], mesh.dims, mesh.nodes, mesh.coefficients, mesh.bidx, script["tag"], script["ops"], script["final"], script["stats"]])
    return h.hexdigest()

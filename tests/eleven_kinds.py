"""All eleven kinds of capture plan in one table, with no GPU in it: what tests/test_gpu_poisoned_captures.py,
tests/test_gpu_newest_fold_extremes.py and tests/test_gpu_plan_handovers.py share, and what tests/test_eleven_kinds.py holds on the CPU
before any of them means anything.  tests/plan_twin.py, tests/waterfall_twin.py and tests/interaural_twin.py are used as they are:
`registered()` nests the two twins' contexts, so that inside it plan_twin.KINDS holds the nine committed kinds and both of theirs, and
leaves plan_twin's tables as it found them.

plan_of(kind) is ONE fixed plan per kind on test_gpu_plan_extremes.BOX (270 nodes of a 12^3 box: two workgroups of a fold, the second
partly idle), stride 1, period 1, whose parameters put every fold on both sides of its own structure:
  - spectrum, modulation, waterfall: five frequencies, a full chunk of four and one over, both ends of the range among them
  - decay, banded, intensity, waterfall: 4 bins of 5 captures -- the last bin stays open beyond 20 captures
  - arrival, lateral, banded arrival, interaural: edges [0, 1, 5, 16]
  - banded arrival: two bands, lags [0, 3], a tail of 3 bins of 1 capture from relative capture 17
  - interaural: ears (-1, 0, 1) and (1, -1, 0) -- both in plan_twin's hull, one node wide -- max_lag 5 (the fold's LMAX = 8 class)
    and a cascade of four sections; UNFILTERED turns it into the float-sample instance with the longest ring: max_lag 16, no sections
second_plan_of(kind) is a smaller plan of the same kind with ANOTHER state size and box (fewer bins, edges, bands, frequencies or
lags): what replaces plan_of(kind) where a kind hands over to itself."""
import contextlib

import numpy as np

import interaural_twin as IT
import plan_twin as P
import waterfall_twin as WT
from wayverb_amd import decay as D

# the nine committed kinds in plan_twin.KINDS' order, then the two twins' (tests/test_eleven_kinds.py holds it to the tables)
KINDS11 = P.KINDS8 + ("arrival_bands", WT.KIND, IT.KIND)
assert len(KINDS11) == 11 == len(set(KINDS11))

BOX = ((1, 1, 4), (10, 9, 3))              # tests/test_gpu_plan_extremes.py's (asserted equal in tests/test_eleven_kinds.py)
SECOND_BOX = ((2, 3, 2), (7, 5, 2))        # 70 nodes: one workgroup, partly idle; its hull lies inside a 12^3 mesh
FREQS = [0.0, 0.5, 0.123, 0.31, 0.25]
EDGES = [0, 1, 5, 16]
UNFILTERED = dict(max_lag=16, sections=None)
ONSET_KINDS = ("arrival", "lateral", "arrival_bands", "interaural")
PEAK_KINDS = ("arrival", "arrival_bands")


@contextlib.contextmanager
def registered():
    with WT.registered(), IT.registered():
        yield


def octave_bands(centres):
    """One 4th-order Butterworth band-pass (four sections) per octave around `centres`, designed at the rate of the captured series."""
    return np.stack([D.butterworth_bandpass(lo, hi, 1.0) for lo, hi in D.octave_band_edges(centres)])


def _details(kind, second):
    """What a plan of `kind` has beside its cadence: the first plan's, or the second, smaller plan's."""
    freqs = FREQS[:3] if second else FREQS
    n_bins, bin_captures = (2, 3) if second else (4, 5)
    edges = [0, 2] if second else EDGES
    threshold = dict(edges=edges, threshold=0.0, threshold_map=None)
    bands = octave_bands([0.1] if second else [0.1, 0.2])
    return {
        "snapshots": dict(),
        "spectrum": dict(freqs=freqs),
        "decay": dict(n_bins=n_bins, bin_captures=bin_captures),
        "banded": dict(n_bins=n_bins, bin_captures=bin_captures, bands=bands),
        "intensity": dict(n_bins=n_bins, bin_captures=bin_captures),
        "arrival": threshold,
        "lateral": threshold,
        "modulation": dict(freqs=freqs, bands=bands),
        "arrival_bands": dict(threshold, bands=bands, lag=[2] if second else [0, 3], tail=None if second else (3, 17, 1)),
        "waterfall": dict(freqs=freqs, n_bins=n_bins, bin_captures=bin_captures),
        "interaural": dict(threshold, ear_a=(0, 0, 0) if second else (-1, 0, 1), ear_b=(0, 1, 0) if second else (1, -1, 0),
                           max_lag=2 if second else 5, sections=bands[0, 2:] if second else bands[0]),
    }[kind]


def plan_of(kind, **over):
    return dict(dict(kind=kind, box=BOX, stride=(1, 1, 1), first_step=0, period=1, **_details(kind, False)), **over)


def second_plan_of(kind, **over):
    return dict(dict(kind=kind, box=SECOND_BOX, stride=(1, 1, 1), first_step=0, period=1, **_details(kind, True)), **over)


def state_size(plan):
    """Numbers per taken node that the plan's fold keeps on the device, near enough to tell two plans of one kind apart: what
    Checkpoint::PlanSave sizes its copies by, times the nodes."""
    bands = plan.get("bands")
    k, s = (bands.shape[0], bands.shape[1]) if bands is not None else (1, 0)
    per_node = {
        "snapshots": lambda p: 1,
        "spectrum": lambda p: 2 * len(p["freqs"]),
        "decay": lambda p: p["n_bins"],
        "banded": lambda p: k * (p["n_bins"] + 2 * s),
        "intensity": lambda p: 4 * p["n_bins"] + 3,
        "arrival": lambda p: 5 + len(p["edges"]),
        "lateral": lambda p: 5 + 10 * len(p["edges"]),
        "modulation": lambda p: k * (1 + 2 * len(p["freqs"]) + 2 * s),
        "arrival_bands": lambda p: 3 + k * (2 + len(p["edges"]) + (p["tail"][0] if p["tail"] else 0) + 2 * s),
        "waterfall": lambda p: 2 * len(p["freqs"]) * p["n_bins"],
        "interaural": lambda p: 3 + len(p["edges"]) * (2 * p["max_lag"] + 3) + 2 * p["max_lag"]
                                + 4 * (0 if p["sections"] is None else len(p["sections"])),
    }[plan["kind"]](plan)
    return per_node * int(np.prod(P.taken(plan)))


# ---- comparing outputs that hold NaNs -------------------------------------------------------------------------------------------------

def assert_outputs_but_nan_bytes(got, want, where):
    """plan_twin.assert_outputs for outputs with NaNs in them: names, dtype and shape equal; NaN exactly where the definition has one;
    every other entry equal BYTEWISE, +-inf and signed zeros included.  The bytes of a NaN are nobody's contract and are not compared:
    an x86 host makes the negative quiet NaN out of inf - inf, gfx950 the positive one, and the NumPy definitions themselves give NaNs
    of both signs."""
    assert sorted(got) == sorted(want), where
    for name in sorted(want):
        g, w = got[name], want[name]
        if not isinstance(w, np.ndarray):
            assert g == w, (name, g, w, where)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape, where)
        if w.dtype.kind in "fc":
            holes = np.isnan(w)
            assert np.array_equal(np.isnan(g), holes), (name, int(np.isnan(g).sum()), int(holes.sum()), where)
            parts = [(g.real, w.real), (g.imag, w.imag)] if w.dtype.kind == "c" else [(g, w)]
            for gp, wp in parts:       # (a complex entry is NaN where either part is: the other part is still compared)
                keep = ~np.isnan(wp)
                assert np.array_equal(np.isnan(gp), ~keep), (name, where)
                assert gp[keep].tobytes() == wp[keep].tobytes(), (name, where)
        else:
            assert g.tobytes() == w.tobytes(), (name, where)


def float_outputs(want):
    return {name: v for name, v in want.items() if isinstance(v, np.ndarray) and v.dtype.kind in "fc"}


# ---- section 1's captures and conditions ----------------------------------------------------------------------------------------------

POISONS = (np.nan, np.inf, -np.inf)
POISON_STEP = 14
LAST_STEP = 30
THRESHOLD = 0.3
START_SCALE = 0.2 * THRESHOLD
PUT_BACK_SCALE = 0.25


def poisoned_nodes(mesh_dims, inside, box=BOX, seed=21):
    """15 of the box's inside nodes, a seeded choice: (node indices int64[3][5] -- NaN's, +inf's, -inf's)."""
    nx, ny, nz = mesh_dims
    (x0, y0, z0), (ex, ey, ez) = box
    in_box = np.zeros((nz, ny, nx), dtype=bool)
    in_box[z0:z0 + ez, y0:y0 + ey, x0:x0 + ex] = True
    candidates = np.nonzero(in_box.reshape(-1) & inside)[0]
    return np.random.default_rng(seed).choice(candidates, 15, replace=False).reshape(3, 5)


def poison(field, nodes):
    out = np.array(field, dtype=np.float64)
    for value, where in zip(POISONS, nodes):
        out[where] = value
    return out


def in_capture(nodes, plan, mesh_dims):
    """The poisoned nodes as boolean masks [3][...] over what the plan's outputs cover (the box; every one of them lies in it)."""
    nx, ny, nz = mesh_dims
    masks = []
    for where in nodes:
        field = np.zeros(nz * ny * nx, dtype=bool)
        field[where] = True
        masks.append(np.ascontiguousarray(P.subsample(field.reshape(nz, ny, nx), plan, mesh_dims)))
    return masks


CAN_GO_BAD = {     # per kind, the outputs a NaN or an infinite capture must reach (every float output but an arrival plan's peak, which no NaN enters)
    "snapshots": ("snapshots",), "spectrum": ("spectrum",), "decay": ("bins",), "banded": ("bins",), "intensity": ("bins", "velocity"),
    "arrival": ("peak", "pre", "moment", "bins"), "lateral": ("pre", "velocity", "bins"), "modulation": ("energy", "sums"),
    "arrival_bands": ("peak", "pre", "moment", "bins"), "waterfall": ("waterfall",), "interaural": ("pre", "bins"),
}


def assert_poison_conditions(plan, want, snaps, masks, poison_capture):
    """What keeps the NaN mask from hiding a failure, asserted on the EXPECTED values: few NaNs, something bad and something finite in
    every output that can go bad, and the onset rules.  `snaps`: the captures float32[n, ...] as the twin got them (the hull's for a
    hull kind); `masks`: in_capture's; `poison_capture`: the number of the capture that holds the poison."""
    kind = plan["kind"]
    with np.errstate(invalid="ignore"):
        for name, v in float_outputs(want).items():
            assert np.isnan(v).mean() < 0.15, (kind, name, float(np.isnan(v).mean()))
        for name in CAN_GO_BAD[kind]:
            v = want[name]
            assert (~np.isfinite(v)).any() and (np.isfinite(v) & (v != 0)).any(), (kind, name)
    if kind not in ONSET_KINDS:
        return
    onset = want["onset"]
    none = onset == 0xFFFFFFFF
    nan_nodes, plus, minus = masks
    # the magnitude the onset rule sees at every capture, as the kind's definition takes it
    if kind == "interaural":
        a, b = IT.ear_planes(plan, snaps)
        with np.errstate(invalid="ignore"):
            mag = np.fmax(np.abs(a), np.abs(b))      # (the other operand where one is a NaN)
        # a seat sees the poison at its EARS: a NaN where both hold one (none, perhaps), an infinity where either does
        touched = ~(np.isfinite(a[poison_capture]) & np.isfinite(b[poison_capture]))
        nan_nodes, infinite = np.isnan(mag[poison_capture]), np.isinf(mag[poison_capture])
        one_nan = (np.isnan(a[poison_capture]) | np.isnan(b[poison_capture])) & ~infinite
        assert touched.sum() >= 20 and infinite.sum() >= 10 and one_nan.sum() >= 5
    else:
        mag = np.abs(snaps[(slice(None),) + tuple(P.hull_of(plan)[1])]) if P.KINDS[kind].hull else np.abs(snaps)
        infinite = plus | minus
        touched = one_nan = nan_nodes
        assert nan_nodes.sum() == 5 and infinite.sum() == 10 and np.isnan(mag[poison_capture][nan_nodes]).all()
    assert mag.shape[1:] == onset.shape and np.isinf(mag[poison_capture][infinite]).all()
    thr = np.broadcast_to(np.asarray(P.threshold_of(plan), dtype=np.float32), onset.shape)
    with np.errstate(invalid="ignore"):
        reached = mag >= thr                         # False for a NaN
    quiet = ~reached.any(axis=0)
    # the onset is the first capture that reached the threshold, and there is none where none did
    assert np.array_equal(none, quiet) and np.array_equal(onset[~quiet], np.argmax(reached, axis=0)[~quiet].astype(np.uint32))
    # +-inf is an onset: the poisoned capture's or an earlier one's ("the onset capture itself" where the poison is capture 0)
    assert (onset[infinite] <= poison_capture).all() and (onset[infinite] == poison_capture).any(), (kind, onset[infinite])
    # a NaN is no onset: not at the poisoned capture, and at none where the node's other captures stay under the threshold -- of which
    # there is one at the least, and one that is heard later
    assert (onset[one_nan] != poison_capture).all()
    assert (one_nan & none).any() and (one_nan & ~none).any(), (kind, onset[one_nan])
    assert (onset[~none] > poison_capture).any() and len(np.unique(onset[~none])) >= 3, kind       # onsets behind the poison, at several captures
    if kind in PEAK_KINDS:
        assert not np.isnan(want["peak"]).any() and np.isinf(want["peak"][infinite]).all()
    if kind == "interaural" and poison_capture:
        # the history carried the poison across the fold: captures 0 .. 15 are the first fold, and a seat with onset o puts capture c
        # into bin(c - o), so a bin w with o + edges[w] >= 16 holds products of the second fold only.  One that is NaN at a seat whose
        # ears were finite from capture 16 on got the poison from the ring (or, filtered, from the cascade's state)
        assert np.isfinite(a[16:]).all() and np.isfinite(b[16:]).all()
        found = 0
        for w, e in enumerate(plan["edges"]):
            later = touched & ~none & (onset.astype(np.int64) + e >= 16)
            found += int(np.isnan(want["bins"][w][:, later]).sum())
        assert found, "no bin of the second fold is NaN at a poisoned seat"


def poison_case():
    """test_gpu_plan_extremes.the_case with a signal that lasts: a 12^3 box, a hard source of zeros in the middle, one receiver."""
    from wayverb_amd import engine as E
    from wayverb_amd import mesh as M
    mesh = M.box_mesh(12, 12, 12)
    return dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=np.zeros(40),
                recv=[mesh.compute_index(7, 6, 6)])


def poison_fields(mesh):
    """(inside, [previous, current] at START_SCALE, [previous, current] put back behind the flag at PUT_BACK_SCALE): uniform(-1, 1) on
    the inside nodes, +0.0 elsewhere.  The start stays under THRESHOLD for good (the scheme conserves energy: a field of uniform(-1, 1)
    * s keeps a standard deviation of 0.58 s, and 0.3 is 8.6 of them at s = 0.06), so no node has an onset ahead of the poisoned
    capture but an infinite one; what is put back has a standard deviation of 0.58 * 0.25 = 0.14, so that over the 16 captures behind
    it a node reaches 0.3 = 2.1 deviations often but not always: onsets at several captures, and nodes without."""
    from wayverb_amd import mesh as M
    rng = np.random.default_rng(31)
    inside = (mesh.nodes["boundary_type"] & M.ID_INSIDE) != 0
    start = [np.where(inside, rng.uniform(-1, 1, mesh.num_nodes) * START_SCALE, 0.0) for _ in range(2)]
    back = [np.where(inside, rng.uniform(-1, 1, mesh.num_nodes) * PUT_BACK_SCALE, 0.0) for _ in range(2)]
    return inside, start, back



def twin_captures(oracle, plan, poison_capture):
    """Section 1's sequence on the oracle alone, the poisoned field never stepped (the engine's run stops on its flag there and the
    fields are put back): (steps, captures float32[31, ...], the poisoned nodes).  The f64 engine is the oracle bit for bit,
    so these are the captures the GPU test sees."""
    case = poison_case()
    mesh = case["mesh"]
    inside, start, back = poison_fields(mesh)
    nodes = poisoned_nodes(mesh.dims, inside)
    twin = P.PlanTwin(oracle, mesh, np.float64)
    twin.kind, twin.node, twin.signal, twin.pos = case["source_kind"], case["source_node"], case["signal"], 0
    twin.prev, twin.cur = start[0].copy(), start[1].copy()
    twin.set_plan(plan)
    if poison_capture == POISON_STEP:
        assert twin.run(POISON_STEP - 1) == POISON_STEP - 1
        twin.outside_step()
        assert twin.next == twin.step_no == POISON_STEP
    else:
        assert poison_capture == 0 == twin.step_no
    kept = twin.cur
    twin.cur = poison(kept, nodes)
    twin.capture()                       # begin_run: the step the engine stands at is a plan step
    twin.prev, twin.cur, twin.pos = back[0].copy(), back[1].copy(), 0
    todo = LAST_STEP - twin.step_no
    assert twin.run(todo) == todo
    steps = [s for s, _ in twin.log]
    assert steps == list(range(LAST_STEP + 1))
    return np.array(steps, dtype=np.uint64), np.stack([a for _, a in twin.log]), nodes


# ---- section 2's plans ------------------------------------------------------------------------------------------------------------------

EXTREME_CASES = [("arrival_bands", False), ("arrival_bands", True), ("waterfall", False), ("interaural", False), ("interaural", True),
                 ("interaural-unfiltered", False), ("interaural-unfiltered", True)]
EXTREME_MAIN = {"arrival_bands": "bins", "waterfall": "waterfall", "interaural": "bins"}      # the output that must not be all zeros


def extreme_plan(name, scale, with_map):
    """plan_of for tests/test_gpu_newest_fold_extremes.py: the sections are test_gpu_plan_extremes.scaled_bands()'s cascade -- twice, as
    two bands, for the banded arrival plan, once for the filtered interaural plan -- and the map is made as that file makes it: around
    half the field's scale, a decade either way, so that at 1e-41 every entry is a subnormal float."""
    from test_gpu_plan_extremes import scaled_bands
    kind = name.split("-")[0]
    over = {}
    if name == "arrival_bands":
        over["bands"] = np.concatenate([scaled_bands(), scaled_bands()])
    elif name == "interaural":
        over["sections"] = scaled_bands()[0]
    elif name == "interaural-unfiltered":
        over.update(UNFILTERED)
    plan = plan_of(kind, **over)
    if with_map:
        factors = 10.0 ** np.random.default_rng(12).uniform(-1, 1, P.taken(plan)[::-1])
        plan["threshold_map"] = (0.5 * scale * factors).astype(np.float32)
    return plan


def first_section_state(section, series):
    """The two memories of one biquad section (decay.biquad_cascade's three lines) behind `series` float32[T, ...]: float64[2, ...]."""
    b0, b1, b2, a1, a2 = (np.float64(v) for v in section)
    z1, z2 = np.zeros(series.shape[1:]), np.zeros(series.shape[1:])
    for x in series.astype(np.float64):
        out = x * b0 + z1
        z1 = (x * b1 - a1 * out) + z2
        z2 = x * b2 - a2 * out
    return np.stack([z1, z2])


def assert_extreme_conditions(name, plan, scale, want, snaps):
    """What the expected values must hold before the comparison means anything: finite, not all zeros, with a map nodes with an onset
    and nodes without and three distinct onsets, without one every onset at capture 0 (|p| >= 0 holds of a zero too); behind a filter at
    1e-41, more than half of the first section's states subnormal doubles."""
    kind = plan["kind"]
    tiny64 = np.finfo(np.float64).tiny
    assert np.any(want[EXTREME_MAIN[kind]] != 0) and all(np.isfinite(v).all() for v in float_outputs(want).values()), name
    if kind in ONSET_KINDS:
        heard = want["onset"] != 0xFFFFFFFF
        if plan["threshold_map"] is not None:
            assert heard.any() and (~heard).any() and len(np.unique(want["onset"][heard])) >= 3, name
        else:
            assert (want["onset"] == 0).all(), name
    sections = plan["bands"][0] if kind == "arrival_bands" else plan.get("sections")
    if sections is not None and scale < 1:
        series = IT.ear_planes(plan, snaps)[0] if kind == "interaural" else snaps
        with np.errstate(under="ignore"):
            state = first_section_state(sections[0], series)
        assert ((state != 0) & (np.abs(state) < tiny64)).mean() > 0.5, name


# ---- section 3's script -----------------------------------------------------------------------------------------------------------------

HANDOVER_THRESHOLD = 0.3      # of the four kinds with an onset: noise of uniform(-0.25, 0.25) reaches it at some nodes and not at others
RUNS = dict(first=21, on=5, under_b=7, passes=19, end=3)


def handover_plan(kind, second=False, **over):
    make = second_plan_of if second else plan_of
    return make(kind, **dict(dict(threshold=HANDOVER_THRESHOLD) if kind in ONSET_KINDS else {}, **over))


def handover_mesh():
    """A 12^3 box whose walls have filters with memory (tests/test_gpu_triple.py's source of them)."""
    from wayverb_amd import mesh as M
    return M.box_mesh(12, 12, 12, coefficients=M.passive_peak_filter_coefficients(np.random.default_rng(2), 2), surface_of_face=[0, 1, 0, 1, 0, 1])


def handover_script(oracle, a, b, f32):
    """The handover of kind `a` to kind `b` as a script plan_twin.replay plays on an engine (its calls are plan_twin.set_plan, stop_plan,
    assert_outputs, assert_rollback_refused and refusal_words' sentence), the same for every pair, inside registered():

       1  plan_of(a) set, 21 steps: one fold of 16 captures, 6 staged        7  a checkpoint under b
       2  a checkpoint: folds, and fills PlanSave[a]                          8  19 steps; every output compared
       3  5 steps                                                             9  a rollback; every output compared: the checkpoint's
       4  a != b: b's setter refused in refusal_words(a, b), a's outputs     10  19 steps again; every output compared: the first pass's,
          compared, a stopped.  a == b: nothing -- 5 replaces in one call        bytewise
       5  b's plan set, first_step two steps in the past; 7 steps            11  b stopped: its count says that no plan is set
       6  a rollback: refused where b accumulates on the device (the plan   12  3 steps
          was set after the checkpoint); b == snapshots: it goes through,
          and the script goes on from the checkpoint's step

    where a == b the plan of 5 is second_plan_of(a): another state size, another box.  Returns the script and what
    tests/test_eleven_kinds.py asserts of it: dict(a_captures, b_before, b_after, something)."""
    from wayverb_amd import engine as E
    mesh = handover_mesh()
    tag, dtype = ("f32", np.float32) if f32 else ("f64", np.float64)
    rng = np.random.default_rng(29000 + 11 * KINDS11.index(a) + KINDS11.index(b))
    twin = P.PlanTwin(oracle, mesh, dtype)
    live = mesh.nodes["boundary_type"] != 0
    ops = []

    def did(op):
        op["cur"], op["prev"] = twin.cur.copy(), twin.prev.copy()
        ops.append(op)

    def run(n):
        done = twin.run(n)
        assert done == n
        did(dict(op="run", n=n, done=done))

    def fetch():
        with np.errstate(all="ignore"):
            want = twin.expected()
        did(dict(op="fetch", kind=twin.plan["kind"], want=want))
        return want

    def same_outputs(x, y):
        return sorted(x) == sorted(y) and all(x[k].tobytes() == y[k].tobytes() if isinstance(x[k], np.ndarray) else x[k] == y[k] for k in x)

    ci = mesh.compute_index
    twin.kind, twin.node, twin.signal, twin.pos = E.SOURCE_HARD, ci(6, 6, 6), rng.uniform(-0.3, 0.3, 80), 0
    did(dict(op="source", kind=twin.kind, node=twin.node, signal=twin.signal))
    for which in (E.BUF_PREVIOUS, E.BUF_CURRENT):
        field = np.where(live, rng.uniform(-0.25, 0.25, mesh.num_nodes), 0.0).astype(dtype)
        if which == E.BUF_CURRENT:
            twin.cur = field.copy()
        else:
            twin.prev = field.copy()
        did(dict(op="field", field=field, which=which))
    twin.recv, twin.rows, twin.recv_from = [ci(7, 5, 5)], [], 0
    did(dict(op="receivers", recv=list(twin.recv)))
    # 1 - 3
    plan_a = handover_plan(a)
    twin.set_plan(plan_a)
    did(dict(op="plan", plan=plan_a, stop=None, want=None))
    run(RUNS["first"])
    twin.checkpoint()
    did(dict(op="checkpoint"))
    run(RUNS["on"])
    # 4, 5
    plan_b = handover_plan(b, second=a == b, first_step=twin.step_no - 2)
    with np.errstate(all="ignore"):
        want_a = twin.expected()
    a_captures = want_a["count"][0]
    if a != b:
        did(dict(op="refused-plan", plan=plan_b, words=P.refusal_words(a, b)))
        did(dict(op="fetch", kind=a, want=want_a))
        did(dict(op="stop", stop=a, want=want_a))
        twin.set_plan(None)
        twin.set_plan(plan_b)
        did(dict(op="plan", plan=plan_b, stop=None, want=None))
    else:
        assert state_size(plan_a) != state_size(plan_b) and plan_a["box"] != plan_b["box"]
        twin.set_plan(plan_b)
        did(dict(op="same", plan=plan_b, stop=a, want=want_a))
    set_at = twin.step_no
    run(RUNS["under_b"])
    # 6
    if b == "snapshots":
        # engine_snapshot.hip.h, snapshot_rollback: the plan was set after the checkpoint, at a later step, so no snapshot stays and the
        # next one is the first plan step at or after the step the plan was set at
        assert twin.log and twin.log[0][0] == set_at > twin.saved["step_no"]
        twin.rollback()
        twin.log, twin.next = [], P.next_plan_step(plan_b, set_at)
        did(dict(op="rollback"))
        b_before = 0
    else:
        did(dict(op="refused-rollback", words="plan was set after the checkpoint"))
        b_before = len(twin.log)
    # 7 - 10
    twin.checkpoint()
    did(dict(op="checkpoint"))
    at_checkpoint = fetch()
    run(RUNS["passes"])
    first_pass = fetch()
    twin.rollback()
    did(dict(op="rollback"))
    assert same_outputs(fetch(), at_checkpoint)
    run(RUNS["passes"])
    second_pass = fetch()
    assert same_outputs(second_pass, first_pass)
    b_after = second_pass["count"][0] - at_checkpoint["count"][0]
    # 11, 12
    did(dict(op="stop", stop=b, want=second_pass))
    twin.set_plan(None)
    run(RUNS["end"])
    final = dict(want=None, step_no=twin.step_no, memories=[m["filter_memory"].copy() for m in twin.bd], recv=list(twin.recv),
                 rows=[list(r) for r in twin.rows], recv_from=twin.recv_from)
    script = dict(room="box", mesh=mesh, tag=tag, dtype=dtype, ops=ops, final=final, stats={})
    return script, dict(a_captures=a_captures, b_before=b_before, b_after=b_after, something=P.KINDS[b].something(second_pass, plan_b),
                        a_something=P.KINDS[a].something(want_a, plan_a))


def extreme_captures(oracle, plan, scale):
    """Section 2's run on the oracle, which the f64 engine is bit for bit: (steps, captures float32[21, ...], the placed negative
    zeros over what is captured)."""
    from test_gpu_plan_extremes import STEPS, fields_of, the_case
    case = the_case()
    mesh = case["mesh"]
    previous, current, placed = fields_of(mesh, scale)
    twin = P.PlanTwin(oracle, mesh, np.float64)
    twin.kind, twin.node, twin.signal, twin.pos = case["source_kind"], case["source_node"], case["signal"], 0
    twin.prev, twin.cur = previous.copy(), current.copy()
    twin.set_plan(plan)
    with np.errstate(under="ignore"):
        assert twin.run(STEPS) == STEPS
    here = np.ascontiguousarray(P.subsample(placed.reshape(mesh.dims[::-1]), P.capture_box(plan), mesh.dims))
    return np.array([s for s, _ in twin.log], dtype=np.uint64), np.stack([a for _, a in twin.log]), here

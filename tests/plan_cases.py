"""What the GPU tests of the capture plans share, with no test in it and no GPU at import: the stepping forms and the engine of a golden
case (FORMS, make_engine), the tables of cases the per-kind files draw their parameters from (FORM_CASES, BOXES, HULL_BOXES, LAYOUTS),
the reference of every comparison (reference_snapshots: an identical engine with a SNAPSHOT plan, computed once per key and read
only), the filter sections, frequencies and data-drawn thresholds the files name, the columns the life-cycle tests need beside
plan_twin.KINDS (COLUMNS, kind_row) and the one comparison of a plan with its definition (check).

A plan here is plan_twin's: dict(kind, box=((x0, y0, z0), extent), stride=(sx, sy, sz), first_step, period, the kind's details);
plan_on writes one from what the tests say ("mesh", an extent of None, a scalar stride).  A threshold or a threshold map that a
test draws from the data is a callable(snaps, plan) in the plan's details; `resolved` calls it once the reference snapshots exist.

A new kind of plan is one entry of plan_twin.KINDS (or a twin of its own, registered through eleven_kinds.registered) and one entry
of COLUMNS; tests/test_eleven_kinds.py holds the two tables to each other and to the engine on the CPU, and
tests/test_gpu_plan_life_cycle.py then runs the kind through the whole life cycle."""
from types import SimpleNamespace

import numpy as np

import cases
import plan_twin as P
from helpers import initial_fields, set_tuning
from wayverb_amd import arrival as A
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import interaural as IA
from wayverb_amd import mesh as M

# how tests/test_gpu_pair.py and tests/test_gpu_triple.py force theirs (tile_lists=0: a small box would otherwise count as a sparse room)
FORMS = {
    "single": dict(pair=0, triple=0),
    "graph": dict(pair=0, triple=0, graph=1),
    "pair": dict(pair=1, triple=0, tile_lists=0),
    "triple": dict(pair=1, triple=1, tile_lists=0),
}
ALL_FORMS = dict(FORMS, whole=dict(pair=0, triple=0, whole_step=1))     # (one launch per step)


def default_tuning_afterwards():
    """What every plan test file's autouse fixture does behind its test: the library's defaults for whatever runs next."""
    set_tuning()


def make_engine(case, tag, plan=None):
    eng = E.Engine(case["mesh"], precision=tag)
    if case["init"] is not None:
        prev, cur = initial_fields(case, eng.dtype)
        eng.write_field(prev, E.BUF_PREVIOUS)
        eng.write_field(cur, E.BUF_CURRENT)
    eng.set_source(case["source_kind"], case["source_node"], case["signal"])
    eng.set_receivers(case["recv"])
    if plan is not None:
        eng.set_snapshots(**plan)
    return eng


FORM_CASES = [("single", 1, None), ("single", 5, None), ("graph", 16, None),
              ("pair", 2, E.Engine.QUERY_PASSES), ("pair", 3, E.Engine.QUERY_PASSES), ("pair", 7, E.Engine.QUERY_PASSES),
              ("triple", 3, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 4, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 7, E.Engine.QUERY_TRIPLE_PASSES)]
# for the folds that carry a state from capture to capture: period 1 (every step ends a pass), 3 (three-step passes stay whole) and 7
STATE_FORM_CASES = [("single", 1, None), ("single", 7, None), ("graph", 1, None), ("graph", 3, None),
                    ("pair", 1, None), ("pair", 3, E.Engine.QUERY_PASSES), ("pair", 7, E.Engine.QUERY_PASSES),
                    ("triple", 1, None), ("triple", 3, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 7, E.Engine.QUERY_TRIPLE_PASSES)]
FORM_QUERIES = {"single": None, "graph": None, "pair": E.Engine.QUERY_PASSES, "triple": E.Engine.QUERY_TRIPLE_PASSES}

BOXES = {
    "sub-box-630": dict(box=((3, 2, 4), (10, 9, 7))),             # not a multiple of 64, an odd number of rows; two nodes per lane
    "sub-box-567-odd": dict(box=((3, 2, 4), (9, 9, 7))),          # an odd B: one node per lane, three workgroups, a tail
    "sub-box-16-byte-rows": dict(box=((4, 1, 2), (16, 5, 3))),
    "every-face-stride-3": dict(box="mesh", stride=3),            # 24 / 3, 20 / 3 and 28 / 3: the last two do not divide
    "strides-1-2-3": dict(box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3)),
    "one-node": dict(box=((5, 6, 7), (1, 1, 1))),
}
# for the kinds that take every node's six neighbours: the hull stays on the grid
HULL_BOXES = {
    "sub-box-630": dict(box=((3, 2, 4), (10, 9, 7))),             # not a multiple of 64, three workgroups of the fold, a tail
    "sub-box-567-odd": dict(box=((3, 2, 4), (9, 9, 7))),
    "sub-box-16-byte-rows": dict(box=((4, 1, 2), (16, 5, 3))),
    "strides-1-2-3": dict(box=((1, 1, 2), (21, 18, 24)), stride=(1, 2, 3)),
    "interior-stride-3": dict(box=((1, 1, 1), (22, 18, 26)), stride=3),
    "one-node": dict(box=((5, 6, 7), (1, 1, 1))),
    "hull-touches-every-face": dict(box=((1, 1, 1), (22, 18, 26))),   # the neighbours of the outermost nodes are wall nodes
}

# (n_bins, bin_captures) against the 16-slot stage, 33 captures: 16 + 16 + 1 for the fetch
LAYOUTS = {
    "W1-every-capture-a-new-bin": (33, 1),       # r = t
    "W5-edges-inside-and-across-folds": (7, 5),
    "W16-a-stage-per-bin": (3, 16),
    "W17": (2, 17),
    "W40-whole-folds-in-one-bin": (2, 40),      # (the second bin stays +0.0)
    "one-bin": (1, 1),
    "open-ended-last-bin": (4, 3),               # 12 captures fill the bins, the last takes the other 21
    "more-bins-than-captures": (4096, 1),
}


def case_of(case):
    """A case of tests/golden/cases.py by its name, or the case itself."""
    return cases.CASES[case]() if isinstance(case, str) else case


_reference = {}


def reference_snapshots(case_name, tag, form, plan, n_steps):
    """(snapshots, steps) of an identical engine with a snapshot plan of the same box and cadence; computed once per key, read only."""
    key = (case_name, tag, form, repr(sorted(plan.items())), n_steps)
    if key not in _reference:
        set_tuning(**FORMS[form])
        eng = make_engine(cases.CASES[case_name](), tag, plan)
        try:
            assert eng.run_steps(n_steps) == (n_steps, 0)
            snaps, steps = eng.fetch_snapshots()
        finally:
            eng.close()
        snaps.setflags(write=False)
        _reference[key] = (snaps, steps)
    return _reference[key]


_sections = {}


def sections(k_bands, n_sections):
    """K octave bands from 0.2 cycles per capture downwards, the first S sections of the 4th-order Butterworth band-pass (S = 1: the
    reference's single band-pass biquad).  Designed once, read only."""
    key = (k_bands, n_sections)
    if key not in _sections:
        edges = D.octave_band_edges([0.2 / 2 ** k for k in range(k_bands)])
        if n_sections == 1:
            s = np.stack([D.bandpass_biquad(lo, hi, 1.0) for lo, hi in edges])
        else:
            s = np.stack([D.butterworth_bandpass(lo, hi, 1.0)[4 - n_sections:] for lo, hi in edges])
        s.setflags(write=False)
        _sections[key] = s
    return _sections[key]


def box_scene():
    """A 24^3 box room with a flat wall filter as canonical() takes it: (simulation, voxels and mesh, source, receiver)."""
    from wayverb_amd import simulation as W
    mesh = M.box_mesh(24, 24, 24, coefficients=np.array([M.flat_coefficients(0.1)], dtype=M.coefficients_dtype))
    vm = W.VoxelsAndMesh(None, None, 0, None, None, mesh, (0.0, 0.0, 0.0))
    sp = mesh.spacing
    return W, vm, (12 * sp, 12 * sp, 12 * sp), (15 * sp, 12 * sp, 12 * sp)


# ---- plans as the tests write them ----------------------------------------------------------------------------------------------------

def plan_on(case, kind, box="mesh", stride=1, first_step=0, period=1, **details):
    """plan_twin's plan of `kind` on the mesh of `case` (a name, a case or the mesh's dims): "mesh" and extents of None filled in, a
    scalar stride three times; a plan with a threshold has a threshold map, None unless `details` bring one."""
    dims = tuple(case) if isinstance(case, (tuple, list)) else case_of(case)["mesh"].dims
    origin, extent = ((0, 0, 0), (None, None, None)) if isinstance(box, str) else box
    extent = tuple(d - o if e is None else e for d, o, e in zip(dims, origin, extent))
    stride = (stride,) * 3 if np.isscalar(stride) else tuple(stride)
    if "threshold" in details:
        details = dict(dict(threshold_map=None), **details)
    return dict(kind=kind, box=(tuple(origin), extent), stride=stride, first_step=first_step, period=period, **details)


def cadence_of(plan):
    """The plan's box and cadence as a setter's keywords."""
    return dict(box=plan["box"], stride=plan["stride"], first_step=plan["first_step"], period=plan["period"])


def constants(plan):
    """Of a plan as the tests write it: the integrator sees a series sampled every `period` steps, that rate."""
    return P.intensity_constants(dict(dict(period=1), **plan))


def hull_of(plan):
    """plan: box = ((x0, y0, z0), extent in mesh nodes), stride, period, first_step as the tests write it -> the snapshot plan of the
    box's hull at stride 1 and the same cadence, and the slices that pick the taken nodes out of a hull snapshot (plan_twin.hull_of)."""
    stride = plan.get("stride", 1)
    hull, box_in_hull = P.hull_of(dict(box=plan["box"], stride=(stride,) * 3 if np.isscalar(stride) else tuple(stride)))
    hplan = dict(box=hull, period=plan.get("period", 1))
    if "first_step" in plan:
        hplan["first_step"] = plan["first_step"]
    return hplan, box_in_hull


def captured_by(plan):
    """The snapshot plan that takes what the kind's definition reads: the box itself, or the hull of the box at stride 1."""
    cut = P.capture_box(plan)
    return dict(cadence_of(plan), box=cut["box"], stride=cut["stride"])


def whole_mesh(plan):
    """... or the whole mesh: an interaural plan's ears lie up to eight nodes from the seat, plan_twin's hull is one node wide."""
    return dict(box="mesh", first_step=plan["first_step"], period=plan["period"])


def resolved(plan, snaps):
    """The plan with the thresholds its test draws from the data: callables(snaps, plan), the scalar first."""
    out = dict(plan)
    for key in ("threshold", "threshold_map"):
        if callable(out.get(key)):
            out[key] = out[key](snaps, out)
    return out


def scaled_map(threshold, factors):
    """A per-node map of `factors(shape)` times the data-drawn `threshold`, for a plan whose scalar threshold is 0."""
    return lambda snaps, plan: (threshold(snaps, plan) * factors(P.taken(plan)[::-1])).astype(np.float32)


def box_of(snaps, plan):
    """The taken nodes' own snapshots [T][nz][ny][nx] out of a hull kind's."""
    return np.ascontiguousarray(snaps[(slice(None),) + tuple(P.hull_of(plan)[1])])


def median_threshold(snaps, plan=None):
    """The median, over the box's nodes, of the reference snapshots' per-node max |p| (float32, as the plan holds it)."""
    return np.float32(np.median(np.abs(snaps).max(axis=0)))


def quantile_threshold(snaps, plan, q):
    """The q-quantile, over the box's nodes that ever hold anything, of the per-node max |p| (float32, as the plan holds it)."""
    highest = np.abs(box_of(snaps, plan)).max(axis=0)
    return np.float32(np.quantile(highest[highest > 0], q))


def median_or_lower_quartile(snaps, plan=None):
    """The median, over the box's nodes, of the snapshots' per-node max |p|, so that lanes of one wave sit in different bins; where
    that is 0 (an impulse seen at an even period: more than half of the nodes never move) the lower quartile of the non-zero maxima."""
    highest = np.abs(snaps).max(axis=0)
    median = np.float32(np.median(highest))
    return median if median > 0 or not (highest > 0).any() else np.float32(np.quantile(highest[highest > 0], 0.25))


def ears_on_the_mesh(plan, snaps):
    """The two ear planes float32[T, nz, ny, nx] cut from snapshots of the whole mesh: every taken node's, an ear's offset away."""
    out = []
    for ear in (plan["ear_a"], plan["ear_b"]):
        cut = []
        for axis in range(3):
            first, ext, s = plan["box"][0][axis] + ear[axis], plan["box"][1][axis], plan["stride"][axis]
            assert first >= 0 and first + ext - 1 - (ext - 1) % s < snaps.shape[3 - axis]
            cut.append(slice(first, first + ext, s))
        out.append(np.ascontiguousarray(snaps[:, cut[2], cut[1], cut[0]]))
    return out


def levels(a, b):
    """Interaural thresholds made of the INPUT: a scalar half the nodes reach early, and a map that puts every node's onset at a
    capture of its own -- and every seventh node's nowhere."""
    mag = np.fmax(np.abs(a), np.abs(b))
    rng = np.random.default_rng(a.shape[0])
    order = np.sort(mag.reshape(mag.shape[0], -1), axis=0)
    pick = rng.integers(0, mag.shape[0], order.shape[1])
    tmap = order[pick, np.arange(order.shape[1])].astype(np.float32)
    tmap[3::7] = np.float32(3e38)
    return float(np.median(mag.max(axis=0))) * 0.5, tmap.reshape(mag.shape[1:])


def ear_level(snaps, plan):
    return levels(*ears_on_the_mesh(plan, snaps))[0]


def ear_map(snaps, plan):
    return levels(*ears_on_the_mesh(plan, snaps))[1]


def interaural_on_the_mesh(plan, snaps, steps):
    a, b = ears_on_the_mesh(plan, snaps)
    out = IA.interaural_fold(a, b, P.threshold_of(plan), plan["edges"], plan["max_lag"], plan["sections"])
    return dict(captures=len(snaps), onset=out["onset"], pre=out["pre"], bins=np.ascontiguousarray(out["bins"]))


# ---- the columns of the kinds table that the life cycle needs --------------------------------------------------------------------------
# queries: Engine.QUERY_<KIND>_{CAPTURES, FOLDS, NS}, and _GATHERS / _GATHER_NS where the kind gathers ahead of its fold.
# rollback: what wv_rollback says of this kind's plan set after the checkpoint; no_plan: what the kind's count and fetch say once the
# plan is stopped (behind "error -6: ").  answer: (the Engine attribute that holds the setter's answer, the output of that shape).
# meaningful(want, plan, at=None): the comparison is not one of zeros, as the kind's tests state it -- for the kinds with an onset, with
# `at`: onsets on both sides of capture `at`.  spread: what check() asserts instead where the kind's tests ask more of a whole run.
# captures(plan) / expect(plan, snaps, steps): the reference's snapshot plan and the definition over it, where they are not
# plan_twin's (captured_by, KINDS[kind].expect).

def queries(name, gathers=False):
    names = ("captures", "folds", "ns") + (("gathers", "gather_ns") if gathers else ())
    return {n: getattr(E.Engine, "QUERY_%s_%s" % (name, n.upper())) for n in names}


def sentences(name, fetch, lost, count=None):
    return dict(rollback="wv_rollback: the %s plan was set after the checkpoint (%s no copy to go back to)" % (name, lost),
                no_plan=dict(count="wv_%s_count: no %s plan is set" % (count or name, name), fetch="wv_fetch_%s: no %s plan is set" % (fetch, name)))


def every_band(bins):
    """every band of [K, n_bins, ...] holds something"""
    return bool((bins.reshape(bins.shape[0], -1).max(axis=1) > 0).all())


def every_band_and_frequency(energy, sums):
    """every band holds energy, and every frequency of every band a sum"""
    k, m = sums.shape[:2]
    return bool((energy.reshape(k, -1).max(axis=1) > 0).all() and (np.abs(sums).reshape(k, m, -1).max(axis=2) > 0).all())


def every_plane(bins, velocity):
    return all(np.abs(bins[a]).max() > 0 for a in range(4)) and all(np.abs(velocity[a]).max() > 0 for a in range(3))


def onsets(want, plan, at=None):
    """A node with an onset; with `at`, onsets up to capture `at` and onsets behind it."""
    heard = want["onset"] != A.NONE
    if at is None:
        return bool(heard.any())
    return bool((want["onset"][heard] <= at).any() and (want["onset"][heard] > at).any())


def heard_and_unheard(want):
    heard = want["onset"] != A.NONE
    return bool(heard.any() and (~heard).any())


def filled_bins(plane):
    return (np.abs(plane).reshape(plane.shape[0], -1).max(axis=1) > 0).sum()


def quarters(want, plan):
    """What the reference alone must show before a comparison means anything: at least a quarter of the nodes with an onset, at
    least a quarter without, three distinct onsets, two bins that hold something (a lateral plan: in E)."""
    heard = want["onset"] != A.NONE
    nodes = heard.size
    assert heard.sum() >= nodes / 4 and (~heard).sum() >= nodes / 4, (heard.sum(), nodes)
    assert len(set(want["onset"][heard].tolist())) >= 3, sorted(set(want["onset"][heard].tolist()))
    assert filled_bins(want["bins"][0] if plan["kind"] == "lateral" else want["bins"]) >= 2
    return True


def quarters_and_tensor(want, plan):
    """... and (a lateral plan) two bins in at least one Q plane."""
    return quarters(want, plan) and max(filled_bins(want["bins"][a]) for a in range(4, 10)) >= 2


def spread_in_every_band(want, plan):
    heard = want["onset"] != A.NONE
    assert heard.any() and (~heard).any() and len(set(want["onset"][heard].tolist())) >= 3
    return bool((want["bins"].reshape(want["bins"].shape[:2] + (-1,)).max(axis=2) > 0).sum(axis=1).min() >= 2)


def column(queries, sentences, answer, meaningful, spread=None, captures=captured_by, expect=None):
    return SimpleNamespace(queries=queries, rollback=sentences["rollback"], no_plan=sentences["no_plan"], answer=answer, meaningful=meaningful,
                           spread=spread or meaningful, captures=captures, **(dict(expect=expect) if expect else {}))


COLUMNS = {
    "spectrum": column(queries("SPECTRUM"), sentences("spectrum", "spectrum", "its sums have"), ("spectrum_shape", "spectrum"),
                       lambda want, plan, at=None: bool(np.abs(want["spectrum"]).max() > 0)),
    "decay": column(queries("DECAY"), sentences("decay", "decay", "its bins have"), ("decay_shape", "bins"),
                    lambda want, plan, at=None: bool(want["bins"].max() > 0)),
    "banded": column(queries("DECAY"), sentences("decay", "decay", "its bins have"), ("decay_shape", "bins"),
                     lambda want, plan, at=None: every_band(want["bins"])),
    "intensity": column(queries("INTENSITY", gathers=True), sentences("intensity", "intensity", "its bins have"), ("intensity_shape", "bins"),
                        lambda want, plan, at=None: every_plane(want["bins"], want["velocity"])),
    "arrival": column(queries("ARRIVAL"), sentences("arrival", "arrival", "its state has"), ("arrival_shape", "bins"), onsets, spread=quarters),
    "lateral": column(queries("LATERAL", gathers=True), sentences("lateral", "lateral", "its state has"), ("lateral_shape", "bins"), onsets,
                      spread=quarters_and_tensor),
    "modulation": column(queries("MODULATION"), sentences("modulation", "modulation", "its sums have"), ("modulation_shape", "sums"),
                         lambda want, plan, at=None: every_band_and_frequency(want["energy"], want["sums"])),
    "arrival_bands": column(queries("ARRIVAL_BANDS"), sentences("banded arrival", "arrival_bands", "its state has", count="arrival_bands"),
                            ("arrival_bands_shape", "bins"), onsets, spread=spread_in_every_band),
    "waterfall": column(queries("WATERFALL"), sentences("waterfall", "waterfall", "its sums have"), ("waterfall_shape", "waterfall"),
                        lambda want, plan, at=None: bool(np.abs(want["waterfall"].real).max() > 0)),
    "interaural": column(queries("INTERAURAL"), sentences("interaural", "interaural", "its state has"), ("interaural_shape", "bins"),
                         lambda want, plan, at=None: bool(np.abs(want["bins"]).max() > 0), captures=whole_mesh, expect=interaural_on_the_mesh),
}
COLUMN_NAMES = ("queries", "rollback", "no_plan", "answer", "meaningful", "spread", "captures")


def kind_row(kind):
    """plan_twin.KINDS' entry of `kind` with the life cycle's columns beside it (inside eleven_kinds.registered())."""
    return SimpleNamespace(**dict(vars(P.KINDS[kind]), **vars(COLUMNS[kind])))


def expected(plan, snaps, steps):
    """Every output of the plan by the shipped definition over the reference's captures, under PlanTwin.expected's names."""
    n = len(snaps)
    return {"count": (n, int(steps[-1]) if n else 0), **kind_row(plan["kind"]).expect(plan, snaps, steps)}


def refuses(call, sentence):
    """WV_E_STATE with the full sentence."""
    import pytest
    with pytest.raises(E.WaveguideError) as refusal:
        call()
    assert str(refusal.value).endswith("error -6: " + sentence), str(refusal.value)


def plan_engine(case, tag, form, plan):
    """An engine of the case in the stepping form with the plan set: the setter's node axes are the plan's."""
    set_tuning(**ALL_FORMS[form])
    eng = make_engine(case_of(case), tag)
    try:
        P.set_plan(eng, plan)
    except BaseException:
        eng.close()
        raise
    return eng


def check(kind, case_name, tag, form, plan, n_steps, query=None, condition="the kind's"):
    """One run of `n_steps` under the plan against the definition over the reference's snapshots (of the hull for a hull kind), taken
    in the same form: the run's result and the count, the fetch and its captures, the CAPTURES query and the bound on the folds, dtype
    and shape against the setter's answer and the definition, every output BYTEWISE, the kind's condition that the comparison is not
    one of zeros (`condition`: another, or None for a plan that cannot show it) and a non-zero last snapshot.  Returns (the outputs as
    fetched, the definition's, the resolved plan, snapshots, steps)."""
    row = kind_row(kind)
    snaps, steps = reference_snapshots(case_name, tag, "single" if form == "whole" else form, row.captures(plan), n_steps)
    plan = resolved(plan, snaps)
    want = expected(plan, snaps, steps)
    where = (kind, case_name, tag, form, n_steps)
    eng = plan_engine(case_name, tag, form, plan)
    try:
        answer = tuple(getattr(eng, row.answer[0]))
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert row.count(eng) == (len(steps), int(steps[-1]))
        got = row.fetch(eng)
        assert got.get("captures", len(steps)) == len(steps) > 1
        if query is not None:
            assert eng.query(query) > 0
        assert eng.query(row.queries["captures"]) == len(steps)
        assert eng.query(row.queries["folds"]) <= -(-len(steps) // 16) + 1
        P.assert_outputs(eng, kind, want, where)
    finally:
        eng.close()
    assert answer == want[row.answer[1]].shape, (answer, want[row.answer[1]].shape)
    condition = row.spread if condition == "the kind's" else condition
    assert condition is None or condition(want, plan), where
    assert np.abs(snaps[-1]).max() > 0      # (the comparison is not of zeros)
    return got, want, plan, snaps, steps


# ---- the life cycle's plans: each kind's own parameters, test by test, as the kinds' files had them ------------------------------------

TESTS = ("counts", "mid_run", "calls", "flag", "rollback", "generic", "nothing", "timing")
FREQS5 = [0.0, 0.5, 0.125, 0.0371, 1.0 / 3.0]
EDGES5 = (0, 1, 5, 16, 17)
TAIL_W3 = (4, 19, 3)          # begins inside the second fold for an onset at capture 0; its last bin is open-ended from rel 28 on
SECTIONS = D.butterworth_bandpass(500.0, 2000.0, 8000.0)                # four sections; [:1] is a cascade of one
EDGES4 = [0, 3, 8, 20]
SEAT_EARS = dict(ear_a=(0, -2, 0), ear_b=(0, 2, 0))


def random_sections(K, S, seed):
    """float64[K][S][5]: stable sections (|a1| < 1 + a2, 0 < a2 < 1) with numerators of either sign -- the fold is held to the bits
    whatever the filter is."""
    rng = np.random.default_rng(seed)
    a2 = rng.uniform(0.1, 0.8, (K, S))
    a1 = rng.uniform(-0.9, 0.9, (K, S)) * (1.0 + a2)
    b = rng.standard_normal((K, S, 3))
    return np.ascontiguousarray(np.concatenate([b, a1[..., None], a2[..., None]], axis=2))


def modulation_freqs(m):
    """M frequencies over the whole range, both ends included (cycles per step)."""
    return np.array([0.013]) if m == 1 else np.linspace(0.0, 0.5, m)


def waterfall_freqs(k):
    """K frequencies in cycles per step: both ends of the range, then draws between them."""
    return ([0.0, 0.5] + [float(f) for f in np.random.default_rng(k).uniform(0.0, 0.5, max(k - 2, 0))])[:k]


def f32(value):
    """A threshold as the plan holds it."""
    return float(np.float32(value))


def by_test(**rows):
    """One row per life-cycle test, by name: a test added to TESTS is a row missing here."""
    assert tuple(rows) == TESTS, tuple(rows)
    return rows


WHOLE_RUN = dict(edges=EDGES5, threshold=None)       # None: drawn from the reference's snapshots, each kind in its own way (DRAWN)
BINS = by_test(counts=(5, 5), mid_run=(6, 5), calls=(6, 5), flag=(3, 2), rollback=(3, 2), generic=(2, 2), nothing=(4, 2), timing=(3, 8))       # (n_bins, bin_captures)
BANDS = by_test(counts=(2, 3), mid_run=(3, 4), calls=(3, 4), flag=(2, 3), rollback=(3, 4), generic=(2, 3), nothing=(3, 4), timing=(3, 4))    # sections(K, S)
MODULATION_FREQS = by_test(counts=5, mid_run=14, calls=14, flag=5, rollback=5, generic=5, nothing=14, timing=14)
WATERFALL_FREQS = by_test(counts=5, mid_run=5, calls=4, flag=3, rollback=5, generic=3, nothing=5, timing=3)
ONSETS = by_test(counts=WHOLE_RUN, mid_run=WHOLE_RUN, calls=WHOLE_RUN, flag=dict(edges=(0, 1), threshold=1e-3), rollback=dict(edges=(0, 2, 6), threshold=None),
                 generic=dict(edges=(0, 1), threshold=0.2), nothing=dict(edges=(0, 2, 4), threshold=0.3), timing=dict(edges=(0, 4, 8), threshold=1e-6))
DRAWN = {"arrival": median_threshold, "lateral": lambda snaps, plan: quantile_threshold(snaps, plan, 0.5), "arrival_bands": median_or_lower_quartile}
# a banded arrival plan's random_sections(K, S, seed), tail and lags
LAGGED = dict(sections=(3, 4, 2), tail=TAIL_W3, lag=(0, 2, 20))
ARRIVAL_BANDS = by_test(counts=LAGGED, mid_run=LAGGED, calls=LAGGED, flag=dict(sections=(2, 3, 12), tail=(2, 2, 2), lag=(0, 1)),
                        rollback=dict(sections=(2, 3, 8), tail=(3, 8, 2), lag=(0, 2)), generic=dict(sections=(2, 2, 5), tail=(2, 2, 1), lag=(0, 1)),
                        nothing=dict(sections=(3, 4, 1), tail=(2, 5, 1), lag=(0, 1, 2)), timing=dict(sections=(2, 4, 1), tail=(4, 12, 4), lag=(0, 0)))
SEAT7 = dict(edges=EDGES4, max_lag=7, threshold=ear_level, sections=SECTIONS[:2], **SEAT_EARS)
INTERAURAL = by_test(
    counts=SEAT7, mid_run=SEAT7,
    calls=dict(edges=EDGES4, max_lag=16, threshold=0.0, threshold_map=ear_map, sections=SECTIONS, **SEAT_EARS),
    flag=dict(edges=[0, 2], max_lag=3, threshold=f32(1e-6), sections=SECTIONS[:1], **SEAT_EARS),
    rollback=dict(edges=EDGES4, max_lag=6, threshold=ear_level, sections=SECTIONS[:2], ear_a=(-2, 0, 1), ear_b=(2, 0, -1)),
    generic=dict(edges=[0, 1], max_lag=2, threshold=0.0, sections=None, **SEAT_EARS),
    nothing=dict(edges=EDGES4, max_lag=8, threshold=0.0, sections=SECTIONS[:2], **SEAT_EARS),
    timing=dict(edges=[0, 8], max_lag=8, threshold=0.0, sections=SECTIONS[:2], ear_a=(0, -1, 0), ear_b=(0, 1, 0)))


def onset_details(kind, test):
    edges, threshold = ONSETS[test]["edges"], ONSETS[test]["threshold"]
    return dict(edges=list(edges), threshold=DRAWN[kind] if threshold is None else f32(threshold))


def details(kind, test):
    """What a plan of `kind` has beside its cadence in `test`."""
    bins = dict(zip(("n_bins", "bin_captures"), BINS[test]))
    if kind == "spectrum":
        return dict(freqs=FREQS5)
    if kind in ("decay", "intensity"):
        return bins
    if kind == "banded":
        return dict(bins, bands=sections(*BANDS[test]))
    if kind in ("arrival", "lateral"):
        return onset_details(kind, test)
    if kind == "modulation":
        return dict(freqs=modulation_freqs(MODULATION_FREQS[test]), bands=sections(*BANDS[test]))
    if kind == "arrival_bands":
        row = ARRIVAL_BANDS[test]
        return dict(onset_details(kind, test), bands=random_sections(*row["sections"]), tail=row["tail"], lag=list(row["lag"]))
    if kind == "waterfall":
        return dict(bins, freqs=waterfall_freqs(WATERFALL_FREQS[test]))
    return INTERAURAL[test] if kind == "interaural" else {}[kind]


# where the plans lie, per test: (the box of most kinds, the box of the kinds whose hull must stay on the grid, the box of the interaural
# plan, whose ears must)
SUB_BOX, ODD_BOX = BOXES["sub-box-630"]["box"], BOXES["sub-box-567-odd"]["box"]
PLACES = {
    "flag": (((0, 0, 6), (None, None, 1)), ((1, 1, 5), (10, 10, 1)), ((0, 2, 6), (None, 8, 1))),                 # of the 12^3 box
    "rollback": (((2, 3, 4), (12, 11, 9)),) * 3,                                                                 # of "random", strides (1, 2, 2)
    "plane": (((0, 0, 15), (None, None, 1)), ((1, 1, 15), (30, 30, 1)), None),                                   # of the 32^3 impulse room
    "generic": (((0, 0, 0), (None, None, 2)), ((1, 1, 1), (22, 18, 2)), SUB_BOX),
    "nothing": ("mesh", ((1, 1, 1), (22, 18, 26)), ((0, 2, 0), (None, 16, None))),
    "timing": ("mesh", ((1, 1, 1), (30, 30, 30)), ((0, 1, 15), (None, 30, 1))),
}


def place(kind, test):
    return PLACES[test][2 if kind == "interaural" else 1 if kind in ("intensity", "lateral") else 0]


def plan_for(kind, test, case, box, **cadence):
    return plan_on(case, kind, box=box, **dict(cadence, **details(kind, test)))


# ---- the two life-cycle tests that the kinds' own files still name ------------------------------------------------------------------------

# COUNTS / ALL_FORMS: every case of the two tests.  FILE_COUNTS / FILE_FORMS: the cases the ten kinds' own files name, under the ids they
# always had -- the files parametrise from these rows, tests/test_gpu_plan_life_cycle.py runs whatever they leave, and a kind with no
# row here gets every case there.
COUNTS = (1, 15, 16, 17, 32, 33)
FILE_COUNTS = dict({kind: (1, 16, 17, 33) for kind in ("spectrum", "decay", "banded", "intensity", "modulation", "waterfall")},
                   lateral=(15, 16, 17, 32, 33), interaural=(1, 15, 16, 17, 33))
FILE_FORMS = dict({kind: tuple(sorted(FORMS)) for kind in ("spectrum", "decay", "banded", "intensity", "arrival", "lateral", "modulation", "arrival_bands", "waterfall")},
                  interaural=tuple(sorted(ALL_FORMS)))


def outputs(eng, kind):
    """Every output of the active plan under plan_twin's names, the count first."""
    row = kind_row(kind)
    return dict(count=row.count(eng), **row.fetch(eng))


def capture_counts(kind, captures):
    """A run on "random" in f64 that takes exactly `captures` captures of the kind's plan, period 1 (the lateral plan in three-step
    passes on the odd box, one node per lane; the others in single steps with two): the count, no fold merely because the run ended
    (at most one per 16 captures before the fetch, one more for it), the CAPTURES query, and the definition's bytes over the first
    `captures` of the reference's 33 snapshots."""
    form, box = ("triple", ODD_BOX) if kind == "lateral" else ("single", SUB_BOX)
    row = kind_row(kind)
    plan = plan_for(kind, "counts", "random", box)
    snaps, steps = reference_snapshots("random", "f64", form, row.captures(plan), 32)
    plan = resolved(plan, snaps)
    want = expected(plan, snaps[:captures], steps[:captures])
    eng = plan_engine("random", "f64", form, plan)
    try:
        assert eng.run_steps(captures - 1) == (captures - 1, 0)
        assert row.count(eng) == (captures, captures - 1)
        assert eng.query(row.queries["folds"]) <= (captures - 1) // 16   # (nothing is folded merely because a run ended)
        got = outputs(eng, kind)
        assert got.get("captures", captures) == captures == eng.query(row.queries["captures"])
        assert eng.query(row.queries["folds"]) <= -(-captures // 16) + 1
    finally:
        eng.close()
    P.assert_same(got, want, (kind, captures))
    if captures == 1 and "onset" in want:
        # the threshold of these plans is drawn from all 33 snapshots of the reference (the median of the nodes' maxima) and applied
        # here to a run of ONE capture, where few nodes reach it or none: what such a run shows is an onset or, short of one, the
        # energy ahead of it
        assert row.meaningful(want, plan) or np.abs(want["pre"]).max() > 0
    else:
        assert row.meaningful(want, plan) and (kind not in ("arrival", "lateral", "arrival_bands") or heard_and_unheard(want))


def changes_nothing(kind, tag, form):
    """The case's 60 steps of "random" with the kind's plan (first_step 3, period 7, strides (1, 2, 1)) and without: receiver traces,
    final current / previous and the three filter memories equal, bytewise; the plan counted (9, 59) and holds something (every band
    of it, where it has bands)."""
    set_tuning(**ALL_FORMS[form])
    case = case_of("random")
    row = kind_row(kind)
    plan = plan_for(kind, "nothing", "random", place(kind, "nothing"), stride=(1, 2, 1), period=7, first_step=3)
    out = []
    for with_plan in (False, True):
        eng = make_engine(case, tag)
        try:
            if with_plan:
                P.set_plan(eng, plan)
            assert eng.run_steps(case["steps"]) == (case["steps"], 0)
            out.append([eng.fetch_receivers(0, case["steps"]), eng.read_field(E.BUF_CURRENT), eng.read_field(E.BUF_PREVIOUS)] +
                       [eng.read_boundary_data(d) for d in (1, 2, 3)])
            if with_plan:
                assert row.count(eng) == (9, 59)   # steps 3, 10, ..., 59
                fetched = row.fetch(eng)
                assert any(np.any(v) for v in fetched.values() if isinstance(v, np.ndarray) and v.dtype.kind in "fc")
                assert kind not in ("banded", "modulation") or row.meaningful(fetched, plan)      # every band holds something
        finally:
            eng.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert np.abs(out[0][0]).max() > 0

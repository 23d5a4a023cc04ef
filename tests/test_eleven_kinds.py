"""What tests/test_gpu_poisoned_captures.py, tests/test_gpu_newest_fold_extremes.py and tests/test_gpu_plan_handovers.py need before a
run on the GPU means anything, held on the CPU: the oracle, the shipped definitions, no engine (tests/eleven_kinds.py).  The f64 engine
is the oracle bit for bit (tests/test_gpu_fuzz.py and the plan sequences hold it to that), so the captures the conditions are asserted
on here are the ones the GPU tests see."""
import warnings

import numpy as np
import pytest

import eleven_kinds as K
import plan_twin as P
from wayverb_amd import decay as D
from wayverb_amd import simulation as W

RATE = 1000.0      # a sample rate at which a capture is a millisecond and a frequency in cycles per step is a thousandth of its hertz
TINY32 = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def eleven_kinds(built_library):
    committed = (list(P.KINDS), list(P.FAMILIES))
    with K.registered():
        assert tuple(P.KINDS) == K.KINDS11 and len(P.FAMILIES) == len(committed[1]) + 2
        yield
    assert (list(P.KINDS), list(P.FAMILIES)) == committed      # (other modules see the committed tables)


def test_registered_leaves_the_tables_as_it_found_them(built_library):
    committed = (dict(P.KINDS), dict(P.FAMILIES), P.KINDS8)
    assert "waterfall" not in P.KINDS and "interaural" not in P.KINDS
    with K.registered():
        assert tuple(P.KINDS) == K.KINDS11 and K.KINDS11[:9] == tuple(committed[0]) and K.KINDS11[9:] == ("waterfall", "interaural")
    assert (dict(P.KINDS), dict(P.FAMILIES), P.KINDS8) == committed
    with pytest.raises(RuntimeError):
        with K.registered():
            raise RuntimeError("a test failed inside")
    assert (dict(P.KINDS), dict(P.FAMILIES)) == committed[:2]


def test_the_plans_are_the_issues():
    from test_gpu_plan_extremes import BOX
    assert K.BOX == BOX == ((1, 1, 4), (10, 9, 3))
    for kind in K.KINDS11:
        plan, second = K.plan_of(kind), K.second_plan_of(kind)
        assert plan["kind"] == second["kind"] == kind and plan["box"] == BOX and plan["stride"] == (1, 1, 1) and plan["period"] == 1
        assert second["box"] != plan["box"] and (kind == "snapshots" or K.state_size(second) / np.prod(P.taken(second)) < K.state_size(plan) / np.prod(P.taken(plan)))
        hull = P.hull_of(second)[0]
        assert all(o >= 0 and o + e <= 12 for o, e in zip(*hull)) and all(o >= 0 and o + e <= 12 for o, e in zip(*P.hull_of(plan)[0]))
    assert K.plan_of("spectrum")["freqs"] == K.plan_of("waterfall")["freqs"] == K.plan_of("modulation")["freqs"] == [0.0, 0.5, 0.123, 0.31, 0.25]
    assert all((K.plan_of(k)["n_bins"], K.plan_of(k)["bin_captures"]) == (4, 5) for k in ("decay", "banded", "intensity", "waterfall"))
    assert all(K.plan_of(k)["edges"] == [0, 1, 5, 16] for k in K.ONSET_KINDS)
    bands = K.plan_of("arrival_bands")
    assert bands["bands"].shape == (2, 4, 5) and bands["lag"] == [0, 3] and bands["tail"] == (3, 17, 1)
    ears = K.plan_of("interaural")
    assert (ears["ear_a"], ears["ear_b"], ears["max_lag"]) == ((-1, 0, 1), (1, -1, 0), 5) and ears["sections"].shape == (4, 5)
    plain = K.plan_of("interaural", **K.UNFILTERED)
    assert plain["max_lag"] == 16 and plain["sections"] is None and plain["ear_a"] == (-1, 0, 1)


def test_the_life_cycle_columns_are_there_for_every_kind_and_name_what_the_engine_has(eleven_kinds):
    """tests/plan_cases.py COLUMNS beside plan_twin.KINDS: every accumulating kind has every column, the query constants are
    Engine's own (three per kind, five where the kind gathers, the two decay kinds sharing theirs), the refusal sentences are the ones
    the library's sources and tests/golden/arrival_bands_refusals.json spell, and a plan written by plan_on is plan_twin's."""
    import json
    import os
    import re
    import plan_cases as C
    from wayverb_amd import engine as E
    assert tuple(C.COLUMNS) == tuple(k for k in K.KINDS11 if k != "snapshots")
    constants = {name: getattr(E.Engine, name) for name in dir(E.Engine) if name.startswith("QUERY_")}
    used = []
    for kind, column in C.COLUMNS.items():
        row = C.kind_row(kind)
        assert all(hasattr(row, name) for name in C.COLUMN_NAMES + ("set", "stop", "count", "fetch", "expect", "something", "hull", "setter", "active")), kind
        assert tuple(column.queries)[:3] == ("captures", "folds", "ns") and len(column.queries) in (3, 5), kind
        prefix = {name[:-len("_CAPTURES")] for name, value in constants.items() if value == column.queries["captures"] and name.endswith("_CAPTURES")}
        assert len(prefix) == 1, kind
        for name, value in column.queries.items():
            assert constants[prefix.copy().pop() + "_" + name.upper()] == value, (kind, name)
        assert ("gathers" in column.queries) == (prefix.copy().pop() + "_GATHERS" in constants), kind
        used.append(tuple(column.queries.values()))
        assert re.fullmatch(r"wv_rollback: the [a-z ]+ plan was set after the checkpoint \(its (sums|bins|state) ha(ve|s) no copy to go back to\)", column.rollback), kind
        assert sorted(column.no_plan) == ["count", "fetch"] and all(re.fullmatch(r"wv_\w+: no [a-z ]+ plan is set", s) for s in column.no_plan.values()), kind
        assert hasattr(E.Engine, "set_" + column.answer[0][:-len("_shape")]) and callable(column.meaningful) and callable(column.spread) and callable(column.captures)
    assert len(set(used)) == 9 and used[1] == used[2]         # decay and banded decay: one plan in the engine, one set of counters
    source = "".join(open(os.path.join(os.path.dirname(E.__file__), "csrc", name)).read() for name in ("engine.hip.h", "engine_staged.hip.h", "engine_io.hip.h"))
    for kind, column in C.COLUMNS.items():        # the sentences are put together from StagedPlan's name and `lost`
        name, lost = re.fullmatch(r"wv_rollback: the (.+) plan was set after the checkpoint \((.+) no copy to go back to\)", column.rollback).groups()
        assert '"%s", "%s", "%s"' % (name, P.KINDS["decay" if kind == "banded" else kind].setter, lost) in source, kind
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arrival_bands_refusals.json")))
    bands = C.COLUMNS["arrival_bands"]
    assert golden["rollback"] == [-6, bands.rollback]
    assert golden["no_plan"] == dict(arrival_bands_count=[-6, bands.no_plan["count"]], fetch_arrival_bands=[-6, bands.no_plan["fetch"]])
    plan = C.plan_on("random", "interaural", box=((0, 2, 0), (None, 16, None)), stride=3, period=7, threshold=0.0, ear_a=(0, -2, 0), ear_b=(0, 2, 0))
    assert plan["box"] == ((0, 2, 0), (24, 16, 28)) and plan["stride"] == (3, 3, 3) and plan["first_step"] == 0 and plan["threshold_map"] is None
    assert P.taken(plan) == (8, 6, 10) and C.whole_mesh(plan) == dict(box="mesh", first_step=0, period=7)
    hull = C.plan_on((24, 20, 28), "lateral", box=((3, 2, 4), (9, 9, 7)), threshold=0.5)
    assert C.captured_by(hull) == dict(box=((2, 1, 3), (11, 11, 9)), stride=(1, 1, 1), first_step=0, period=1) == dict(C.hull_of(hull)[0], stride=(1, 1, 1), first_step=0)
    assert C.resolved(dict(hull, threshold=lambda snaps, plan: snaps + plan["period"]), 2)["threshold"] == 3


def front_form(plan):
    """(the kind's *_plan_arguments applied to the plan written as canonical's dict at RATE, the keys of the answer that must be the
    plan's own) -- or None for a kind that has no such function (snapshots and the two decay plans go to the engine as they are)."""
    kind = plan["kind"]
    mesh = K.poison_case()["mesh"]
    common = dict(box=plan["box"], stride=plan["stride"], first_step=plan["first_step"])
    ms = lambda edges: tuple(float(e) for e in edges[1:])
    hz = lambda bands_of: [(lo * RATE, hi * RATE) for lo, hi in bands_of]
    first = "bands" in plan and plan["bands"].shape[0] == 2
    octaves = D.octave_band_edges([0.1, 0.2] if first else [0.1])
    freqs_hz = [f * RATE for f in plan.get("freqs", [])]
    if kind == "spectrum":
        return W.spectrum_plan_arguments(dict(common, freqs_hz=freqs_hz, period=1), RATE), ("freqs", "box", "stride", "first_step", "period")
    if kind == "intensity":
        out = W.intensity_plan_arguments(dict(common, n_bins=plan["n_bins"], bin_seconds=plan["bin_captures"] / RATE), mesh, RATE, W.Environment(), 0.06)
        return out, ("n_bins", "bin_captures", "box", "stride", "first_step", "period")
    if kind == "arrival":
        out = W.arrival_plan_arguments(dict(common, threshold=plan["threshold"], early_ms=ms(plan["edges"])), mesh, RATE)
        return out, ("edges", "threshold", "threshold_map", "box", "stride", "first_step", "period")
    if kind == "arrival_bands":      # (the front's lags are the bands' group delays or 0: the plan's own lags go to the engine as they are)
        tail = dict(tail_ms=float(plan["tail"][1] + plan["tail"][0] * plan["tail"][2]), tail_bin_ms=float(plan["tail"][2])) if plan["tail"] else {}
        out = W.arrival_bands_plan_arguments(dict(common, threshold=plan["threshold"], early_ms=ms(plan["edges"]), bands=hz(octaves), lag=0, **tail), mesh, RATE)
        return out, ("edges", "bands", "tail", "threshold", "threshold_map", "box", "stride", "first_step", "period")
    if kind == "lateral":
        out = W.lateral_plan_arguments(dict(common, threshold=plan["threshold"], edges_ms=(0.0,) + ms(plan["edges"])), mesh, RATE, W.Environment())
        return out, ("edges", "threshold", "threshold_map", "box", "stride", "first_step", "period")
    if kind == "modulation":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (an octave that reaches above a quarter of the sample rate is warned about)
            out = W.modulation_plan_arguments(dict(common, bands_hz=[100.0, 200.0] if first else [100.0], freqs_hz=freqs_hz), mesh, RATE)
        return out, ("freqs", "bands", "box", "stride", "first_step", "period")
    if kind == "waterfall":
        out = W.waterfall_plan_arguments(dict(common, freqs_hz=freqs_hz, n_bins=plan["n_bins"], bin_captures=plan["bin_captures"]), mesh, RATE)
        return out, ("freqs", "n_bins", "bin_captures", "box", "stride", "first_step", "period")
    if kind == "interaural":
        band = None
        if plan["sections"] is not None:
            assert plan["sections"].shape[0] in (2, 4)
            band = hz(D.octave_band_edges([0.1]))[0] if plan["sections"].shape[0] == 4 else None      # (the second plan's half cascade is no design of the front's)
        out = W.interaural_plan_arguments(dict(common, threshold=plan["threshold"], edges_ms=(0.0,) + ms(plan["edges"]), ears=(plan["ear_a"], plan["ear_b"]),
                                               max_lag_ms=float(plan["max_lag"]), band_hz=band), mesh, RATE)
        return out, ("edges", "ear_a", "ear_b", "max_lag", "threshold", "threshold_map", "box", "stride", "first_step", "period") + (("sections",) if band or plan["sections"] is None else ())
    return None


@pytest.mark.parametrize("kind", K.KINDS11 + ("interaural-unfiltered",))
def test_the_front_accepts_every_plan_and_makes_it_of_its_canonical_form(built_library, kind):
    """Every plan_of and every second plan, written as canonical's dict at a rate of 1000 (a capture a millisecond), goes through the
    kind's *_plan_arguments and comes back as itself: integers and boxes equal, designs and frequencies to rounding."""
    over = K.UNFILTERED if kind.endswith("unfiltered") else {}
    for plan in (K.plan_of(kind.split("-")[0], **over), K.second_plan_of(kind.split("-")[0])):
        form = front_form(plan)
        if form is None:
            assert plan["kind"] in ("snapshots", "decay", "banded")
            continue
        out, keys = form
        for key in keys:
            if isinstance(plan[key], np.ndarray) or key == "freqs":
                np.testing.assert_allclose(np.asarray(out[key], dtype=np.float64), np.asarray(plan[key], dtype=np.float64), rtol=1e-9, atol=1e-15, err_msg=key)
            else:
                assert out[key] == plan[key], (key, out[key], plan[key])


# ---- section 1 --------------------------------------------------------------------------------------------------------------------

POISON_CASES = [(kind, {}) for kind in K.KINDS11] + [("interaural", K.UNFILTERED)]


@pytest.mark.parametrize("poison_capture", [K.POISON_STEP, 0])
@pytest.mark.parametrize("kind,over", POISON_CASES, ids=list(K.KINDS11) + ["interaural-unfiltered"])
def test_the_poisoned_captures_hold_what_the_comparison_needs(oracle, eleven_kinds, kind, over, poison_capture):
    """On the captures of the sequence itself, from the oracle: the poison is in the capture it was written for and nowhere else, and the
    definitions' outputs hold eleven_kinds.assert_poison_conditions -- fewer than 15 % NaNs, something bad and something finite in every
    output that can go bad, the onset rules, the poison carried across the fold by the interaural history."""
    plan = K.plan_of(kind, **dict(dict(threshold=K.THRESHOLD) if kind in K.ONSET_KINDS else {}, **over))
    steps, snaps, nodes = K.twin_captures(oracle, plan, poison_capture)
    dims = K.poison_case()["mesh"].dims
    nan_at, plus_at, minus_at = K.in_capture(nodes, P.capture_box(plan), dims)
    bad = snaps[poison_capture]
    assert np.array_equal(np.isnan(bad), nan_at) and np.array_equal(bad == np.inf, plus_at) and np.array_equal(bad == -np.inf, minus_at)
    assert nan_at.sum() == plus_at.sum() == minus_at.sum() == 5 and np.isfinite(np.delete(snaps, poison_capture, axis=0)).all()
    if kind in K.ONSET_KINDS and poison_capture:      # the start stays under the threshold: no onset ahead of the poison but an infinite one
        assert np.abs(snaps[:poison_capture]).max() < K.THRESHOLD
    twin = P.PlanTwin(None, K.poison_case()["mesh"], np.float64)
    twin.set_plan(plan)
    twin.log = [(int(s), a) for s, a in zip(steps, snaps)]
    with np.errstate(all="ignore"):
        want = twin.expected()
    assert want["count"][0] == K.LAST_STEP + 1
    K.assert_poison_conditions(plan, want, snaps, K.in_capture(nodes, plan, dims), poison_capture)
    K.assert_outputs_but_nan_bytes({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}, want, kind)


def test_the_comparison_tells_a_nan_from_a_number_and_an_infinity_from_its_negative():
    want = dict(count=(2, 1), bins=np.array([1.0, np.nan, np.inf, -0.0]), sums=np.array([1 + 2j, complex(np.nan, 3.0)]))
    flipped = np.array([1.0, -np.nan, np.inf, -0.0])
    K.assert_outputs_but_nan_bytes(dict(want, bins=flipped), want, "the sign of a NaN")
    for bins in ([1.0, 2.0, np.inf, -0.0], [np.nan, np.nan, np.inf, -0.0], [1.0, np.nan, -np.inf, -0.0], [1.0, np.nan, np.inf, 0.0]):
        with pytest.raises(AssertionError):
            K.assert_outputs_but_nan_bytes(dict(want, bins=np.array(bins)), want, bins)
    for sums in ([1 + 2j, complex(np.nan, 4.0)], [1 + 2j, complex(1.0, 3.0)], [1 + 2j, complex(np.nan, np.nan)]):
        with pytest.raises(AssertionError):
            K.assert_outputs_but_nan_bytes(dict(want, sums=np.array(sums)), want, sums)
    with pytest.raises(AssertionError):
        K.assert_outputs_but_nan_bytes(dict(want, count=(2, 2)), want, "count")


# ---- section 2 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1e-41, 1e30])
@pytest.mark.parametrize("name,with_map", K.EXTREME_CASES, ids=["%s%s" % (n, "-map" if m else "") for n, m in K.EXTREME_CASES])
def test_the_extreme_captures_hold_what_the_comparison_needs(oracle, eleven_kinds, name, with_map, scale):
    """With the real sections (test_gpu_plan_extremes.scaled_bands) and the library's twiddle: the three definitions are finite and not
    all zeros at both scales; at 1e-41 more than half the captures, every threshold of a map and more than half of the first section's
    states are subnormal; at 1e30 the placed negative zeros are the only ones; a map gives nodes with an onset, nodes without, and three
    distinct onsets."""
    plan = K.extreme_plan(name, scale, with_map)
    steps, snaps, placed = K.extreme_captures(oracle, plan, scale)
    assert len(steps) == 21 and np.isfinite(snaps).all()
    if scale < 1:
        assert ((snaps != 0) & (np.abs(snaps) < TINY32)).mean() > 0.5
        if with_map:
            assert ((plan["threshold_map"] != 0) & (plan["threshold_map"] < TINY32)).all()
    else:
        assert placed.sum() >= 10 and np.array_equal(np.signbit(snaps[0]) & (snaps[0] == 0), placed) and np.abs(snaps).max() > 1e29
    twin = P.PlanTwin(None, K.poison_case()["mesh"], np.float64)
    twin.set_plan(plan)
    twin.log = [(int(s), a) for s, a in zip(steps, snaps)]
    with np.errstate(under="ignore"):
        want = twin.expected()
    K.assert_extreme_conditions(name, plan, scale, want, snaps)
    if with_map:
        heard = want["onset"] != 0xFFFFFFFF
        print(name, scale, "onsets at %.0f %% of the nodes, at %d distinct captures" % (100 * heard.mean(), len(np.unique(want["onset"][heard]))))


# ---- section 3 --------------------------------------------------------------------------------------------------------------------

def test_every_handover_script_holds_what_the_replay_needs(oracle, eleven_kinds):
    """The script of every one of the 121 pairs, on the twin alone: both plans have captures (a: one fold of 16 and more staged); b
    folds before its checkpoint (which folds what is staged: 8 captures; a snapshot plan folds nothing and was rolled back to none)
    and after it (19 captures from 8: the stage fills at 16); neither plan's outputs are all zeros; of the kinds with an onset, b has
    nodes that heard one in every pair."""
    seen = set()
    unheard = 0
    for i, a in enumerate(K.KINDS11):
        for j, b in enumerate(K.KINDS11):
            script, held = K.handover_script(oracle, a, b, f32=(i + j) % 2 == 1)
            seen.add((a, b, script["tag"]))
            assert script["tag"] == ("f32" if (i + j) % 2 else "f64") and max(op.get("n", 0) for op in script["ops"]) <= 21
            assert script["final"]["step_no"] <= 60 and len(script["final"]["rows"]) == script["final"]["step_no"]
            assert held["a_captures"] == 27 > 16
            assert (held["b_before"], held["b_after"]) == ((0, 15) if b == "snapshots" else (8, 19)), (a, b, held)
            names = [op["op"] for op in script["ops"]]
            assert names.count("checkpoint") == 2 and names.count("rollback") == (2 if b == "snapshots" else 1)
            assert names.count("refused-rollback") == (0 if b == "snapshots" else 1) and names.count("refused-plan") == (0 if a == b else 1)
            assert names.count("same") == (1 if a == b else 0) and names.count("stop") == (1 if a == b else 2)
            wants = [op["want"] for op in script["ops"] if op.get("want") is not None]
            for want in (wants[0], wants[-1]):      # a's outputs at the handover, b's at its stop
                assert any(np.any(v != 0) for v in K.float_outputs(want).values()), (a, b)
            if b in K.ONSET_KINDS:
                onset = wants[-1]["onset"]
                assert (onset != 0xFFFFFFFF).any(), (a, b)
                unheard += int((onset == 0xFFFFFFFF).any())
    assert len(seen) == 121 and sum(1 for s in seen if s[2] == "f32") == 60
    assert unheard >= 22, unheard      # of the 44 pairs whose b has an onset: nodes without one too, in half of them at the least

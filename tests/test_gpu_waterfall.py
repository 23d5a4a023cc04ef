"""Waterfall maps: per time bin, the Fourier sums of a box of the field accumulated on the device while wv_run keeps going
(wv_set_waterfall; csrc/waterfall_kernels.hip.h, engine_waterfall.hip.h).  The reference of every comparison is a second, identical
engine with a SNAPSHOT plan of the same box and cadence, whose snapshots go through waterfall.waterfall_fold -- `a + p * c` on float64
arrays in capture order, which is the definition.  Equality is BYTEWISE, and every comparison also asserts that it is not one of zeros.
Small meshes, forms forced, a few dozen steps."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import plan_argument_faults as F
import plan_twin as P
import waterfall_twin as T
from helpers import numpy_fold, set_tuning
from plan_cases import (BOXES, FILE_COUNTS, FILE_FORMS, FORM_CASES, LAYOUTS, box_scene, capture_counts, changes_nothing, check,
                        default_tuning_afterwards, make_engine, plan_engine, plan_on, reference_snapshots)
from test_gpu_plan_refusals import BANDS, SET, STOP, refusal
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd import waterfall as WF
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB_BOX = dict(box=((3, 2, 4), (10, 9, 7)), period=1)      # BOXES["sub-box-630"], every step


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def freqs_of(k):
    """K frequencies in cycles per step: both ends of the range, then draws between them."""
    return ([0.0, 0.5] + [float(f) for f in np.random.default_rng(k).uniform(0.0, 0.5, max(k - 2, 0))])[:k]


def waterfall_plan(case, cadence, freqs, n_bins, bin_captures):
    return plan_on(case, "waterfall", freqs=freqs, n_bins=n_bins, bin_captures=bin_captures, **cadence)


def nonzero(bins):
    """Not a comparison of zeros: something in the real parts, and in the imaginary ones wherever a frequency has any."""
    return bool(np.abs(bins.real).max() > 0)


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_sums_of_the_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes, periods that do and do not divide 2 and 3: one plane of the 32^3 impulse
    room, K = 3, four captures per bin."""
    n_steps = 64 if form == "graph" else 30
    captures = n_steps // period + 1
    check("waterfall", "impulse_flat", tag, form, waterfall_plan("impulse_flat", dict(box=((0, 0, 15), (None, None, 1)), period=period), freqs_of(3), -(-captures // 4), 4), n_steps, query)


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; every step captured, 21 captures (more
    than the stage holds), K = 5, 7 bins of 3."""
    check("waterfall", "random", tag, "triple", waterfall_plan("random", dict(BOXES[name], period=1), freqs_of(5), 7, 3), 20)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 9, 64])
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_numbers_of_frequencies_around_the_chunk_in_both_lane_widths(name, k):
    """K below, at and above the fold's chunk of four, a chunk with a tail, and the most there is; B even (two nodes per lane) and odd
    (one): 33 captures into 4 bins of 5, the last open-ended."""
    check("waterfall", "random", "f64", "pair", waterfall_plan("random", dict(BOXES[name], period=1), freqs_of(k), 4, 5), 32)


LAYOUT_CASES = [(layout, k) for layout in sorted(LAYOUTS) for k in (1, 5) if LAYOUTS[layout][0] * k <= 4096]


@pytest.mark.parametrize("layout,k", LAYOUT_CASES, ids=["%s-K%d" % c for c in LAYOUT_CASES])
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_bin_layouts_against_the_stage(name, layout, k):
    """test_gpu_decay.py's eight layouts of bins against the 16-slot stage, 33 captures (16 + 16 + 1 for the fetch): every capture a new
    bin, edges inside and across folds, whole folds inside one bin, one bin, the open-ended last bin.  4096 bins are more than the cap
    on sums allows at K = 5: that layout runs at K = 1, where the bins no capture reached must be +0.0 with the sign bit clear."""
    n_bins, bin_captures = LAYOUTS[layout]
    got = check("waterfall", "random", "f64", "pair", waterfall_plan("random", dict(BOXES[name], period=1), freqs_of(k), n_bins, bin_captures), 32)[0]["waterfall"]
    if layout == "more-bins-than-captures":
        untouched = np.stack([got[33:].real, got[33:].imag])
        assert k == 1 and (untouched == 0).all() and not np.signbit(untouched).any()
    assert ("more-bins-than-captures", 1) in LAYOUT_CASES and len(LAYOUT_CASES) == 15


@pytest.mark.parametrize("k", [1, 5])
def test_one_bin_is_the_spectrum_plan_bytewise(k):
    """n_bins = 1: the bytes of fetch_spectrum of an identical engine (and of the spectrum's definition, helpers.numpy_fold)."""
    freqs = freqs_of(k)
    eng = plan_engine("random", "f64", "triple", waterfall_plan("random", SUB_BOX, freqs, 1, 3))
    other = make_engine(cases.CASES["random"](), "f64")
    other.set_spectrum(freqs, **SUB_BOX)
    try:
        for e in (eng, other):
            assert e.run_steps(20) == (20, 0)
        got, count = eng.fetch_waterfall()
        spectrum, spectrum_count = other.fetch_spectrum()
    finally:
        eng.close()
        other.close()
    snaps, steps = reference_snapshots("random", "f64", "triple", SUB_BOX, 20)
    assert count == spectrum_count == 21 and got.shape == (1,) + spectrum.shape
    assert got[0].tobytes() == spectrum.tobytes() == numpy_fold(snaps, steps, freqs).tobytes() and nonzero(got)


# ---- refusals: the 12 x 10 x 9 fp32 box mesh of tests/plan_argument_faults.py, no stepping ------------------------------------------

WF_BASE = dict(F.BOX, n_freqs=2, n_bins=3, bin_captures=2, freqs=[0.0, 0.125])
WF_FAULTS = dict(F.SHARED, **F.FREQS, **F.BINS, **{"n_freqs 0": F.put(n_freqs=0), "n_freqs 65": F.put(n_freqs=65),
                                                  "product 2 x 2049": F.put(n_bins=2049)})
INVALID = -1


def expected_refusal(a):
    """[code, sentence] by the order the issue sets for wv_set_waterfall's checks, restated: n_freqs, NULL frequencies, each frequency,
    n_bins, bin_captures, the product cap, then the shared strides / period / box; None for a plan that is taken."""
    def says(text):
        return [INVALID, text if text == "null argument" else "wv_set_waterfall: " + text]
    if not 1 <= a["n_freqs"] <= 64:
        return says("n_freqs must be 1 .. 64")
    if a["freqs"] is None:
        return says("null argument")
    if any(not 0.0 <= f <= 0.5 for f in a["freqs"][:a["n_freqs"]]):
        return says("a frequency outside [0, 0.5] cycles per step")
    if not 1 <= a["n_bins"] <= 4096:
        return says("n_bins must be 1 .. 4096")
    if a["bin_captures"] < 1:
        return says("bin_captures must be >= 1")
    if a["n_freqs"] * a["n_bins"] > 4096:
        return says("n_freqs * n_bins must be <= 4096 (64 KiB of sums per node)")
    if min(a["sx"], a["sy"], a["sz"]) < 1:
        return says("strides must be >= 1")
    if a["period"] < 1:
        return says("period must be >= 1")
    for o, n, s, d in zip((a["x0"], a["y0"], a["z0"]), (a["nx"], a["ny"], a["nz"]), (a["sx"], a["sy"], a["sz"]), F.MESH):
        if n < 1 or o < 0 or o + (n - 1) * s >= d:
            return says("the box leaves the mesh")
    return None


def call_setter(eng, args):
    plan = E.WvWaterfallPlan()
    for name, _ in plan._fields_:
        if name in args:
            setattr(plan, name, args[name])
    freqs = None if args["freqs"] is None else np.ascontiguousarray(args["freqs"], dtype=np.float64)
    rc = eng.lib.wv_set_waterfall(eng.h, C.byref(plan), F.pointer(freqs))
    return None if rc == 0 else [rc, eng.lib.wv_last_error().decode()]


@pytest.fixture(scope="module")
def fault_engine(built_library):
    eng = F.make_engine()
    yield eng
    eng.close()


def test_every_argument_fault_and_every_ordered_pair_with_code_and_sentence(fault_engine):
    """Every single fault and every ordered pair of two (the second wins where both touch one argument): the code and the WHOLE
    sentence, by the precedence the checks have; the engine is untouched by every refused call, and an earlier plan's sums are."""
    eng = fault_engine
    # (the valid plan goes through the Python layer, which remembers the shape its fetch allocates; the faulty ones go to the library itself)
    assert eng.set_waterfall(WF_BASE["freqs"], WF_BASE["n_bins"], WF_BASE["bin_captures"], box=((1, 1, 1), (4, 3, 2))) == (3, 2, 2, 3, 4)
    assert eng.run_steps(3) == (3, 0)
    kept, kept_count = eng.fetch_waterfall()
    before = F.state(eng)
    said = set()
    names = list(WF_FAULTS)
    for first in names:
        for second in names:
            args = dict(WF_BASE)
            for name in ([first] if first == second else [first, second]):
                WF_FAULTS[name](args)
            want = expected_refusal(args)
            got = call_setter(eng, args)
            assert want is not None, (first, second)      # (no two of these faults undo each other: every case is a refusal)
            assert got == want, (first, second, got, want)
            said.add(want[1])
            assert F.state(eng) == before, (first, second)
            again, count = eng.fetch_waterfall()
            assert count == kept_count == 4 and again.tobytes() == kept.tobytes(), (first, second)
    assert nonzero(kept) and len(names) == 21 and expected_refusal(dict(WF_BASE)) is None
    assert len(said) == 9       # every sentence the setter has for an argument was said
    eng.set_waterfall(None, None, None)


def test_the_cap_on_sums_per_node(fault_engine):
    """(65, 64) and (64, 65) for (K, n_bins) are refused -- the first for K, the second for the product -- while (64, 64) is taken."""
    eng = fault_engine
    box = dict(box=((1, 1, 1), (4, 3, 2)))
    f = list(np.linspace(0.0, 0.5, 65))
    assert refusal(lambda e: e.set_waterfall(f, 64, 1, **box), eng) == [INVALID, "wv_set_waterfall: n_freqs must be 1 .. 64"]
    assert refusal(lambda e: e.set_waterfall(f[:64], 65, 1, **box), eng) == [INVALID, "wv_set_waterfall: n_freqs * n_bins must be <= 4096 (64 KiB of sums per node)"]
    assert eng.set_waterfall(f[:64], 64, 1, **box) == (64, 64, 2, 3, 4)
    got, count = eng.fetch_waterfall()
    assert got.shape == (64, 64, 2, 3, 4) and count == 0 and not got.any()
    eng.set_waterfall(None, None, None)


NINE = dict(SET, modulation=lambda e: e.set_modulation([0.0, 0.125], BANDS, box=((1, 1, 1), (4, 3, 2))),
            arrival_bands=lambda e: e.set_arrival_bands((0, 4), BANDS, 1e-3, box=((1, 1, 1), (4, 3, 2))))
NINE_STOP = dict(STOP, modulation=lambda e: e.set_modulation(None, None), arrival_bands=lambda e: e.set_arrival_bands(None, None))
TWIN_KIND = dict(decay_bands="banded")       # test_gpu_plan_refusals.py's names -> plan_twin's


def test_the_plan_excludes_each_of_the_nine_others_in_both_directions(fault_engine):
    """Under a waterfall plan every existing setter says the new row's sentence; under each existing plan the new setter says that
    plan's row.  WV_E_STATE throughout, and the refused call changes nothing: the active plan is still the one its count answers for."""
    eng = fault_engine
    assert sorted(NINE) == sorted(["snapshots", "spectrum", "decay", "decay_bands", "intensity", "arrival", "lateral", "modulation", "arrival_bands"])
    set_waterfall = lambda e: e.set_waterfall([0.0, 0.125], 3, 2, box=((1, 1, 1), (4, 3, 2)))       # noqa: E731
    set_waterfall(eng)
    for kind, setter in NINE.items():
        entry = P.KINDS[TWIN_KIND.get(kind, kind)]
        assert refusal(setter, eng) == [-6, entry.setter + ": a waterfall plan is active (wv_set_waterfall(e, NULL, NULL) stops it); the plans exclude each other"], kind
        assert eng.waterfall_count() == (0, 0)
    eng.set_waterfall(None, None, None)
    for kind, setter in NINE.items():
        entry = P.KINDS[TWIN_KIND.get(kind, kind)]
        setter(eng)
        assert refusal(set_waterfall, eng) == [-6, "wv_set_waterfall: " + entry.active + P.TAIL], kind
        assert refusal(lambda e: e.waterfall_count(), eng) == [-6, "wv_waterfall_count: no waterfall plan is set"]
        NINE_STOP[kind](eng)
        set_waterfall(eng)      # with the plan stopped the setter that was refused goes through
        eng.set_waterfall(None, None, None)
    # a plan set after the checkpoint has nothing to roll back to
    eng.checkpoint()
    set_waterfall(eng)
    code, text = refusal(lambda e: e.rollback(), eng)
    assert code == -6 and "waterfall plan was set after the checkpoint" in text and "its sums have" in text
    eng.set_waterfall(None, None, None)
    eng.rollback()
    eng.drop_checkpoint()


def test_a_slab_of_a_chain_and_a_group_refuse():
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    assert refusal(lambda e: e.set_waterfall([0.1], 2, 2, box=((0, 0, 0), (4, 4, 1))), slab) == [-6, "wv_set_waterfall: not on a slab of a chain (one domain only)"]
    slab.close()
    eng = E.Engine(mesh, precision="f32")
    group = E.LocalSlabGroup([eng])
    eng.set_waterfall([0.1], 2, 2, box=((0, 0, 0), (4, 4, 1)))
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_run_group accumulates no waterfall maps: .*\(wv_set_waterfall\(e, NULL, NULL\) stops the plan\)"):
        group.run_steps(4)
    eng.set_waterfall(None, None, None)
    assert group.run_steps(4) == (4, 0)
    group.close()


# ---- the family's scripts, replayed -----------------------------------------------------------------------------------------------------

MODES = {"default": {}, "three-step-passes": dict(pair=1, triple=1), "single-steps": dict(pair=0)}
_script = {}


@pytest.fixture(scope="module", autouse=True)
def waterfall_family():
    """(for the whole module: the shared check reads the kind's entry too)"""
    with T.registered():
        yield


@pytest.mark.parametrize("seed", range(T.SEEDS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_random_plan_sequence(oracle, waterfall_family, seed, mode):
    """The eight scripts tests/test_waterfall_twin.py holds to what the comparison needs, through plan_twin.replay: after every call
    both fields, at every fetch, handover, stop and the end every output of the plan, bytewise."""
    if seed not in _script:
        _script[seed] = P.build_script(oracle, T.FAMILY, seed)
    script = _script[seed]
    set_tuning(**MODES[mode])
    eng = E.Engine(script["mesh"], precision=script["tag"], all_tiles=False)
    try:
        P.replay(eng, script)
    finally:
        eng.close()


# ---- the Python front and the tools -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("captures", FILE_COUNTS["waterfall"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("waterfall", captures)


@pytest.mark.parametrize("form", FILE_FORMS["waterfall"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("waterfall", tag, form)


def test_canonical_returns_the_bins_beside_the_receiver_output():
    """simulation.canonical(..., waterfall=...): the records are those of a run without a plan, the bins are the engine-level ones
    (folded from canonical's own snapshots of the same box and cadence); a second plan beside it is refused with the engine's message."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    z = 12 * vm.mesh.spacing
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=dict(box=((0, 0, 12), (None, None, 1)), period=2))
    hz = [0.0, rate / 40.0, rate / 8.0]
    bands, (bins, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                          waterfall=dict(freqs_hz=hz, plane=z, every=2, n_bins=5, bin_captures=4))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 21 and bins.shape == (5, 3, 1, 24, 24)
    assert bins.tobytes() == WF.waterfall_fold(fields, steps, np.asarray(hz) / rate, 5, 4).tobytes() and nonzero(bins)
    maps = WF.waterfall_maps(bins[:, :, 0], 4, 2, rate)
    assert maps["csd_db"].shape == (5, 3, 24, 24) and maps["decay_s"].shape == (3, 24, 24) and maps["times_s"].shape == (5,)
    with pytest.raises(E.WaveguideError, match="error -6: wv_set_waterfall: a decay plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, decay=dict(n_bins=2, bin_captures=2), waterfall=dict(freqs_hz=hz, plane=z, bin_ms=1.0))
    with pytest.raises(ValueError, match="waterfall sums are accumulated on one domain only"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, waterfall=dict(freqs_hz=hz, plane=z, bin_ms=1.0))


def test_the_tool_writes_the_waterfall_of_one_plane(tmp_path):
    """tools/waterfall_map.py on a 24^3 room: the complex bins, the CSD level and the modal decay times of one plane."""
    out = tmp_path / "waterfall.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "waterfall_map.py"), "--room", "24", "--seconds", "0.05", "--precision", "f32",
                        "--freqs", "40,80,120", "--plane", "z=1.5", "--every", "2", "--bin-ms", "4", "--out", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        bins, csd, decay, captures = f["bins"], f["csd_db"], f["decay_s"], int(f["captures"])
        per_bin, period, rate, freqs, times = int(f["bin_captures"]), int(f["period"]), float(f["sample_rate"]), f["freqs_hz"], f["times_s"]
    assert "wrote" in p.stdout and bins.dtype == np.complex128 and bins.ndim == 4 and bins.shape[1] == 3 and bins.shape[2:] == (24, 24)
    assert period == 2 and per_bin == max(1, int(round(0.004 * rate / 2))) and list(freqs) == [40.0, 80.0, 120.0]
    assert bins.shape[0] == max(1, min(-(-captures // per_bin), 4096 // 3)) == times.shape[0]
    assert csd.shape == bins.shape and decay.shape == bins.shape[1:] and nonzero(bins) and (csd[0][np.isfinite(csd[0])] == 0).all()


def test_the_rate_tool_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/waterfall_rate.py --side 64 --steps 48: every row is there and the sums of the snapshot-and-host way equal the plan's
    bytewise in both cases."""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "waterfall_rate.py"), "--side", "64", "--steps", "48",
                        "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 2, p.stdout
    report = json.load(open(str(out)))
    assert len(report["cases"]) == 2 and all(c["bytewise_equal"] and c["not_zeros"] for c in report["cases"].values())
    assert all(set(c["steps_per_second"]) == {"no plan", "snapshots + numpy", "waterfall plan"} for c in report["cases"].values())

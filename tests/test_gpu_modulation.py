"""Modulation maps: per band the energy of the filtered captures and the Fourier sums of their squares at modulation frequencies, on
the device while wv_run keeps going (wv_set_modulation; csrc/modulation_kernels.hip.h, engine_modulation.hip.h).  The reference of
every comparison is a second, identical engine with a SNAPSHOT plan of the same box and cadence, pushed through
modulation.modulation_fold -- the definition evaluated on float64 arrays, one rounding per operation, with the twiddles of
engine.spectrum_twiddle.  Equality is BYTEWISE, and every comparison asserts that it is not one of zeros.  Small meshes, forms
forced, a few dozen steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import set_tuning
from plan_cases import (BOXES, FILE_COUNTS, FILE_FORMS, FORMS, box_scene, capture_counts, changes_nothing, check, default_tuning_afterwards,
                        make_engine, plan_engine, plan_on, reference_snapshots, sections)
from plan_cases import every_band_and_frequency as not_zeros
from test_gpu_plan_refusals import KINDS, SET, STOP, refusal
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd import modulation as MOD
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]]])
SENTENCE = "a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it); the plans exclude each other"


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def freqs(m):
    """M frequencies over the whole range, both ends included (cycles per step)."""
    return np.array([0.013]) if m == 1 else np.linspace(0.0, 0.5, m)


def modulation_plan(case, cadence, bands, f):
    return plan_on(case, "modulation", freqs=f, bands=bands, **cadence)


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


FORM_CASES = [(form, period, {("pair", 3): E.Engine.QUERY_PASSES, ("pair", 7): E.Engine.QUERY_PASSES, ("triple", 3): E.Engine.QUERY_TRIPLE_PASSES,
                              ("triple", 7): E.Engine.QUERY_TRIPLE_PASSES}.get((form, period)))
              for form in ("single", "graph", "pair", "triple") for period in (1, 3, 7)]


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_sums_of_the_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes; period 1 (every step ends a pass), 3 (three-step passes stay whole) and 7;
    one plane of the 32^3 impulse room, three bands of four sections, five modulation frequencies."""
    n_steps = 64 if form == "graph" else 30
    check("modulation", "impulse_flat", tag, form, modulation_plan("impulse_flat", dict(box=((0, 0, 15), (None, None, 1)), period=period), sections(3, 4), freqs(5)), n_steps, query)


MODULATION_BOXES = ["sub-box-630", "sub-box-567-odd", "one-node", "strides-1-2-3"]


@pytest.mark.parametrize("name", MODULATION_BOXES)
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_with_the_state_carried_across_two_folds(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters; B = 630 (more than one workgroup), 567 (odd, a tail),
    one node, strides (1, 2, 3); every step captured, 21 captures: 16 in the first fold, 5 in the second, which starts from the state
    and the sums the first one stored; the standard's 14 frequencies' worth of planes."""
    check("modulation", "random", tag, "triple", modulation_plan("random", dict(BOXES[name], period=1), sections(3, 4), freqs(14)), 20)


@pytest.mark.parametrize("k_bands,n_sections", [(1, 1), (2, 3), (8, 4)])
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_band_and_section_counts(name, k_bands, n_sections):
    check("modulation", "random", "f64", "pair", modulation_plan("random", dict(BOXES[name], period=1), sections(k_bands, n_sections), freqs(5)), 32)


@pytest.mark.parametrize("m", [1, 5, 14, 16])
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_frequency_counts_on_either_side_of_the_chunk(name, m):
    check("modulation", "random", "f64", "pair", modulation_plan("random", dict(BOXES[name], period=1), sections(2, 3), freqs(m)), 32)


@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_the_identity_section_at_zero_frequency_gives_the_plain_plans_sum(name):
    """{1, 0, 0, 0, 0} and f = 0: Re equals E bytewise, Im is zero, and both equal a plain decay plan's single bin."""
    plan = dict(BOXES[name], period=1)
    got = check("modulation", "random", "f64", "pair", modulation_plan("random", plan, IDENTITY, np.array([0.0])), 32)[0]
    got = (got["energy"], got["sums"])
    set_tuning(**FORMS["pair"])
    eng = make_engine(cases.CASES["random"](), "f64")
    eng.set_decay(1, 1, **plan)
    assert eng.run_steps(32) == (32, 0)
    plain, _ = eng.fetch_decay()
    eng.close()
    assert got[0][0].tobytes() == plain[0].tobytes() == np.ascontiguousarray(got[1][0, 0].real).tobytes() and plain.max() > 0
    assert not got[1].imag.any()


def test_either_destination_of_the_fetch_may_be_null():
    """wv_fetch_modulation with a NULL for the energies, for the sums, for both: the other comes back, and the captures with either."""
    plan = modulation_plan("random", dict(box=((3, 2, 4), (10, 9, 7)), period=1), sections(3, 4), freqs(14))
    eng = plan_engine("random", "f64", "pair", plan)
    try:
        assert eng.run_steps(30) == (30, 0)
        end = eng.fetch_modulation()
        captures = E.C.c_uint64()
        only_energy = np.zeros_like(end[0])
        E._check(eng.lib.wv_fetch_modulation(eng.h, only_energy.ctypes.data_as(E.C.c_void_p), None, E.C.byref(captures)))
        only_sums = np.zeros_like(end[1])
        E._check(eng.lib.wv_fetch_modulation(eng.h, None, only_sums.ctypes.data_as(E.C.c_void_p), None))
        E._check(eng.lib.wv_fetch_modulation(eng.h, None, None, None))
    finally:
        eng.close()
    assert captures.value == 31 and not_zeros(*end)
    assert only_energy.tobytes() == end[0].tobytes() and only_sums.tobytes() == end[1].tobytes()


def test_bad_arguments_and_a_null_plan_leave_an_earlier_plan_intact():
    """K = 0 or 9, S = 0 or 5, M = 0 or 17, a NaN or infinite coefficient, a NaN or a frequency outside [0, 0.5], a box that leaves the
    mesh, a zero stride or period: WV_E_INVALID_ARGUMENT, and after each the earlier plan's results are what they were and it goes on
    capturing.  A NULL plan stops it; then nothing is there to fetch or count."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    bands, f = sections(2, 3), freqs(5)
    snaps, steps = reference_snapshots("random", "f64", "single", plan, 32)
    eng = make_engine(case, "f64")
    assert refusal(lambda e: e.modulation_count(), eng) == [-6, "wv_modulation_count: no modulation plan is set"]
    assert refusal(lambda e: e.fetch_modulation(), eng) == [-6, "wv_fetch_modulation: no modulation plan is set"]
    eng.set_modulation(f, bands, **plan)
    assert eng.run_steps(5) == (5, 0)
    before = eng.fetch_modulation()
    for shape in ((0, 4, 5), (9, 4, 5), (1, 0, 5), (1, 5, 5)):
        assert refusal(lambda e: e.set_modulation(f, np.zeros(shape), **plan), eng) == [-1, "wv_set_modulation: n_bands must be 1 .. 8 and n_sections 1 .. 4"]
    for m in (0, 17):
        assert refusal(lambda e: e.set_modulation(np.full(m, 0.1), bands, **plan), eng) == [-1, "wv_set_modulation: n_freqs must be 1 .. 16"]
    for bad in (np.nan, np.inf, -np.inf):
        poisoned = bands.copy()
        poisoned[1, 2, 3] = bad
        assert refusal(lambda e: e.set_modulation(f, poisoned, **plan), eng) == [-1, "wv_set_modulation: every coefficient must be finite"]
    for bad in (np.nan, -1e-9, 0.5000001, np.inf):
        assert refusal(lambda e: e.set_modulation([0.1, bad], bands, **plan), eng) == [-1, "wv_set_modulation: a frequency outside [0, 0.5] cycles per step"]
    assert refusal(lambda e: e.set_modulation(f, bands, box=((0, 0, 0), (25, 20, 28))), eng) == [-1, "wv_set_modulation: the box leaves the mesh"]
    assert refusal(lambda e: e.set_modulation(f, bands, box="mesh", period=0), eng) == [-1, "wv_set_modulation: period must be >= 1"]
    assert refusal(lambda e: e.set_modulation(f, bands, box="mesh", stride=(1, 0, 1)), eng)[0] == -1
    assert eng.lib.wv_set_modulation(eng.h, E.C.byref(E.WvModulationPlan(nx=1, ny=1, nz=1, sx=1, sy=1, sz=1, period=1, n_freqs=1)), None, None, 1, 1) == -1
    after = eng.fetch_modulation()
    assert eng.modulation_count() == (6, 5) and same(after, before) and same(before, MOD.modulation_fold(snaps[:6], steps[:6], f, bands))
    assert eng.run_steps(3) == (3, 0) and eng.modulation_count() == (9, 8)
    want = MOD.modulation_fold(snaps[:9], steps[:9], f, bands)
    assert same(eng.fetch_modulation(), want) and not_zeros(*want)
    assert eng.set_modulation(None, None) is None
    assert refusal(lambda e: e.modulation_count(), eng) == [-6, "wv_modulation_count: no modulation plan is set"]
    assert refusal(lambda e: e.fetch_modulation(), eng) == [-6, "wv_fetch_modulation: no modulation plan is set"]
    assert eng.query(E.Engine.QUERY_MODULATION_CAPTURES) == 0
    # setting the plan again replaces it and forgets its sums
    eng.set_modulation(f, bands, **plan)
    eng.set_modulation(f, bands, **plan)
    assert eng.modulation_count() == (0, 0) and not eng.fetch_modulation()[0].any()
    eng.close()


ACTIVE = {
    "snapshots": "a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)",
    "spectrum": "a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)",
    "decay": "a decay plan is active (wv_set_decay(e, NULL) stops it)",
    "decay_bands": "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)",
    "intensity": "an intensity plan is active (wv_set_intensity(e, NULL) stops it)",
    "arrival": "an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it)",
    "lateral": "a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it)",
}
SETTER = {"snapshots": "wv_set_snapshots", "spectrum": "wv_set_spectrum", "decay": "wv_set_decay", "decay_bands": "wv_set_decay_bands",
          "intensity": "wv_set_intensity", "arrival": "wv_set_arrival", "lateral": "wv_set_lateral"}


def test_the_plans_exclude_each_other_in_both_orders():
    """The new plan under each of the seven existing kinds, each existing setter under the new plan: WV_E_STATE with the full sentence,
    the plan that was active untouched by the refusal (it still counts, and it can be stopped and set again)."""
    from wayverb_amd import engine as E2
    eng = E2.Engine(M.box_mesh(12, 10, 9), precision="f32")
    set_new = lambda e: e.set_modulation([0.0, 0.125], IDENTITY, box=((1, 1, 1), (4, 3, 2)))   # noqa: E731
    try:
        assert sorted(ACTIVE) == sorted(KINDS)
        for active in KINDS:
            SET[active](eng)
            assert refusal(set_new, eng) == [-6, "wv_set_modulation: " + ACTIVE[active] + "; the plans exclude each other"], active
            assert refusal(lambda e: e.modulation_count(), eng) == [-6, "wv_modulation_count: no modulation plan is set"]
            STOP[active](eng)
            set_new(eng)
            assert refusal(SET[active], eng) == [-6, SETTER[active] + ": " + SENTENCE], active
            assert eng.modulation_count() == (0, 0)
            eng.set_modulation(None, None)
            SET[active](eng)         # with the plan stopped the setter that was refused goes through
            STOP[active](eng)
    finally:
        eng.close()


def test_slabs_and_groups_refuse_the_plan():
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    assert refusal(lambda e: e.set_modulation([0.1], IDENTITY, box=((0, 0, 0), (4, 4, 1))), slab) == \
        [-6, "wv_set_modulation: not on a slab of a chain (one domain only)"]
    slab.close()
    eng = E.Engine(mesh, precision="f32")
    group = E.LocalSlabGroup([eng])
    eng.set_modulation([0.1], IDENTITY, box=((0, 0, 0), (4, 4, 1)))
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_run_group accumulates no modulation maps: .*wv_set_modulation\(e, NULL, NULL, NULL, 0, 0\) stops the plan"):
        group.run_steps(4)
    eng.set_modulation(None, None)
    assert group.run_steps(4) == (4, 0)
    group.close()


@pytest.mark.parametrize("captures", FILE_COUNTS["modulation"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("modulation", captures)


@pytest.mark.parametrize("form", FILE_FORMS["modulation"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_modulation_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("modulation", tag, form)


def test_canonical_designs_the_bands_at_the_rate_of_the_captured_series():
    """simulation.canonical(..., modulation=dict(plane=, every=2, bands_hz=, freqs_hz=)): the sums are the engine-level ones --
    modulation_fold over canonical's own snapshots of the same box and cadence with butterworth_bandpass(lo, hi, sample_rate / 2) over
    the octaves around bands_hz and freqs_hz / sample_rate cycles per step."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    box = ((0, 0, 12), (None, None, 1))
    centres, hz = [rate / 2 * 0.06, rate / 2 * 0.12], [rate * 0.01, rate * 0.05, rate * 0.2]
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=dict(box=box, period=2))
    out, ((energy, sums), captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                                  modulation=dict(plane=12 * vm.mesh.spacing, every=2, bands_hz=centres, freqs_hz=hz))
    assert out[0][0].tobytes() == plain[0][0].tobytes() and out[0][1:] == plain[0][1:]
    assert captures == 21 and energy.shape == (2, 1, 24, 24) and sums.shape == (2, 3, 1, 24, 24)
    bands = np.stack([D.butterworth_bandpass(lo, hi, rate / 2) for lo, hi in D.octave_band_edges(centres)])
    want = MOD.modulation_fold(fields, steps, MOD.cycles_per_step(hz, rate), bands)
    assert same((energy, sums), want) and not_zeros(*want)
    # a band the run cannot carry is warned about (here: above a quarter of the sample rate), as --decay-bands does
    with pytest.warns(UserWarning, match="above a quarter of the sample rate"):
        W.modulation_plan_arguments(dict(plane=12 * vm.mesh.spacing, bands_hz=[rate * 0.2]), vm.mesh, rate)


def test_the_tool_writes_the_maps_and_with_the_rest_of_the_bands_the_index(tmp_path):
    """tools/impulse_response.py --modulation-map z=1.5 --modulation-bands 31.5,63 on its built-in hall, a short run: mtf, mti,
    bands_hz, freqs_hz, captures; sti only when --sti-rest completes the seven bands."""
    base = [sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.03", "--precision", "f32",
            "--out", str(tmp_path / "ir.wav"), "--modulation-map", "z=1.5", "--modulation-every", "1"]
    out = tmp_path / "modulation.npz"
    p = subprocess.run(base + ["--modulation-bands", "31.5,63", "--modulation-out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        keys = set(f.files)
        mtf, mti, energy, captures = f["mtf"], f["mti"], f["energy"], int(f["captures"])
        assert list(f["bands_hz"]) == [31.5, 63.0] and list(f["freqs_hz"]) == list(MOD.STI_MODULATION_HZ)
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    assert {"mtf", "mti", "bands_hz", "freqs_hz", "captures"} <= keys and "sti" not in keys
    assert captures == steps + 1 and mtf.shape == (2, 14, dims[1], dims[0]) and mti.shape == (2, dims[1], dims[0])
    heard = energy > 0
    assert heard.any(axis=(1, 2)).all() and np.isnan(mtf[:, 0][~heard]).all()
    assert (mtf[:, :, heard.all(axis=0)] <= 1 + 1e-12).all() and (mtf[:, :, heard.all(axis=0)] >= 0).all()
    assert mti.tobytes() == MOD.mti(mtf).tobytes()
    # a 100 Hz cut-off (667 Hz sample rate) carries the 125 Hz octave, above a quarter of the sample rate: said, not refused; with the
    # other six bands given the index is written, with one of them missing it is not
    rest = "250:0.55,500:0.5,1000:0.5,2000:0.5,4000:0.45,8000:0.4"
    out2 = tmp_path / "sti.npz"
    p = subprocess.run(base + ["--modulation-bands", "125", "--sti-rest", rest, "--modulation-out", str(out2)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "above a quarter of the sample rate" in p.stderr
    with np.load(str(out2)) as f:
        sti, mti = f["sti"], f["mti"]
    assert sti.shape == mti.shape[1:]
    want = MOD.sti({125: mti[0]}, rest={250: 0.55, 500: 0.5, 1000: 0.5, 2000: 0.5, 4000: 0.45, 8000: 0.4})
    assert np.array_equal(sti, want, equal_nan=True) and np.isfinite(sti).any()
    assert ((sti[np.isfinite(sti)] > 0) & (sti[np.isfinite(sti)] < 1)).all()
    out3 = tmp_path / "no_sti.npz"
    p = subprocess.run(base + ["--modulation-bands", "125", "--sti-rest", rest.rsplit(",", 1)[0], "--modulation-out", str(out3)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "no sti is written" in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out3)) as f:
        assert "sti" not in f.files and "mti" in f.files


def test_the_rate_tool_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/modulation_rate.py on a 48 x 48 x 16 room, 48 steps per repeat, 2 bands and 5 frequencies: the rows none / decay bands /
    modulation at both periods are there, the sums equal modulation.modulation_fold over the snapshots bytewise at both, and the
    figures land in the JSON file."""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "modulation_rate.py"), "--dims", "48,48,16", "--steps", "48",
                        "--bands", "2", "--freqs", "5", "--repeats", "2", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 2 and "MODULATION RATE OK" in p.stdout, p.stdout
    report = json.load(open(str(out)))
    rows = ["%s, 2 bands every %d" % (plan, period) for plan in ("none", "decay bands", "modulation") for period in (1, 3)]
    assert sorted(report["f64"]["rows"]) == sorted(rows)
    assert report["f64"]["bytewise_equal"] == {"2 bands every 1": True, "2 bands every 3": True}
    for period in (1, 3):
        row = report["f64"]["rows"]["modulation, 2 bands every %d" % period]
        assert row["folds"] >= 1 and row["mean_fold_ms"] > 0 and row["model_bytes_mean_fold"] > 0
        ratio = report["f64"]["modulation_over_decay_bands"]["2 bands every %d" % period]
        assert ratio["per_fold_model"] > 1 and ratio["per_fold_measured"] > 0


def test_an_absorbing_room_transmits_modulation_better_than_a_nearly_rigid_one():
    """One physical check.  The same 16^3 cube (3.2 m a side at 0.2 m spacing, 2.9 kHz), source and plane twice: walls of absorption
    0.02 and of 0.7 in every band (filters.surface_coefficients).  An impulse, period 1, 1500 steps (half a second), one octave band
    centred at 0.05 of the sample rate.  Reverberation smears the envelope of the squared response: in the nearly rigid room the
    energy fills the half second, in the absorbing one it is gone after a tenth of it, so the mean transmission index over the
    plane's inside nodes is higher in the absorbing room at every modulation frequency above 2 Hz.  An inequality only."""
    from wayverb_amd import filters as F
    set_tuning()
    side, steps, spacing, speed = 16, 1500, 0.2, 340.0
    rate = speed * np.sqrt(3.0) / spacing
    lo, hi = D.octave_band_edges([0.05 * rate])[0]
    bands = D.butterworth_bandpass(lo, hi, rate)[None]
    hz = np.array(MOD.STI_MODULATION_HZ)
    f = MOD.cycles_per_step(hz, rate)
    means = []
    for absorption in (0.02, 0.7):
        mesh = M.box_mesh(side, side, side, coefficients=np.array([F.surface_coefficients(np.full(8, absorption), speed, spacing)],
                                                                   dtype=M.coefficients_dtype), spacing=spacing)
        signal = np.zeros(steps)
        signal[0] = 1.0
        eng = E.Engine(mesh, precision="f64")
        eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2 + 2, side // 2 - 1, side // 2 + 1), signal)
        eng.set_receivers([mesh.compute_index(5, 5, 5)])
        eng.set_modulation(f, bands, box=((0, 0, side // 4), (None, None, 1)), period=1)
        assert eng.run_steps(steps - 1) == (steps - 1, 0)
        energy, sums = eng.fetch_modulation()
        assert eng.modulation_count() == (steps, steps - 1)
        eng.close()
        inside = (mesh.nodes["boundary_type"].reshape(side, side, side)[side // 4] & M.ID_INSIDE) != 0
        ti = MOD.transmission_index(MOD.mtf(energy, sums))[0, :, 0][:, inside]
        assert inside.sum() > 100 and np.isfinite(ti).all()
        means.append(ti.mean(axis=1))
    print("mean transmission index over the plane, rigid / absorbing, per modulation frequency:")
    for row in zip(hz, means[0], means[1]):
        print("  %5.2f Hz  %.4f  %.4f" % row)
    above = hz > 2.0
    assert above.sum() == 8 and (means[1][above] > means[0][above]).all()

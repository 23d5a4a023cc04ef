"""Band-limited decay maps: biquad cascades per node and band ahead of the energy fold, on the device while wv_run keeps going
(wv_set_decay_bands; csrc/decay_bands_kernels.hip.h, engine_decay.hip.h).  The reference of every comparison is a second, identical
engine with a SNAPSHOT plan of the same box and cadence, pushed through decay.banded_bins -- the definition evaluated on float64 arrays,
one rounding per operation.  Equality is BYTEWISE, and every comparison asserts that it is not one of zeros.  Small meshes, forms forced,
a few dozen steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import numpy_bins, set_tuning
from plan_cases import (BOXES, FILE_COUNTS, FILE_FORMS, FORMS, LAYOUTS, STATE_FORM_CASES, box_scene, capture_counts, changes_nothing,
                        check, default_tuning_afterwards, make_engine, plan_on, reference_snapshots, sections)
from plan_cases import every_band as not_zeros
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]]])


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def banded_plan(case, cadence, bands, n_bins, bin_captures):
    return plan_on(case, "banded", bands=bands, n_bins=n_bins, bin_captures=bin_captures, **cadence)


@pytest.mark.parametrize("form,period,query", STATE_FORM_CASES, ids=["%s-every%d" % c[:2] for c in STATE_FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_banded_bins_of_the_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes; period 1 (every step ends a pass), 3 (three-step passes stay whole) and 7;
    one plane of the 32^3 impulse room, three bands of four sections, four captures per bin."""
    n_steps = 64 if form == "graph" else 30
    captures = n_steps // period + 1
    plan = banded_plan("impulse_flat", dict(box=((0, 0, 15), (None, None, 1)), period=period), sections(3, 4), -(-captures // 4), 4)
    check("banded", "impulse_flat", tag, form, plan, n_steps, query)


BAND_BOXES = ["sub-box-630", "sub-box-567-odd", "one-node", "strides-1-2-3"]


@pytest.mark.parametrize("name", BAND_BOXES)
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_with_the_state_carried_across_two_folds(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters; B = 630 (more than one workgroup), 567 (odd, a tail),
    one node, strides (1, 2, 3); every step captured, 21 captures: 16 in the first fold, 5 in the second, which starts from the state
    the first one stored."""
    check("banded", "random", tag, "triple", banded_plan("random", dict(BOXES[name], period=1), sections(3, 4), 7, 3), 20)


@pytest.mark.parametrize("k_bands,n_sections", [(1, 1), (8, 4), (2, 3)])
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_band_and_section_counts(name, k_bands, n_sections):
    check("banded", "random", "f64", "pair", banded_plan("random", dict(BOXES[name], period=1), sections(k_bands, n_sections), 7, 5), 32)


BAND_LAYOUTS = ["W1-every-capture-a-new-bin", "W5-edges-inside-and-across-folds", "W40-whole-folds-in-one-bin", "one-bin", "open-ended-last-bin"]


@pytest.mark.parametrize("layout", BAND_LAYOUTS)
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_bin_layouts_against_the_stage(name, layout):
    n_bins, bin_captures = LAYOUTS[layout]
    check("banded", "random", "f64", "pair", banded_plan("random", dict(BOXES[name], period=1), sections(2, 3), n_bins, bin_captures), 32)


@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_the_identity_section_gives_the_plain_plans_bins(name):
    """{1, 0, 0, 0, 0}: out = x * 1 + 0 = x exactly, the states stay +0.0 or -0.0 and add nothing: one band of a banded plan equals a
    plain set_decay engine's bins bytewise (and both the NumPy bins of the snapshots)."""
    plan = dict(BOXES[name], period=1)
    got, _, _, snaps, _ = check("banded", "random", "f64", "pair", banded_plan("random", plan, IDENTITY, 7, 5), 32)
    got = got["bins"]
    set_tuning(**FORMS["pair"])
    eng = make_engine(cases.CASES["random"](), "f64")
    eng.set_decay(7, 5, **plan)
    assert eng.run_steps(32) == (32, 0)
    plain, _ = eng.fetch_decay()
    eng.close()
    assert got[0].tobytes() == plain.tobytes() == numpy_bins(snaps, 7, 5).tobytes() and plain.max() > 0


def test_subnormal_floats_and_subnormal_states():
    """The field written through write_field at 1e-41: every captured float is a subnormal, which the conversion to double must keep.
    The first section's numerator is scaled by 1e-280, so its output and the states of the sections behind it are SUBNORMAL DOUBLES
    (about 1e-321, a few hundred units of the last place); the last section scales by 1e+280 back to where a square is not zero.
    Flushing either kind to zero would leave zeros, and rounding a subnormal differently other bytes."""
    set_tuning(**FORMS["pair"])
    mesh = M.box_mesh(12, 12, 12)
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=np.zeros(24),
                recv=[mesh.compute_index(7, 6, 6)])
    plan = dict(box=((0, 0, 5), (None, None, 2)), period=1)
    bw = D.butterworth_bandpass(0.05, 0.2, 1.0)
    first = bw[0].copy()
    first[:3] *= 1e-280
    bands = np.array([[first, bw[2], [1e280, 0.0, 0.0, 0.0, 0.0]]])
    rng = np.random.default_rng(11)
    fields = [rng.uniform(-1, 1, mesh.num_nodes) * 1e-41 * (mesh.nodes["boundary_type"] & M.ID_INSIDE != 0) for _ in range(2)]
    engines = [make_engine(case, "f64", plan), make_engine(case, "f64")]
    engines[1].set_decay(4, 5, bands=bands, **plan)
    for eng in engines:
        eng.write_field(fields[0], E.BUF_PREVIOUS)
        eng.write_field(fields[1], E.BUF_CURRENT)
        assert eng.run_steps(20) == (20, 0)
    snaps, steps = engines[0].fetch_snapshots()
    got, count = engines[1].fetch_decay()
    for eng in engines:
        eng.close()
    tiny32, tiny64 = np.finfo(np.float32).tiny, np.finfo(np.float64).tiny
    assert count == 21 and ((snaps != 0) & (np.abs(snaps) < tiny32)).mean() > 0.5
    want, state = D.banded_bins(snaps, bands, 4, 5, return_state=True)
    assert ((state[0, :2] != 0) & (np.abs(state[0, :2]) < tiny64)).mean() > 0.5
    assert got.tobytes() == want.tobytes() and (want[0].reshape(4, -1).max(axis=1) > 0).all()


def test_refusals_leave_an_earlier_plan_intact():
    """K = 0 or 9, S = 0 or 5, a NaN or infinite coefficient, whatever wv_set_decay refuses in a plan: WV_E_INVALID_ARGUMENT; another
    plan while a banded plan is active and a banded plan while another is -- a plain decay plan included, in both orders: WV_E_STATE
    with the plan to stop in the message; the wrong fetch: WV_E_STATE naming the other call.  After each refusal the earlier plan's
    results are what they were and it goes on capturing."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    bands = sections(2, 3)
    snaps, _ = reference_snapshots("random", "f64", "single", plan, 32)
    eng = make_engine(case, "f64")
    eng.set_decay(4, 2, bands=bands, **plan)
    assert eng.run_steps(5) == (5, 0)
    before, before_count = eng.fetch_decay()
    for shape in ((0, 4, 5), (9, 4, 5), (1, 0, 5), (1, 5, 5)):
        with pytest.raises(E.WaveguideError, match="error -1: .*n_bands must be 1 .. 8 and n_sections 1 .. 4"):
            eng.set_decay(4, 2, bands=np.zeros(shape), **plan)
    for bad in (np.nan, np.inf, -np.inf):
        poisoned = bands.copy()
        poisoned[1, 2, 3] = bad
        with pytest.raises(E.WaveguideError, match="error -1: .*finite"):
            eng.set_decay(4, 2, bands=poisoned, **plan)
    for n_bins, bin_captures in ((0, 1), (4097, 1), (4, 0)):
        with pytest.raises(E.WaveguideError, match="error -1: wv_set_decay_bands: .*(n_bins|bin_captures)"):
            eng.set_decay(n_bins, bin_captures, bands=bands, **plan)
    with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
        eng.set_decay(4, 2, bands=bands, box=((0, 0, 0), (25, 20, 28)))
    with pytest.raises(E.WaveguideError, match="error -1: .*period"):
        eng.set_decay(4, 2, bands=bands, box="mesh", period=0)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_snapshots: a banded decay plan is active \(wv_set_decay_bands\(e, NULL, NULL, 0, 0\)"):
        eng.set_snapshots(**plan)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_spectrum: a banded decay plan is active \(wv_set_decay_bands\(e, NULL, NULL, 0, 0\)"):
        eng.set_spectrum([0.1], **plan)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_decay: a banded decay plan is active \(wv_set_decay_bands\(e, NULL"):
        eng.set_decay(4, 2, **plan)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_fetch_decay: .*wv_fetch_decay_bands"):
        eng.fetch_decay(banded=False)
    after, after_count = eng.fetch_decay()
    assert after_count == before_count == 6 and after.tobytes() == before.tobytes() == D.banded_bins(snaps[:6], bands, 4, 2).tobytes()
    assert eng.run_steps(3) == (3, 0) and eng.decay_count() == (9, 8)
    want = D.banded_bins(snaps[:9], bands, 4, 2)
    assert eng.fetch_decay()[0].tobytes() == want.tobytes() and not_zeros(want)
    # a NULL plan through either setter stops it; then nothing is there to fetch or count
    eng.set_decay(None)
    with pytest.raises(E.WaveguideError, match="error -6: .*no decay plan"):
        eng.fetch_decay(banded=True)
    with pytest.raises(E.WaveguideError, match="error -6: .*no decay plan"):
        eng.decay_count()
    assert eng.lib.wv_set_decay_bands(eng.h, None, None, 0, 0) == 0
    eng.close()
    # the other orders: a plain decay plan is active
    eng = make_engine(case, "f64")
    eng.set_decay(4, 2, **plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_decay_bands: a plain decay plan is active \(wv_set_decay\(e, NULL\)"):
        eng.set_decay(4, 2, bands=bands, **plan)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_fetch_decay_bands: .*wv_fetch_decay "):
        eng.fetch_decay(banded=True)
    assert eng.run_steps(2) == (2, 0)
    assert eng.fetch_decay()[0].tobytes() == numpy_bins(snaps[:5], 4, 2).tobytes()
    assert eng.lib.wv_set_decay_bands(eng.h, None, None, 0, 0) == 0       # ... stops a plain plan as well
    with pytest.raises(E.WaveguideError, match="error -6: .*no decay plan"):
        eng.decay_count()
    eng.close()
    # ... a snapshot plan is active
    eng = make_engine(case, "f64", plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_decay_bands: a snapshot plan is active \(wv_set_snapshots\(e, NULL\)"):
        eng.set_decay(4, 2, bands=bands, **plan)
    assert eng.run_steps(2) == (2, 0)
    got, steps = eng.fetch_snapshots()
    assert list(steps) == [0, 1, 2, 3, 4] and got.tobytes() == snaps[:5].tobytes()
    eng.close()
    # ... a spectrum plan is active
    eng = make_engine(case, "f64")
    eng.set_spectrum([0.0], **plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match=r"error -6: wv_set_decay_bands: a spectrum plan is active \(wv_set_spectrum\(e, NULL, NULL\)"):
        eng.set_decay(4, 2, bands=bands, **plan)
    assert eng.run_steps(2) == (2, 0)
    spectrum, count = eng.fetch_spectrum()
    plain = np.zeros(snaps.shape[1:])
    for p in snaps[:5]:
        plain = plain + p.astype(np.float64)
    assert count == 5 and spectrum[0].real.tobytes() == plain.tobytes() and np.abs(plain).max() > 0
    eng.close()
    # a slab of a chain
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    with pytest.raises(E.WaveguideError, match="error -6: wv_set_decay_bands: .*slab of a chain"):
        slab.set_decay(2, 2, bands=bands, box=((0, 0, 0), (4, 4, 1)))
    slab.close()
    # a group takes no engine with a banded plan
    eng = E.Engine(mesh, precision="f32")
    group = E.LocalSlabGroup([eng])
    eng.set_decay(2, 2, bands=bands, box=((0, 0, 0), (4, 4, 1)))
    with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no decay bins"):
        group.run_steps(4)
    eng.set_decay(None)
    assert group.run_steps(4) == (4, 0)
    group.close()


@pytest.mark.parametrize("captures", FILE_COUNTS["banded"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("banded", captures)


@pytest.mark.parametrize("form", FILE_FORMS["banded"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_banded_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("banded", tag, form)


def test_canonical_designs_the_bands_at_the_rate_of_the_captured_series():
    """simulation.canonical(..., decay=dict(..., bands=[(lo_hz, hi_hz), ...])): the bins are the engine-level ones -- banded_bins over
    canonical's own snapshots of the same box and cadence with butterworth_bandpass(lo, hi, sample_rate / period)."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    box = ((0, 0, 12), (None, None, 1))
    edges = [(rate / 2 * 0.04, rate / 2 * 0.08), (rate / 2 * 0.08, rate / 2 * 0.16)]
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=dict(box=box, period=2))
    out, (bins, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                        decay=dict(n_bins=5, bin_captures=4, box=box, period=2, bands=edges))
    assert out[0][0].tobytes() == plain[0][0].tobytes() and out[0][1:] == plain[0][1:]
    assert captures == 21 and bins.shape == (2, 5, 1, 24, 24)
    want = D.banded_bins(fields, np.stack([D.butterworth_bandpass(lo, hi, rate / 2) for lo, hi in edges]), 5, 4)
    assert bins.tobytes() == want.tobytes() and not_zeros(want)


def test_the_tool_writes_per_band_maps(tmp_path):
    """tools/impulse_response.py --decay-map z=... --decay-bands 31.5,63 --decay-every 1 on its built-in hall, a short run: every map
    has a leading band axis, and the warnings about a band above a quarter of the sample rate do not fire for these."""
    out = tmp_path / "decay.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.03",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--decay-map", "z=1.5", "--decay-bin-ms", "5",
                        "--decay-every", "1", "--decay-bands", "31.5,63", "--decay-out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        bins, captures, per_bin, period, rate = f["bins"], int(f["captures"]), int(f["bin_captures"]), int(f["period"]), float(f["sample_rate"])
        maps = {k: f[k] for k in ("edt_s", "t20_s", "t30_s", "edt_r", "t20_r", "t30_r", "level_db", "edc_db")}
        centres, edges = f["band_centres_hz"], f["band_edges_hz"]
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    assert period == 1 and captures == steps + 1 and per_bin == max(1, int(round(0.005 * rate)))
    assert bins.dtype == np.float64 and bins.shape == (2, -(-captures // per_bin), dims[1], dims[0]) and not_zeros(bins)
    assert list(centres) == [31.5, 63.0] and edges.shape == (2, 2) and edges[1, 1] < 0.25 * rate and "warning" not in p.stderr
    for name in ("edt_s", "t20_s", "t30_s", "edt_r", "t20_r", "t30_r", "level_db"):
        assert maps[name].shape == (2, dims[1], dims[0]), name
    assert maps["edc_db"].shape == bins.shape and np.isfinite(maps["level_db"]).any(axis=(1, 2)).all()
    want = D.band_decay_maps(bins, per_bin, 1, rate)
    assert all(maps[name].tobytes() == want[name].tobytes() for name in maps)
    assert bins[0].tobytes() != bins[1].tobytes()


def test_the_tool_warns_about_bands_the_run_cannot_carry(tmp_path):
    """A 1 kHz octave on a mesh sampled for a 100 Hz cut-off, captured every third step: above a quarter of the sample rate is said,
    above the Nyquist rate of the captured series is said, and the design function refuses the band."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.01",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--decay-map", "z=1.5", "--decay-bands", "1000",
                        "--decay-out", str(tmp_path / "decay.npz")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert "above a quarter of the sample rate" in p.stderr and "it aliases" in p.stderr
    assert p.returncode != 0 and "lo_hz < hi_hz < sample_rate / 2" in p.stderr


def test_the_rate_tool_with_bands_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/decay_rate.py --bands 2 on a 48^3 room, 48 steps per repeat: the rows none / plain / bands 2 at both periods are there, the
    banded bins equal decay.banded_bins over the snapshots bytewise at both, and the figures land in the JSON file."""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "decay_rate.py"), "--side", "48", "--steps", "48",
                        "--bin-captures", "5", "--bands", "2", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 2 and "DECAY BANDS RATE OK" in p.stdout, p.stdout
    report = json.load(open(str(out)))
    rows = ["%s every %d" % (plan, period) for plan in ("none", "plain", "bands 2") for period in (1, 3)]
    assert sorted(report["f64"]["rows"]) == sorted(rows)
    assert report["f64"]["bytewise_equal"] == {"bands 2 every 1": True, "bands 2 every 3": True}
    for period in (1, 3):
        row = report["f64"]["rows"]["bands 2 every %d" % period]
        assert row["folds"] >= 1 and row["mean_fold_ms"] > 0 and row["steps_per_s_median"] > 0


def test_a_room_that_absorbs_more_at_high_frequencies_decays_faster_there():
    """One physical check, end to end.  A 40^3 box room (2 m a side, 11.8 kHz), every wall the reference's reflectance filter
    (wv_reflectance_filter) for absorption 0.05 in its four lower bands and 0.4 in its four upper ones -- a ratio of 8, which is the
    ratio of the reverberation times Sabine predicts.  An impulse, period 1, 2400 steps, ten captures per bin, two octave bands centred at
    0.025 and 0.1 of the sample rate (upper edge 0.141, below 0.2), on the plane z = 10 (the source sits at z = 21), at the plane's
    nodes inside the room.  The bars: the median T20 at least 2 x longer in the low band (2 leaves room for Eyring, for the few modes
    of so small a room in the low octave, and for the filter's fit between its bands), and t20_r < -0.95 at no fewer than 90 % of the
    nodes in both bands.  The CPU oracle, through snapshots and decay.py, gives a ratio of 4.23 (0.304 s against 0.0719 s) and shares
    of 100 % and 99.5 %."""
    from wayverb_amd import filters as F
    set_tuning()
    side, steps, per_bin, spacing, speed = 40, 2400, 10, 0.05, 340.0
    rate = speed * np.sqrt(3.0) / spacing
    absorption = np.array([0.05] * 4 + [0.4] * 4)
    mesh = M.box_mesh(side, side, side, coefficients=np.array([F.surface_coefficients(absorption, speed, spacing)], dtype=M.coefficients_dtype),
                      spacing=spacing)
    edges = D.octave_band_edges([0.025 * rate, 0.1 * rate])
    assert edges[1][1] < 0.2 * rate
    bands = np.stack([D.butterworth_bandpass(lo, hi, rate) for lo, hi in edges])
    signal = np.zeros(steps)
    signal[0] = 1.0
    eng = E.Engine(mesh, precision="f64")
    eng.set_source(E.SOURCE_HARD, mesh.compute_index(side // 2 + 3, side // 2 - 2, side // 2 + 1), signal)
    eng.set_receivers([mesh.compute_index(5, 5, 5)])
    eng.set_decay(steps // per_bin, per_bin, bands=bands, box=((0, 0, side // 4), (None, None, 1)), period=1)
    assert eng.run_steps(steps - 1) == (steps - 1, 0)
    bins, captures = eng.fetch_decay()
    eng.close()
    assert captures == steps and bins.shape == (2, steps // per_bin, 1, side, side)
    maps = D.band_decay_maps(bins[:, :, 0], per_bin, 1, rate)
    z = side // 4
    inside = (mesh.nodes["boundary_type"].reshape(side, side, side)[z] & M.ID_INSIDE) != 0
    t20 = [np.nanmedian(maps["t20_s"][k][inside]) for k in range(2)]
    share = [float((maps["t20_r"][k][inside] < -0.95).mean()) for k in range(2)]
    print("median T20 %.4f s / %.4f s (ratio %.3f); t20_r < -0.95 at %.1f %% / %.1f %% of %d nodes"
          % (t20[0], t20[1], t20[0] / t20[1], 100 * share[0], 100 * share[1], int(inside.sum())))
    assert inside.sum() > 1000
    assert t20[0] >= 2 * t20[1] > 0
    assert min(share) >= 0.9

"""Energy decay maps: time-binned field energy accumulated on the device while wv_run keeps going (wv_set_decay;
csrc/decay_kernels.hip.h, engine_decay.hip.h).  The reference of every comparison is a second, identical engine with a SNAPSHOT plan of
the same box and cadence, whose snapshots are binned in NumPy in capture order: `E[b] = E[b] + p * p` on float64 arrays is an exact
product and a rounded sum, which is the definition.  Equality is BYTEWISE.  Small meshes, forms forced, a few dozen steps."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import numpy_bins, set_tuning
from plan_cases import (BOXES, FILE_COUNTS, FILE_FORMS, FORMS, FORM_CASES, LAYOUTS, box_scene, capture_counts, changes_nothing,
                        check, default_tuning_afterwards, make_engine, plan_on, reference_snapshots)
from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def decay_plan(case, cadence, n_bins, bin_captures):
    return plan_on(case, "decay", n_bins=n_bins, bin_captures=bin_captures, **cadence)


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_bins_of_the_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes, periods that do and do not divide 2 and 3: one plane of the 32^3 impulse
    room, four captures per bin.  The bins summed over time are the plain ordered sum of p^2 only up to rounding, so the check on the
    whole is the bytewise one."""
    n_steps = 64 if form == "graph" else 30
    captures = n_steps // period + 1
    check("decay", "impulse_flat", tag, form, decay_plan("impulse_flat", dict(box=((0, 0, 15), (None, None, 1)), period=period), -(-captures // 4), 4), n_steps, query)


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; every step captured, 21 captures
    (more than the stage holds), three captures per bin."""
    check("decay", "random", tag, "triple", decay_plan("random", dict(BOXES[name], period=1), 7, 3), 20)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_bin_layouts_against_the_stage(name, layout):
    n_bins, bin_captures = LAYOUTS[layout]
    got = check("decay", "random", "f64", "pair", decay_plan("random", dict(BOXES[name], period=1), n_bins, bin_captures), 32)[0]["bins"]
    if layout == "more-bins-than-captures":
        assert (got[33:] == 0).all() and not np.signbit(got[33:]).any()    # never touched: +0.0


def test_refusals_leave_an_earlier_plan_intact():
    """n_bins 0 and 4097, zero bin_captures, a zero stride or period, a box off the mesh: WV_E_INVALID_ARGUMENT; either other plan while
    a decay plan is active and a decay plan while either other is: WV_E_STATE with the plan to stop in the message; after each refusal
    the earlier plan's results are what they were and it goes on capturing."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    snaps, _ = reference_snapshots("random", "f64", "single", plan, 32)
    eng = make_engine(case, "f64")
    eng.set_decay(4, 2, **plan)
    assert eng.run_steps(5) == (5, 0)
    before, before_count = eng.fetch_decay()
    for n_bins, bin_captures in ((0, 1), (4097, 1), (4, 0)):
        with pytest.raises(E.WaveguideError, match="error -1: .*(n_bins|bin_captures)"):
            eng.set_decay(n_bins, bin_captures, **plan)
    for bad_box in (((0, 0, 0), (25, 20, 28)), ((-1, 0, 0), (4, 4, 4)), ((0, 0, 28), (1, 1, 1))):
        with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
            eng.set_decay(4, 2, box=bad_box)
    with pytest.raises(E.WaveguideError, match="error -1: .*stride"):
        eng.set_decay(4, 2, box="mesh", stride=(1, 0, 1))
    with pytest.raises(E.WaveguideError, match="error -1: .*period"):
        eng.set_decay(4, 2, box="mesh", period=0)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*decay plan is active \(wv_set_decay\(e, NULL\)"):
        eng.set_snapshots(**plan)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*decay plan is active \(wv_set_decay\(e, NULL\)"):
        eng.set_spectrum([0.1], **plan)
    after, after_count = eng.fetch_decay()
    assert after_count == before_count == 6 and after.tobytes() == before.tobytes() == numpy_bins(snaps[:6], 4, 2).tobytes()
    assert eng.run_steps(3) == (3, 0) and eng.decay_count() == (9, 8)
    assert eng.fetch_decay()[0].tobytes() == numpy_bins(snaps[:9], 4, 2).tobytes() and after.max() > 0
    eng.close()
    # the other orders: a snapshot plan is active
    eng = make_engine(case, "f64", plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*snapshot plan is active \(wv_set_snapshots\(e, NULL\)"):
        eng.set_decay(4, 2, **plan)
    assert eng.run_steps(2) == (2, 0)
    got, steps = eng.fetch_snapshots()
    assert list(steps) == [0, 1, 2, 3, 4] and got.tobytes() == snaps[:5].tobytes()
    eng.close()
    # ... a spectrum plan is active
    eng = make_engine(case, "f64")
    eng.set_spectrum([0.0], **plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match=r"error -6: .*spectrum plan is active \(wv_set_spectrum\(e, NULL, NULL\)"):
        eng.set_decay(4, 2, **plan)
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
    with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
        slab.set_decay(2, 2, box=((0, 0, 0), (4, 4, 1)))
    slab.close()
    # no plan: the library's WV_E_STATE; a group takes no engine with a plan
    eng = E.Engine(mesh, precision="f32")
    with pytest.raises(E.WaveguideError, match="error -6: .*no decay plan"):
        eng.fetch_decay()
    group = E.LocalSlabGroup([eng])
    eng.set_decay(2, 2, box=((0, 0, 0), (4, 4, 1)))
    with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no decay bins"):
        group.run_steps(4)
    eng.set_decay(None)
    assert group.run_steps(4) == (4, 0)
    group.close()


def test_decay_maps_end_to_end_on_one_plane():
    """decay_maps on a decay-plan run of the 32^3 impulse room, one plane, eight captures per bin, every step, against decay.py applied
    to bins accumulated from the snapshots: equal, and the early decay time is finite wherever the level is.  128 captures in 16 bins:
    the first sound reaches the plane's corners after some 40 steps, which leaves every node ten edges behind its arrival.  The plane
    is z = 6, ten nodes from the hard source: in the plane next to the source (z = 15) the three nodes nearest to it hold more than
    90 % of their energy in the impulse itself, their curve falls 12.9 dB inside the first bin, no point lies in 0 .. -10 dB and the
    reference's edt throws there -- NaN by the definition, not a defect (the restated oracle on the CPU shows it; on z = 6 it shows all
    900 heard nodes finite, the unheard 124 being the outside shell)."""
    plan = dict(box=((0, 0, 6), (None, None, 1)), period=1)
    got, _, _, snaps, _ = check("decay", "impulse_flat", "f32", "triple", decay_plan("impulse_flat", plan, 16, 8), 127)
    got = got["bins"]
    rate = 8000.0
    maps = D.decay_maps(got[:, 0], 8, 1, rate)
    want = D.decay_maps(numpy_bins(snaps, 16, 8)[:, 0], 8, 1, rate)
    print("EDT: %d of %d nodes heard, %d finite; range %g .. %g s" % (np.isfinite(maps["level_db"]).sum(), maps["level_db"].size,
          np.isfinite(maps["edt_s"]).sum(), np.nanmin(maps["edt_s"]), np.nanmax(maps["edt_s"])))
    assert sorted(maps) == ["edc_db", "edt_r", "edt_s", "level_db", "t20_r", "t20_s", "t30_r", "t30_s"]
    for name in maps:
        assert maps[name].tobytes() == want[name].tobytes(), name
    assert maps["edt_s"].shape == maps["level_db"].shape == got.shape[2:] and maps["edc_db"].shape == (16,) + got.shape[2:]
    heard = np.isfinite(maps["level_db"])
    assert heard.any() and np.isfinite(maps["edt_s"][heard]).all() and (maps["edt_s"][heard] > 0).all()
    assert np.isnan(maps["edt_s"][~heard]).all()


@pytest.mark.parametrize("captures", FILE_COUNTS["decay"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("decay", captures)


@pytest.mark.parametrize("form", FILE_FORMS["decay"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("decay", tag, form)


def test_canonical_returns_the_bins_beside_the_receiver_output():
    """simulation.canonical(..., decay=...): the records are those of a run without a plan, the bins are the engine-level ones (binned
    from canonical's own snapshots of the same box and cadence); a second plan beside it is refused with the engine's message."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    box = ((0, 0, 12), (None, None, 1))
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=dict(box=box, period=2))
    bands, (bins, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                          decay=dict(n_bins=5, bin_captures=4, box=box, period=2))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 21 and bins.shape == (5, 1, 24, 24)
    assert bins.tobytes() == numpy_bins(fields, 5, 4).tobytes() and bins.max() > 0
    with pytest.raises(E.WaveguideError, match="error -6: .*snapshot plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, snapshots=dict(period=8), decay=dict(n_bins=2, bin_captures=2))
    with pytest.raises(E.WaveguideError, match="error -6: .*spectrum plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, spectrum=dict(freqs_hz=[10.0]), decay=dict(n_bins=2, bin_captures=2))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, decay=dict(n_bins=2, bin_captures=2))


def test_the_tool_writes_the_decay_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --decay-map z=... --decay-bin-ms --decay-every --decay-out FILE.npz on its built-in hall, a short run."""
    out = tmp_path / "decay.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.03",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--decay-map", "z=1.5", "--decay-bin-ms", "5",
                        "--decay-out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        bins, captures, per_bin, period, rate = f["bins"], int(f["captures"]), int(f["bin_captures"]), int(f["period"]), float(f["sample_rate"])
        level, edt, plane, origin, spacing = f["level_db"], f["edt_s"], int(f["plane"]), f["origin"], float(f["spacing"])
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    assert bins.dtype == np.float64 and bins.shape[1:] == (dims[1], dims[0]) and bins.shape[0] == -(-captures // per_bin)
    assert period == 3 and captures == steps // 3 + 1 and per_bin == max(1, int(round(0.005 * rate / 3)))
    assert 0 <= plane < dims[2] and origin.shape == (3,) and spacing > 0 and bins.max() > 0
    assert level.shape == edt.shape == bins.shape[1:] and np.isfinite(level).any()


def test_the_rate_tool_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/decay_rate.py on a 48^3 room, 48 steps per repeat: every row is there, the bins of the snapshot-and-host way equal the
    decay plan's bytewise in all four, and the figures land in the JSON file.  (Whether the bar holds is a matter of the 512^3 run, not
    of this size: the exit status may say either.)"""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "decay_rate.py"), "--side", "48", "--steps", "48",
                        "--bin-captures", "5", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode in (0, 1), p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 4 and "DECAY RATE" in p.stdout, p.stdout
    import json
    report = json.load(open(str(out)))
    rows = ["%s %s every %d" % (way, box, period) for way in "ab" for box in ("field", "plane") for period in (1, 3)]
    assert sorted(report["f64"]["rows"]) == sorted(rows)
    assert len(report["f64"]["verdicts"]) == 4 and all(v["bytewise_equal_to_old"] for v in report["f64"]["verdicts"].values())

"""Intensity maps: time-binned sound intensity of a box accumulated on the device while wv_run keeps going (wv_set_intensity;
csrc/intensity_kernels.hip.h, engine_intensity.hip.h).  The reference of every comparison is a second, identical engine with a SNAPSHOT
plan of the box's HULL at stride 1 and the same cadence, whose snapshots go through intensity.intensity_bins -- the definition, the
float lines on float32 arrays and the rest on float64.  Bins AND velocities are compared BYTEWISE, and every comparison also asserts
that all four planes hold something non-zero.  Small meshes, forms forced, a few dozen steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import canonical_parameters, set_tuning
from plan_cases import HULL_BOXES as BOXES
from plan_cases import (FILE_COUNTS, FILE_FORMS, FORMS, LAYOUTS, STATE_FORM_CASES, box_scene, capture_counts, changes_nothing, check, constants,
                        default_tuning_afterwards, hull_of, make_engine, plan_engine, plan_on, reference_snapshots)
from plan_cases import every_plane as nonzero
from wayverb_amd import engine as E
from wayverb_amd import intensity as I
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACING, RATE, DENSITY = canonical_parameters()


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


def intensity_plan(case, cadence, n_bins, w):
    return plan_on(case, "intensity", n_bins=n_bins, bin_captures=w, **cadence)


def definition(snaps, plan, n_bins, w, **more):
    _, box_in_hull = hull_of(plan)
    c = constants(plan)
    return I.intensity_bins(snaps, box_in_hull, c["spacing"], c["sample_rate"], c["ambient_density"], n_bins, w, return_velocity=True, **more)


PLANE = dict(box=((1, 1, 15), (30, 30, 1)))


@pytest.mark.parametrize("form,period,query", STATE_FORM_CASES, ids=["%s-every%d" % c[:2] for c in STATE_FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_bins_of_the_hull_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes; period 1 (every step ends a pass), 3 (three-step passes stay whole) and 7;
    the plane z = 15 of the 32^3 impulse room less its rim, four captures per bin."""
    n_steps = 64 if form == "graph" else 30
    captures = n_steps // period + 1
    check("intensity", "impulse_flat", tag, form, intensity_plan("impulse_flat", dict(PLANE, period=period), -(-captures // 4), 4), n_steps, query)


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; every step captured, 21 captures (16 in
    the first fold, 5 in the second, which starts from the velocities the first one stored), three captures per bin."""
    got = check("intensity", "random", tag, "triple", intensity_plan("random", dict(BOXES[name], period=1), 7, 3), 20)[0]
    assert np.isfinite(got["bins"]).all()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_bin_layouts_against_the_stage(name, layout):
    n_bins, w = LAYOUTS[layout]
    got = check("intensity", "random", "f64", "pair", intensity_plan("random", dict(BOXES[name], period=1), n_bins, w), 32)[0]["bins"]
    if layout == "more-bins-than-captures":
        assert (got[:, 33:] == 0).all() and not np.signbit(got[:, 33:]).any()    # never touched: +0.0


def test_the_energy_planes_are_a_plain_decay_plans_bins():
    plan = dict(BOXES["strides-1-2-3"], period=2)
    got = check("intensity", "random", "f64", "triple", intensity_plan("random", plan, 4, 3), 30)[0]["bins"]
    set_tuning(**FORMS["triple"])
    eng = make_engine(cases.CASES["random"](), "f64")
    eng.set_decay(4, 3, **plan)
    assert eng.run_steps(30) == (30, 0)
    decay, count = eng.fetch_decay()
    eng.close()
    assert count == 16 and got[3].tobytes() == decay.tobytes() and decay.max() > 0


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_the_receiver_path_carries_the_same_velocities(tag):
    """Four nodes whose 7-point hull does not hold the source node, period 1, first_step 0: the directional receivers' float records
    are (float)(v * p) of the definition's velocities, step by step -- so their sums in double per bin are the definition's sums of
    the rounded products -- and the velocities the receiver path carries after the run equal the plan's, bytewise."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    mesh = case["mesh"]
    sx, sy, sz = mesh.compute_locator(case["source_node"])
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    picks = [(x, y, z) for (x, y, z) in ((3, 2, 4), (12, 10, 10), (7, 6, 5), (4, 10, 9)) if abs(x - sx) + abs(y - sy) + abs(z - sz) > 1]
    assert len(picks) == 4, "the case's source moved next to a picked node"
    n = 24
    recv = make_engine(case, tag)
    recv.set_directional_receivers([mesh.compute_index(*p) for p in picks], SPACING, RATE, DENSITY)
    assert recv.run_steps(n) == (n, 0)                      # records of steps 0 .. n - 1
    records = recv.fetch_directional(0, n)
    recv_v = recv.fetch_directional_velocity(4)
    recv.close()
    eng = plan_engine(case, tag, "pair", intensity_plan(case, plan, 6, 4))
    assert eng.run_steps(n - 1) == (n - 1, 0)               # captures of steps 0 .. n - 1
    assert eng.intensity_count() == (n, n - 1)
    got, _ = eng.fetch_intensity()
    got_v = eng.fetch_intensity_velocity()
    eng.close()
    snaps, _ = reference_snapshots("random", tag, "pair", hull_of(plan)[0], 32)
    want, want_v = definition(snaps[:n], plan, 6, 4)
    assert got.tobytes() == want.tobytes() and got_v.tobytes() == want_v.tobytes()
    v = None
    sums = np.zeros((3, 6, 4))
    for j in range(n):
        _, v = definition(snaps[j:j + 1], plan, 1, 1, velocity=v, first_capture=j)
        for r, (x, y, z) in enumerate(picks):
            at = (z - 4, y - 2, x - 3)
            p = snaps[j][at[0] + 1, at[1] + 1, at[2] + 1]
            rounded = (v[(slice(None),) + at] * np.float64(p)).astype(np.float32)
            assert records[j, r]["pressure"].tobytes() == p.tobytes()
            assert records[j, r]["intensity"].tobytes() == rounded.tobytes(), (j, r)
            sums[:, min(j // 4, 5), r] = sums[:, min(j // 4, 5), r] + rounded.astype(np.float64)
    per_bin = np.zeros((3, 6, 4))
    for j in range(n):
        per_bin[:, min(j // 4, 5), :] = per_bin[:, min(j // 4, 5), :] + records["intensity"][j].astype(np.float64).T
    assert per_bin.tobytes() == sums.tobytes() and np.abs(sums).min() > 0
    for r, (x, y, z) in enumerate(picks):
        assert recv_v[r].tobytes() == got_v[:, z - 4, y - 2, x - 3].tobytes()
    assert np.abs(recv_v).min() > 0


def test_refusals_leave_an_earlier_plan_intact_and_the_plans_exclude_each_other():
    """Every WV_E_INVALID_ARGUMENT leaves the running plan as it was; the five setters refuse each other with the plan to stop in the
    message; a slab of a chain and wv_run_group refuse."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(BOXES["sub-box-630"], period=1)
    c = constants(plan)
    snaps, _ = reference_snapshots("random", "f64", "single", hull_of(plan)[0], 32)
    eng = make_engine(case, "f64")
    eng.set_intensity(4, 2, **plan, **c)
    assert eng.run_steps(5) == (5, 0)
    before, before_count = eng.fetch_intensity()
    for n_bins, w in ((0, 1), (4097, 1), (4, 0)):
        with pytest.raises(E.WaveguideError, match="error -1: .*(n_bins|bin_captures)"):
            eng.set_intensity(n_bins, w, **plan, **c)
    for bad_box in (((1, 1, 1), (24, 18, 26)), ((-1, 1, 1), (4, 4, 4)), ((1, 1, 28), (1, 1, 1))):
        with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
            eng.set_intensity(4, 2, box=bad_box, **c)
    for edge_box in (((0, 1, 1), (4, 4, 4)), ((1, 0, 1), (4, 4, 4)), ((1, 1, 0), (4, 4, 4)), ((1, 1, 1), (23, 4, 4)), ((1, 1, 1), (4, 19, 4)),
                     ((1, 1, 1), (4, 4, 27))):
        with pytest.raises(E.WaveguideError, match="error -1: Can't place directional_receiver at this node as it is adjacent to a boundary."):
            eng.set_intensity(4, 2, box=edge_box, **c)
    with pytest.raises(E.WaveguideError, match="error -1: .*stride"):
        eng.set_intensity(4, 2, stride=(1, 0, 1), **c)
    with pytest.raises(E.WaveguideError, match="error -1: .*period"):
        eng.set_intensity(4, 2, period=0, **c)
    for bad in (dict(c, spacing=0.0), dict(c, sample_rate=-1.0), dict(c, ambient_density=float("inf")), dict(c, spacing=float("nan"))):
        with pytest.raises(E.WaveguideError, match="error -1: .*positive and finite"):
            eng.set_intensity(4, 2, **plan, **bad)
    snapshot_plan = dict(box=plan["box"], period=1)
    bands = np.array([[[1.0, 0, 0, 0, 0]]])
    stop = r"error -6: .*intensity plan is active \(wv_set_intensity\(e, NULL\)"
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_snapshots(**snapshot_plan)
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_spectrum([0.1], **snapshot_plan)
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_decay(4, 2, **snapshot_plan)
    with pytest.raises(E.WaveguideError, match=stop):
        eng.set_decay(4, 2, bands=bands, **snapshot_plan)
    after, after_count = eng.fetch_intensity()
    assert after_count == before_count == 6 and after.tobytes() == before.tobytes() == definition(snaps[:6], plan, 4, 2)[0].tobytes()
    assert eng.run_steps(3) == (3, 0) and eng.intensity_count() == (9, 8)
    want, want_v = definition(snaps[:9], plan, 4, 2)
    assert eng.fetch_intensity()[0].tobytes() == want.tobytes() and eng.fetch_intensity_velocity().tobytes() == want_v.tobytes()
    assert nonzero(want, want_v)
    eng.close()
    # the other orders: each of the four other plans is active
    for setter, stop in ((lambda e: e.set_snapshots(**snapshot_plan), r"snapshot plan is active \(wv_set_snapshots\(e, NULL\)"),
                         (lambda e: e.set_spectrum([0.0], **snapshot_plan), r"spectrum plan is active \(wv_set_spectrum\(e, NULL, NULL\)"),
                         (lambda e: e.set_decay(4, 2, **snapshot_plan), r"a decay plan is active \(wv_set_decay\(e, NULL\)"),
                         (lambda e: e.set_decay(4, 2, bands=bands, **snapshot_plan), r"banded decay plan is active \(wv_set_decay_bands\(e, NULL, NULL, 0, 0\)")):
        eng = make_engine(case, "f64")
        setter(eng)
        assert eng.run_steps(2) == (2, 0)
        with pytest.raises(E.WaveguideError, match="error -6: wv_set_intensity: .*" + stop):
            eng.set_intensity(4, 2, **plan, **c)
        with pytest.raises(E.WaveguideError, match="error -6: .*no intensity plan"):
            eng.fetch_intensity()
        assert eng.run_steps(2) == (2, 0)
        eng.close()
    # a slab of a chain
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
        slab.set_intensity(2, 2, box=((1, 1, 1), (4, 4, 1)), **c)
    slab.close()
    # no plan: the library's WV_E_STATE; a group takes no engine with a plan
    eng = E.Engine(mesh, precision="f32")
    with pytest.raises(E.WaveguideError, match="error -6: .*no intensity plan"):
        eng.fetch_intensity_velocity()
    with pytest.raises(E.WaveguideError, match="error -6: .*no directional receivers"):
        eng.fetch_directional_velocity(1)
    group = E.LocalSlabGroup([eng])
    eng.set_intensity(2, 2, box=((1, 1, 1), (4, 4, 1)), **c)
    with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no intensity bins"):
        group.run_steps(4)
    eng.set_intensity(None)
    assert group.run_steps(4) == (4, 0)
    group.close()


@pytest.mark.parametrize("captures", FILE_COUNTS["intensity"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("intensity", captures)


@pytest.mark.parametrize("form", FILE_FORMS["intensity"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("intensity", tag, form)


def test_canonical_returns_the_bins_beside_the_receiver_output():
    """simulation.canonical(..., intensity=dict(plane=, every=, n_bins=)): the records are those of a run without a plan, the bins are
    the definition's over canonical's own snapshots of the plane's hull at the same cadence, with the mesh's spacing, sample_rate / every
    and the environment's density filled in; a second plan beside it is refused with the engine's message."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    plan = dict(box=((1, 1, 11), (22, 22, 1)), period=3)    # (an odd period: after an impulse alone even steps only would see one parity of the mesh, and I = 0)
    hplan, box_in_hull = hull_of(plan)
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=hplan)
    bands, (bins, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                          intensity=dict(plane=11 * vm.mesh.spacing, every=3, n_bins=5))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 14 == len(steps) and bins.shape == (4, 5, 1, 22, 22)
    want = I.intensity_bins(fields, box_in_hull, vm.mesh.spacing, rate / 3, env.ambient_density, 5, 3)
    assert bins.tobytes() == want.tobytes() and all(np.abs(bins[a]).max() > 0 for a in range(4))
    with pytest.raises(E.WaveguideError, match="error -6: .*snapshot plan is active"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, snapshots=dict(period=8), intensity=dict(plane=0.5))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, intensity=dict(plane=0.5))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, intensity=dict(plane=0.0))     # the floor: no node below it


def test_the_tool_writes_the_intensity_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --intensity-map --intensity-plane z=... --intensity-every --intensity-out FILE.npz on its built-in hall."""
    out = tmp_path / "intensity.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.03",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--intensity-map", "--intensity-plane", "z=1.5",
                        "--intensity-every", "1", "--intensity-bin-ms", "5", "--intensity-out", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        bins, times, direction, diffuse = f["bins"], f["times"], f["net_direction"], f["diffuseness"]
        captures, per_bin, period, rate, plane = int(f["captures"]), int(f["bin_captures"]), int(f["period"]), float(f["sample_rate"]), int(f["plane"])
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    assert bins.dtype == np.float64 and bins.shape == (4, -(-captures // per_bin), dims[1] - 2, dims[0] - 2)
    assert period == 1 and captures == steps + 1 and per_bin == max(1, int(round(0.005 * rate)))
    assert times.shape == (bins.shape[1],) and times[0] == 0 and abs(times[1] - per_bin / rate) < 1e-12 and 1 <= plane <= dims[2] - 2
    assert direction.shape == (3,) + bins.shape[2:] and diffuse.shape == bins.shape[2:]
    assert all(np.abs(bins[a]).max() > 0 for a in range(4)) and np.isfinite(diffuse).any()
    heard = np.isfinite(direction[0])
    assert heard.any() and np.allclose((direction[:, heard] ** 2).sum(axis=0), 1.0)


def test_the_rate_tool_runs_and_its_two_ways_agree_bytewise(tmp_path):
    """tools/intensity_rate.py on a 48^3 room, 48 steps per repeat: every row is there; the plan's E planes equal a decay plan's and
    its velocities equal the receiver-per-node way's bytewise (where the two are defined to agree: period 1); the receiver way's
    records, summed on the host, equal the definition's sums of rounded products; and the figures land in the JSON file.  (Whether
    the bar holds is a matter of the 256^3 run, not of this size: the exit status may say either.)"""
    out = tmp_path / "rate.json"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "intensity_rate.py"), "--side", "48", "--steps", "48",
                        "--bin-captures", "5", "--json", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode in (0, 1), p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFER" not in p.stdout and p.stdout.count("bytewise equal") == 3 and "INTENSITY RATE" in p.stdout, p.stdout
    report = json.load(open(str(out)))
    assert sorted(report["f64"]["rows"]) == sorted(["no plan", "plan every 1", "plan every 3", "receivers every 1"])
    assert all(report["f64"]["bytewise"].values()) and len(report["f64"]["bytewise"]) == 3
    assert report["f64"]["fold"]["model_bytes"] > 0 and report["f64"]["fold"]["launches"] > 0 and report["f64"]["gather"]["launches"] > 0

"""Field spectra accumulated on the device while wv_run keeps going (wv_set_spectrum; csrc/spectrum_kernels.hip.h,
engine_spectrum.hip.h).  The reference of every comparison is a second, identical engine with a SNAPSHOT plan of the same box and
cadence, whose snapshots are folded in NumPy in capture order with twiddles from spectrum_twiddle: `a + p * c` on float64 arrays is
a rounded product and a rounded sum, which is the definition.  Equality is BYTEWISE.  Small meshes, forms forced, a few dozen steps."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from helpers import numpy_fold, set_tuning
from plan_cases import (BOXES, FILE_COUNTS, FILE_FORMS, FORMS, FORM_CASES, box_scene, capture_counts, changes_nothing,
                        check, default_tuning_afterwards, make_engine, plan_on)
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQS5 = [0.0, 0.5, 0.125, 0.0371, 1.0 / 3.0]


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    default_tuning_afterwards()


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_fold_of_the_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes, periods that do and do not divide 2 and 3: one plane of the 32^3 impulse
    room, K = 5 with f = 0 and f = 0.5 among them.  At f = 0 the real part is the plain ordered sum and the imaginary part is zero."""
    n_steps = 64 if form == "graph" else 30
    plan = plan_on("impulse_flat", "spectrum", box=((0, 0, 15), (None, None, 1)), period=period, freqs=FREQS5)
    got, _, _, snaps, _ = check("spectrum", "impulse_flat", tag, form, plan, n_steps, query)
    got = got["spectrum"]
    plain = np.zeros(snaps.shape[1:])
    for p in snaps:
        plain = plain + p.astype(np.float64)
    assert got[0].real.tobytes() == plain.tobytes()
    assert got[0].imag.tobytes() == np.zeros_like(plain).tobytes()


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; every step captured, 21 captures
    (more than the stage holds), three-step passes forced (which then run as single steps: every step ends a pass)."""
    check("spectrum", "random", tag, "triple", plan_on("random", "spectrum", freqs=FREQS5, period=1, **BOXES[name]), 20)


@pytest.mark.parametrize("n_freqs", [1, 3, 4, 5, 9, 64])
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_numbers_of_frequencies_around_the_chunk(name, n_freqs):
    """The fold kernel walks the frequencies in chunks of 4: one frequency, 3 / 4 / 5 around a chunk, 9 (two chunks and one), the
    maximum; with two nodes per lane and with one."""
    freqs = [0.25] if n_freqs == 1 else list(np.linspace(0.0, 0.5, n_freqs))
    check("spectrum", "random", "f64", "pair", plan_on("random", "spectrum", freqs=freqs, period=1, **BOXES[name]), 20)


def test_refusals_leave_an_earlier_plan_intact():
    """n_freqs 0 and 65, f = 0.6, a NaN, a box off the mesh: WV_E_INVALID_ARGUMENT; a snapshot plan while a spectrum plan is active:
    WV_E_STATE; the earlier plan's sums are what they were and it goes on capturing."""
    set_tuning(**FORMS["single"])
    case = cases.CASES["random"]()
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    eng = make_engine(case, "f64")
    eng.set_spectrum(FREQS5, **plan)
    assert eng.run_steps(5) == (5, 0)
    before, before_count = eng.fetch_spectrum()
    for bad_freqs in ([], list(np.linspace(0, 0.5, 65)), [0.1, 0.6], [0.1, float("nan")], [-0.01]):
        with pytest.raises(E.WaveguideError, match="error -1: "):
            eng.set_spectrum(bad_freqs, **plan)
    for bad_box in (((0, 0, 0), (25, 20, 28)), ((-1, 0, 0), (4, 4, 4)), ((0, 0, 28), (1, 1, 1))):
        with pytest.raises(E.WaveguideError, match="error -1: .*leaves the mesh"):
            eng.set_spectrum(FREQS5, box=bad_box)
    with pytest.raises(E.WaveguideError, match="error -1: .*stride"):
        eng.set_spectrum(FREQS5, box="mesh", stride=(1, 0, 1))
    with pytest.raises(E.WaveguideError, match="error -1: .*period"):
        eng.set_spectrum(FREQS5, box="mesh", period=0)
    with pytest.raises(E.WaveguideError, match="error -6: .*exclude each other"):
        eng.set_snapshots(**plan)
    after, after_count = eng.fetch_spectrum()
    assert after_count == before_count == 6 and after.tobytes() == before.tobytes() and np.abs(after).max() > 0
    assert eng.run_steps(3) == (3, 0) and eng.spectrum_count() == (9, 8)
    eng.close()
    # the other order: a snapshot plan is active
    eng = make_engine(case, "f64", plan)
    assert eng.run_steps(2) == (2, 0)
    with pytest.raises(E.WaveguideError, match="error -6: .*exclude each other"):
        eng.set_spectrum(FREQS5, **plan)
    assert eng.run_steps(2) == (2, 0) and list(eng.fetch_snapshots()[1]) == [0, 1, 2, 3, 4]
    eng.close()
    # a slab of a chain
    mesh = M.box_mesh(16, 12, 10)
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
        slab.set_spectrum([0.1], box=((0, 0, 0), (4, 4, 1)))
    slab.close()
    # no plan: the library's WV_E_STATE; a group takes no engine with a plan
    eng = E.Engine(mesh, precision="f32")
    with pytest.raises(E.WaveguideError, match="error -6: .*no spectrum plan"):
        eng.fetch_spectrum()
    group = E.LocalSlabGroup([eng])
    eng.set_spectrum([0.1], box=((0, 0, 0), (4, 4, 1)))
    with pytest.raises(E.WaveguideError, match="error -6: .*wv_run_group accumulates no spectra"):
        group.run_steps(4)
    eng.set_spectrum(None)
    assert group.run_steps(4) == (4, 0)
    group.close()


@pytest.mark.parametrize("captures", FILE_COUNTS["spectrum"])
def test_capture_counts_around_the_stage(captures):
    """One fold per 16 captures and one for the fetch at the most: plan_cases.capture_counts, at the counts this file always named
    (tests/test_gpu_plan_life_cycle.py has the others)."""
    capture_counts("spectrum", captures)


@pytest.mark.parametrize("form", FILE_FORMS["spectrum"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise:
    plan_cases.changes_nothing, in the forms this file always named."""
    changes_nothing("spectrum", tag, form)


def test_canonical_returns_the_spectrum_beside_the_receiver_output():
    """simulation.canonical(..., spectrum=...): Hz become cycles per step with the run's sample rate, the records are those of a run
    without a plan, and the spectrum is the engine-level one (the fold of canonical's own snapshots of the same box and cadence)."""
    set_tuning()
    W, vm, source, receiver = box_scene()
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    seconds = 39.5 / rate      # 40 steps
    box = ((0, 0, 12), (None, None, 1))
    freqs_hz = [0.0, 0.01 * rate, rate / 16.0, rate / 4.0]
    plain, (fields, steps) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", snapshots=dict(box=box, period=2))
    bands, (spectrum, captures) = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32",
                                              spectrum=dict(freqs_hz=freqs_hz, box=box, period=2))
    assert bands[0][0].tobytes() == plain[0][0].tobytes() and bands[0][1:] == plain[0][1:]
    assert captures == 21 and spectrum.shape == (4, 1, 24, 24)
    want = numpy_fold(fields, steps, list(np.asarray(freqs_hz) / rate))
    assert spectrum.tobytes() == want.tobytes() and np.abs(spectrum).max() > 0
    with pytest.raises(ValueError, match="aliases"):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, spectrum=dict(freqs_hz=[rate / 3.0], period=2))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, slabs=2, spectrum=dict(freqs_hz=[10.0]))
    with pytest.raises(ValueError):
        W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, snapshots=dict(period=8), spectrum=dict(freqs_hz=[10.0]))


def test_the_tool_writes_the_complex_maps_of_one_plane(tmp_path):
    """tools/impulse_response.py --spectrum HZ,HZ --spectrum-plane z=... --spectrum-out FILE.npz on its built-in hall, a short run."""
    out = tmp_path / "maps.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impulse_response.py"), "--cutoff", "100", "--seconds", "0.03",
                        "--precision", "f32", "--out", str(tmp_path / "ir.wav"), "--spectrum", "20,31.5,50", "--spectrum-plane", "z=1.5",
                        "--spectrum-out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(str(out)) as f:
        maps, freqs, captures, plane = f["spectrum"], f["freqs_hz"], int(f["captures"]), int(f["plane"])
    dims = [int(v) for v in p.stdout.split("mesh ")[1].split(" ")[0].split("x")]
    steps = int(p.stdout.split(" steps at")[0].split()[-1])
    assert maps.dtype == np.complex128 and maps.shape == (3, dims[1], dims[0]) and list(freqs) == [20.0, 31.5, 50.0]
    assert captures == steps + 1 and 0 <= plane < dims[2] and np.abs(maps).max() > 0


def test_the_rate_tool_runs_and_its_two_ways_agree_bitwise(tmp_path):
    """tools/spectrum_rate.py on a 48^3 room, 48 steps per repeat: every row is there for both precisions, the spectrum of the
    snapshot-and-host-fold way equals the spectrum plan's bytewise in both cases, and the figures land in the JSON file.  (Whether the
    bar holds is a matter of the 512^3 run, not of this size: the exit status may say either.)"""
    out = tmp_path / "rate.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "spectrum_rate.py"), "--side", "48", "--steps", "48", "--json", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode in (0, 1), p.stdout[-2000:] + p.stderr[-4000:]
    assert "DIFFERS" not in p.stdout and p.stdout.count("bitwise equal") == 4 and "SPECTRUM RATE" in p.stdout, p.stdout
    import json
    report = json.load(open(str(out)))
    for precision in ("f64", "f32"):
        assert sorted(report[precision]["rows"]) == ["a", "b field", "b plane", "c field", "c plane"]
        assert all(v["bitwise_equal_to_old"] for v in report[precision]["verdicts"].values())

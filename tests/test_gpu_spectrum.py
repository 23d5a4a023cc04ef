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
from test_gpu_snapshots import FORMS, make_engine
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQS5 = [0.0, 0.5, 0.125, 0.0371, 1.0 / 3.0]


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()



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


def spectrum_engine(case_name, tag, form, plan, freqs):
    set_tuning(**FORMS[form])
    eng = make_engine(cases.CASES[case_name](), tag)
    shape = eng.set_spectrum(freqs, **plan)
    return eng, shape


def check(case_name, tag, form, plan, freqs, n_steps, query=None):
    snaps, steps = reference_snapshots(case_name, tag, form, plan, n_steps)
    want = numpy_fold(snaps, steps, freqs)
    eng, shape = spectrum_engine(case_name, tag, form, plan, freqs)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert eng.spectrum_count() == (len(steps), int(steps[-1]))
        got, captures = eng.fetch_spectrum()
        if query is not None:
            assert eng.query(query) > 0
        assert eng.query(E.Engine.QUERY_SPECTRUM_CAPTURES) == len(steps)
        folds = eng.query(E.Engine.QUERY_SPECTRUM_FOLDS)
    finally:
        eng.close()
    assert captures == len(steps) and len(steps) > 1
    assert got.shape == shape == want.shape and got.dtype == np.complex128
    assert folds <= -(-len(steps) // 16) + 1
    assert got.tobytes() == want.tobytes(), "largest difference %g" % np.abs(got - want).max()
    assert np.abs(got).max() > 0 and np.abs(snaps[-1]).max() > 0   # (the comparison is not of zeros)
    return got, snaps


FORM_CASES = [("single", 1, None), ("single", 5, None), ("graph", 16, None),
              ("pair", 2, E.Engine.QUERY_PASSES), ("pair", 3, E.Engine.QUERY_PASSES), ("pair", 7, E.Engine.QUERY_PASSES),
              ("triple", 3, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 4, E.Engine.QUERY_TRIPLE_PASSES), ("triple", 7, E.Engine.QUERY_TRIPLE_PASSES)]


@pytest.mark.parametrize("form,period,query", FORM_CASES, ids=["%s-every%d" % c[:2] for c in FORM_CASES])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_every_stepping_form_gives_the_fold_of_the_snapshots(form, period, query, tag):
    """Single steps, graph replay, two- and three-step passes, periods that do and do not divide 2 and 3: one plane of the 32^3 impulse
    room, K = 5 with f = 0 and f = 0.5 among them.  At f = 0 the real part is the plain ordered sum and the imaginary part is zero."""
    n_steps = 64 if form == "graph" else 30
    got, snaps = check("impulse_flat", tag, form, dict(box=((0, 0, 15), (None, None, 1)), period=period), FREQS5, n_steps, query)
    plain = np.zeros(snaps.shape[1:])
    for p in snaps:
        plain = plain + p.astype(np.float64)
    assert got[0].real.tobytes() == plain.tobytes()
    assert got[0].imag.tobytes() == np.zeros_like(plain).tobytes()


BOXES = {
    "sub-box-630": dict(box=((3, 2, 4), (10, 9, 7))),             # not a multiple of 64, an odd number of rows; two nodes per lane
    "sub-box-567-odd": dict(box=((3, 2, 4), (9, 9, 7))),          # an odd B: one node per lane, three workgroups, a tail
    "sub-box-16-byte-rows": dict(box=((4, 1, 2), (16, 5, 3))),
    "every-face-stride-3": dict(box="mesh", stride=3),            # 24 / 3, 20 / 3 and 28 / 3: the last two do not divide
    "strides-1-2-3": dict(box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3)),
    "one-node": dict(box=((5, 6, 7), (1, 1, 1))),
}


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_boxes_and_strides_on_a_room_with_walls(name, tag):
    """tests/golden/cases.py "random": 24 x 20 x 28, six different wall filters, a soft source; every step captured, 21 captures
    (more than the stage holds), three-step passes forced (which then run as single steps: every step ends a pass)."""
    check("random", tag, "triple", dict(BOXES[name], period=1), FREQS5, 20)


@pytest.mark.parametrize("n_freqs", [1, 3, 4, 5, 9, 64])
@pytest.mark.parametrize("name", ["sub-box-630", "sub-box-567-odd"])
def test_numbers_of_frequencies_around_the_chunk(name, n_freqs):
    """The fold kernel walks the frequencies in chunks of 4: one frequency, 3 / 4 / 5 around a chunk, 9 (two chunks and one), the
    maximum; with two nodes per lane and with one."""
    freqs = [0.25] if n_freqs == 1 else list(np.linspace(0.0, 0.5, n_freqs))
    check("random", "f64", "pair", dict(BOXES[name], period=1), freqs, 20)


@pytest.mark.parametrize("captures", [1, 16, 17, 33])
def test_capture_counts_around_the_stage(captures):
    """Runs that take exactly 1, 16, 17 and 33 captures: one fold per 16 captures and one for the fetch at the most."""
    n_steps = captures - 1
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    eng, _ = spectrum_engine("random", "f64", "single", plan, FREQS5)
    try:
        assert eng.run_steps(n_steps) == (n_steps, 0)
        assert eng.spectrum_count() == (captures, n_steps)
        assert eng.query(E.Engine.QUERY_SPECTRUM_FOLDS) <= (captures - 1) // 16   # (nothing is folded merely because a run ended)
        got, count = eng.fetch_spectrum()
        assert count == captures == eng.query(E.Engine.QUERY_SPECTRUM_CAPTURES)
        assert eng.query(E.Engine.QUERY_SPECTRUM_FOLDS) <= -(-captures // 16) + 1
    finally:
        eng.close()
    snaps, steps = reference_snapshots("random", "f64", "single", plan, 32)
    assert got.tobytes() == numpy_fold(snaps[:captures], steps[:captures], FREQS5).tobytes()


@pytest.mark.parametrize("form", ["single", "triple"])
def test_calls_of_1_7_and_30_steps_give_the_same_bytes(form):
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=2)
    out = []
    for call in (1, 7, 30):
        eng, _ = spectrum_engine("random", "f32", form, plan, FREQS5)
        left = 30
        while left:
            n = min(call, left)
            assert eng.run_steps(n) == (n, 0)
            left -= n
        out.append(eng.fetch_spectrum())
        eng.close()
    snaps, steps = reference_snapshots("random", "f32", form, plan, 30)
    want = numpy_fold(snaps, steps, FREQS5)
    for got, count in out:
        assert count == 16 and got.tobytes() == want.tobytes()


def test_fetching_mid_run_and_at_the_end():
    plan = dict(box=((3, 2, 4), (10, 9, 7)), period=1)
    eng, _ = spectrum_engine("random", "f64", "pair", plan, FREQS5)
    assert eng.run_steps(13) == (13, 0)
    mid, mid_count = eng.fetch_spectrum()
    again, again_count = eng.fetch_spectrum()
    assert eng.run_steps(17) == (17, 0)
    end, end_count = eng.fetch_spectrum()
    eng.close()
    snaps, steps = reference_snapshots("random", "f64", "pair", plan, 30)
    assert (mid_count, again_count, end_count) == (14, 14, 31)
    assert mid.tobytes() == again.tobytes() == numpy_fold(snaps[:14], steps[:14], FREQS5).tobytes()
    assert end.tobytes() == numpy_fold(snaps, steps, FREQS5).tobytes()


@pytest.mark.parametrize("form", ["single", "triple"])
@pytest.mark.parametrize("bad_step", [12, 13, 14])
def test_a_run_that_stops_on_a_flag_folds_no_capture_of_a_later_step(form, bad_step):
    """inf in the source signal at step f: the run completes f steps; with a capture every 4 steps the sums hold those of 0, 4, 8, 12
    and nothing of 16 (whose field the batch had already produced when the flag was read)."""
    set_tuning(**FORMS[form])
    mesh = M.box_mesh(12, 12, 12)
    sig = np.zeros(40)
    sig[0] = 1.0
    sig[bad_step] = np.inf
    case = dict(mesh=mesh, init=None, source_kind=E.SOURCE_HARD, source_node=mesh.compute_index(6, 6, 6), signal=sig,
                recv=[mesh.compute_index(7, 6, 6)])
    plan = dict(box=((0, 0, 6), (None, None, 1)), period=4)
    ref = make_engine(case, "f64", plan)
    done, flag = ref.run_steps(40)
    assert done == bad_step and flag & M.ERR_INF
    snaps, steps = ref.fetch_snapshots()
    ref.close()
    assert list(steps) == [0, 4, 8, 12]
    eng = make_engine(case, "f64")
    eng.set_spectrum(FREQS5, **plan)
    done, flag = eng.run_steps(40)
    assert done == bad_step and flag & M.ERR_INF
    assert eng.spectrum_count() == (4, 12)
    got, count = eng.fetch_spectrum()
    eng.close()
    assert count == 4 and np.isfinite(got.view(np.float64)).all() and np.abs(got).max() > 0
    assert got.tobytes() == numpy_fold(snaps, steps, FREQS5).tobytes()


@pytest.mark.parametrize("form", ["single", "triple"])
def test_checkpoint_run_rollback_rerun_gives_the_same_sums_twice(form):
    plan = dict(box=((2, 3, 4), (12, 11, 9)), stride=(1, 2, 2), period=5)
    eng, _ = spectrum_engine("random", "f64", form, plan, FREQS5)
    assert eng.run_steps(10) == (10, 0)            # captures of 0, 5, 10
    eng.checkpoint()
    assert eng.run_steps(17) == (17, 0)            # 15, 20, 25
    first, first_count = eng.fetch_spectrum()
    eng.rollback()
    assert eng.step_count() == 10 and eng.spectrum_count() == (3, 10)
    kept, kept_count = eng.fetch_spectrum()
    assert eng.run_steps(17) == (17, 0)
    second, second_count = eng.fetch_spectrum()
    assert eng.spectrum_count() == (6, 25)
    # a plan set after the checkpoint has no sums to go back to
    eng.set_spectrum(FREQS5, **plan)
    with pytest.raises(E.WaveguideError, match="error -6: .*after the checkpoint"):
        eng.rollback()
    eng.close()
    snaps, steps = reference_snapshots("random", "f64", form, plan, 27)
    assert (first_count, kept_count, second_count) == (6, 3, 6)
    assert kept.tobytes() == numpy_fold(snaps[:3], steps[:3], FREQS5).tobytes()
    assert first.tobytes() == second.tobytes() == numpy_fold(snaps, steps, FREQS5).tobytes()


def test_generic_steps_in_between_capture_nothing():
    """wv_step / wv_swap capture nothing and the plan steps they pass are passed; a plan set at a non-zero step count captures that
    very step at the next run."""
    set_tuning(**FORMS["pair"])
    case = cases.CASES["random"]()
    plan = dict(box=((0, 0, 0), (None, None, 2)), period=3)
    engines = [make_engine(case, "f32"), make_engine(case, "f32")]
    for e in engines:
        assert e.run_steps(9) == (9, 0)
    engines[0].set_spectrum(FREQS5, **plan)           # steps 0, 3, 6 lie before the plan; 9 is the count it is set at
    engines[1].set_snapshots(**plan)
    assert engines[0].spectrum_count() == (0, 0)
    for e in engines:
        assert e.run_steps(4) == (4, 0)               # 9 (at the start of this run), 12
        for _ in range(3):                            # 13 -> 16 by generic steps: 15 is passed
            assert e.step() == 0
            e.swap()
    assert engines[0].spectrum_count() == (2, 12)
    for e in engines:
        assert e.run_steps(2) == (2, 0)               # 18
    got, count = engines[0].fetch_spectrum()
    snaps, steps = engines[1].fetch_snapshots()
    assert list(steps) == [9, 12, 18] and count == 3
    assert got.tobytes() == numpy_fold(snaps, steps, FREQS5).tobytes() and np.abs(got).max() > 0
    engines[0].set_spectrum(None)                     # stops and forgets
    with pytest.raises(E.WaveguideError, match="error -6: .*no spectrum plan"):
        engines[0].spectrum_count()
    assert engines[0].run_steps(3) == (3, 0)
    for e in engines:
        e.close()


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


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_plan_changes_nothing_the_run_computes(form, tag):
    """Receiver traces, final current / previous and the filter memories with a plan equal those without one, bytewise."""
    set_tuning(**FORMS[form])
    case = cases.CASES["random"]()
    out = []
    for plan in (None, dict(box="mesh", stride=(1, 2, 1), period=7, first_step=3)):
        eng = make_engine(case, tag)
        if plan:
            eng.set_spectrum(FREQS5, **plan)
        assert eng.run_steps(case["steps"]) == (case["steps"], 0)
        out.append([eng.fetch_receivers(0, case["steps"]), eng.read_field(E.BUF_CURRENT), eng.read_field(E.BUF_PREVIOUS)] +
                   [eng.read_boundary_data(d) for d in (1, 2, 3)])
        if plan:
            assert eng.spectrum_count() == (9, 59)   # steps 3, 10, ..., 59
        eng.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


def test_kernel_timing_accounts_for_the_fold_kernels():
    eng, _ = spectrum_engine("impulse_flat", "f64", "single", dict(box="mesh", period=1), FREQS5)
    eng.enable_kernel_timing(True)
    assert eng.run_steps(20) == (20, 0)
    eng.fetch_spectrum()
    assert eng.query(E.Engine.QUERY_SPECTRUM_FOLDS) == 2 and eng.query(E.Engine.QUERY_SPECTRUM_NS) > 0
    eng.close()


def _box_scene():
    from wayverb_amd import simulation as W
    mesh = M.box_mesh(24, 24, 24, coefficients=np.array([M.flat_coefficients(0.1)], dtype=M.coefficients_dtype))
    vm = W.VoxelsAndMesh(None, None, 0, None, None, mesh, (0.0, 0.0, 0.0))
    sp = mesh.spacing
    return W, vm, (12 * sp, 12 * sp, 12 * sp), (15 * sp, 12 * sp, 12 * sp)


def test_canonical_returns_the_spectrum_beside_the_receiver_output():
    """simulation.canonical(..., spectrum=...): Hz become cycles per step with the run's sample rate, the records are those of a run
    without a plan, and the spectrum is the engine-level one (the fold of canonical's own snapshots of the same box and cadence)."""
    set_tuning()
    W, vm, source, receiver = _box_scene()
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

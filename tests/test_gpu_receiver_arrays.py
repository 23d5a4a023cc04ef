"""Receiver arrays: the wide receiver gather (csrc/receiver_kernels.hip.h; more than 64 columns) and directional receivers recorded
and integrated on the device (wv_set_directional_receivers; csrc/engine_directional.hip.h).  Every comparison is BITWISE, and the
expected side always comes from the path that was there before: columns recorded at most 64 at a time on fresh engines of the same
case (one wave serves them, pre_post_kernel), integrated by postprocess.directional_receiver on the host.  Small meshes, forms forced
as tests/test_gpu_snapshots.py forces them, 30-38 steps."""
import functools

import numpy as np
import pytest

import cases
from helpers import initial_fields, set_tuning
from test_gpu_parity import _random_case
from test_gpu_snapshots import FORMS
from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd import postprocess as P
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

STEPS = 30
FORM_QUERY = {"single": None, "graph": None, "pair": E.Engine.QUERY_PASSES, "triple": E.Engine.QUERY_TRIPLE_PASSES}
WIDTHS = (65, 70, 259, 1000)
# what canonical() hands the integrator for a 200 Hz / 0.6 waveguide: the numbers only scale the records
SPACING, SAMPLE_RATE, DENSITY = float(np.float32(0.4417)), 1333.3333333333333, 400.0 / 340.0


@pytest.fixture(autouse=True)
def _default_tuning_afterwards(built_library):
    yield
    set_tuning()


@functools.lru_cache(maxsize=None)
def the_case(name, source_kind):
    case = cases.CASES["impulse_flat"]() if name == "impulse_flat" else _random_case((24, 20, 28), seed=72, steps=64)
    case = dict(case)
    case["source_kind"] = source_kind
    if name == "impulse_flat":       # (a soft source on a silent field would be a hard one: give it something to add to)
        case["signal"] = np.random.default_rng(5).uniform(-0.1, 0.1, case["steps"])
    return case


def make_engine(case, tag):
    eng = E.Engine(case["mesh"], precision=tag)
    if case["init"] is not None:
        prev, cur = initial_fields(case, eng.dtype)
        eng.write_field(prev, E.BUF_PREVIOUS)
        eng.write_field(cur, E.BUF_CURRENT)
    eng.set_source(case["source_kind"], case["source_node"], case["signal"])
    return eng


@functools.lru_cache(maxsize=None)
def column_list(name):
    """1000 columns with a fixed seed from ALL nodes of the mesh (inside, boundary, outside); its first 65 hold the source node, its
    six neighbours, wall / edge / corner nodes, duplicates and UINT64_MAX entries, so every prefix in WIDTHS has them."""
    mesh = the_case(name, 1)["mesh"]
    src = the_case(name, 1)["source_node"]
    rng = np.random.default_rng(2024)
    t = mesh.nodes["boundary_type"]
    boundary = np.flatnonzero((t != 0) & ((t & (M.ID_INSIDE | M.ID_REENTRANT)) == 0))
    special = [src] + list(mesh.compute_neighbors(src)) + [E.NO_NODE, src, E.NO_NODE] + [int(b) for b in rng.choice(boundary, 12)]
    special += special[7:12]                                             # duplicates of boundary nodes and of a UINT64_MAX entry
    cols = special + [int(v) for v in rng.integers(0, mesh.num_nodes, 1000 - len(special))]
    assert len(cols) == 1000 and len(special) < 65
    return tuple(cols)


def record(case, tag, columns, steps=STEPS, calls=None):
    eng = make_engine(case, tag)
    try:
        eng.set_receivers(np.array(columns, dtype=np.uint64))
        for n in calls or (steps,):
            assert eng.run_steps(n) == (n, 0)
        total = sum(calls) if calls else steps
        return eng.fetch_receivers(0, total), {q: eng.query(q) for q in (E.Engine.QUERY_WIDE_GATHERS, E.Engine.QUERY_PASSES,
                                                                         E.Engine.QUERY_TRIPLE_PASSES)}
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def narrow_reference(name, source_kind, form, tag, chunk=64):
    """The 1000 columns recorded `chunk` at a time on fresh engines: the path every engine took before receiver arrays."""
    set_tuning(**FORMS[form])
    case = the_case(name, source_kind)
    cols = column_list(name)
    parts = []
    for a in range(0, len(cols), chunk):
        got, queries = record(case, tag, cols[a:a + chunk])
        assert queries[E.Engine.QUERY_WIDE_GATHERS] == 0
        if FORM_QUERY[form] is not None:
            assert queries[FORM_QUERY[form]] > 0
        parts.append(got)
    out = np.concatenate(parts, axis=1)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("source_kind", [E.SOURCE_HARD, E.SOURCE_SOFT], ids=["hard", "soft"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["impulse_flat", "random_24x20x28"])
def test_wide_gather_records_what_the_narrow_path_records(name, form, tag, source_kind, width):
    want = narrow_reference(name, source_kind, form, tag)[:, :width]
    set_tuning(**FORMS[form])
    got, queries = record(the_case(name, source_kind), tag, column_list(name)[:width])
    assert queries[E.Engine.QUERY_WIDE_GATHERS] > 0
    if FORM_QUERY[form] is not None:
        assert queries[FORM_QUERY[form]] > 0
    assert got.shape == want.shape == (STEPS, width)
    for c in range(width):
        assert got[:, c].tobytes() == want[:, c].tobytes(), "column %d (node %d) differs" % (c, column_list(name)[c])
    assert np.abs(got).max() > 0
    none = [c for c, node in enumerate(column_list(name)[:width]) if node == E.NO_NODE]
    assert none and not got[:, none].any()


def test_64_columns_stay_on_the_narrow_path_and_65_leave_it():
    set_tuning(**FORMS["single"])
    case = the_case("impulse_flat", E.SOURCE_HARD)
    for width, wide in ((63, False), (64, False), (65, True)):
        _, queries = record(case, "f32", column_list("impulse_flat")[:width], steps=4)
        assert (queries[E.Engine.QUERY_WIDE_GATHERS] > 0) == wide
        if wide:
            assert queries[E.Engine.QUERY_WIDE_GATHERS] == 4      # one per step


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_two_slabs_with_259_columns_equal_the_whole_mesh(tag):
    set_tuning()
    case = the_case("random_24x20x28", E.SOURCE_SOFT)
    cols = list(column_list("random_24x20x28")[:259])
    signal = case["signal"][:STEPS]
    eng = E.Engine(case["mesh"], precision=tag)
    try:
        done, whole = E.run_fast(eng, case["source_kind"], case["source_node"], signal, cols)
        assert eng.query(E.Engine.QUERY_WIDE_GATHERS) > 0
    finally:
        eng.close()
    done2, slabs = E.run_fast_slabs(case["mesh"], 2, case["source_kind"], case["source_node"], signal, cols, precision=tag)
    assert done == done2 == STEPS and slabs.tobytes() == whole.tobytes() and np.abs(whole).max() > 0


# ---- directional receivers on the device ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def centres(name="impulse_flat"):
    """100 centres with all six neighbours on the grid, fixed seed: the source node, nodes next to it, nodes one layer inside the
    walls, a duplicate."""
    case = the_case(name, 1)
    nx, ny, nz = case["mesh"].dims
    ci = case["mesh"].compute_index
    rng = np.random.default_rng(77)
    sx, sy, sz = 16, 16, 16
    first = [ci(19, 16, 16), ci(sx, sy, sz), ci(sx + 1, sy, sz), ci(1, 1, 1), ci(nx - 2, ny - 2, nz - 2), ci(1, 16, 30), ci(19, 16, 16)]
    rest = [ci(int(x), int(y), int(z)) for x, y, z in zip(rng.integers(1, nx - 1, 93), rng.integers(1, ny - 1, 93), rng.integers(1, nz - 1, 93))]
    return tuple(first + rest)


def columns_of(mesh, nodes):
    out = []
    for c in nodes:
        out += [c] + list(mesh.compute_neighbors(c))
    return out


CALLS = (1, 7, 30)


@functools.lru_cache(maxsize=None)
def host_records(form, tag, source_kind=E.SOURCE_HARD):
    """The 100 receivers as they were served before: their 700 columns recorded 63 at a time (nine receivers) on fresh engines, each
    receiver's seven integrated by postprocess.directional_receiver.  [steps, 100] records."""
    set_tuning(**FORMS[form])
    case = the_case("impulse_flat", source_kind)
    cols = columns_of(case["mesh"], centres())
    parts = []
    for a in range(0, len(cols), 63):
        got, queries = record(case, tag, cols[a:a + 63], calls=CALLS)
        assert queries[E.Engine.QUERY_WIDE_GATHERS] == 0
        parts.append(got)
    traces = np.concatenate(parts, axis=1)
    out = np.stack([P.directional_receiver(traces[:, 7 * i:7 * i + 7], SPACING, SAMPLE_RATE, DENSITY) for i in range(len(centres()))], axis=1)
    out.setflags(write=False)
    return out


def directional_engine(case, tag, nodes):
    eng = make_engine(case, tag)
    eng.set_directional_receivers(np.array(nodes, dtype=np.uint64), SPACING, SAMPLE_RATE, DENSITY)
    return eng


@pytest.mark.parametrize("n", [1, 3, 37, 100])
@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_device_integrator_equals_the_host_integration_of_the_columns(form, tag, n):
    """wv_run calls of 1, 7 and 30 steps: the velocities carry from batch to batch."""
    want = host_records(form, tag)[:, :n]
    set_tuning(**FORMS[form])
    eng = directional_engine(the_case("impulse_flat", E.SOURCE_HARD), tag, centres()[:n])
    try:
        for k in CALLS:
            assert eng.run_steps(k) == (k, 0)
        got = eng.fetch_directional(0, sum(CALLS))
        assert eng.query(E.Engine.QUERY_DIRECTIONAL_LAUNCHES) >= len(CALLS)
        assert (eng.query(E.Engine.QUERY_WIDE_GATHERS) > 0) == (7 * n > 64)
        if FORM_QUERY[form] is not None:
            assert eng.query(FORM_QUERY[form]) > 0
    finally:
        eng.close()
    assert got.shape == want.shape == (sum(CALLS), n) and got.dtype == P.directional_output_dtype
    for r in range(n):
        assert got[:, r].tobytes() == want[:, r].tobytes(), "receiver %d differs" % r
    assert np.abs(got["intensity"]).max() > 0 and np.abs(got["pressure"]).max() > 0


@pytest.mark.parametrize("form", ["single", "triple"])
def test_checkpoint_and_rollback_put_the_velocities_back(form):
    set_tuning(**FORMS[form])
    case = the_case("impulse_flat", E.SOURCE_HARD)
    nodes = centres()[:11]                 # 77 columns: the wide gather too
    straight = directional_engine(case, "f64", nodes)
    eng = directional_engine(case, "f64", nodes)
    try:
        assert straight.run_steps(5 + 12) == (17, 0)
        want = straight.fetch_directional(0, 17)
        assert eng.run_steps(5) == (5, 0)
        eng.checkpoint()
        assert eng.run_steps(12) == (12, 0)
        first = eng.fetch_directional(0, 17)
        eng.rollback()
        assert eng.step_count() == 5
        with pytest.raises(E.WaveguideError, match="error -1: .*not recorded yet"):
            eng.fetch_directional(0, 6)
        assert eng.run_steps(12) == (12, 0)
        second = eng.fetch_directional(0, 17)
    finally:
        straight.close()
        eng.close()
    assert first.tobytes() == second.tobytes() == want.tobytes() and np.abs(want["intensity"][5:]).max() > 0


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_run_that_stops_on_a_flag_keeps_the_completed_steps(tag):
    set_tuning(**FORMS["single"])
    case = dict(the_case("impulse_flat", E.SOURCE_HARD))
    case["signal"] = case["signal"].copy()
    case["signal"][9] = np.inf
    nodes = centres()[:10]
    cols = columns_of(case["mesh"], nodes)
    plain = make_engine(case, tag)
    eng = directional_engine(case, tag, nodes)
    try:
        plain.set_receivers(np.array(cols[:63], dtype=np.uint64))
        done, flag = plain.run_steps(STEPS)
        assert 0 < done < STEPS and flag & M.ERR_INF
        traces = plain.fetch_receivers(0, done)
        assert eng.run_steps(STEPS) == (done, flag)
        got = eng.fetch_directional(0, done)
        with pytest.raises(E.WaveguideError, match="error -1: .*not recorded yet"):
            eng.fetch_directional(0, done + 1)
    finally:
        plain.close()
        eng.close()
    for r in range(9):                     # (the receivers whose seven columns the narrow engine recorded)
        want = P.directional_receiver(traces[:, 7 * r:7 * r + 7], SPACING, SAMPLE_RATE, DENSITY)
        assert got[:, r].tobytes() == want.tobytes()


def test_steps_driven_from_outside_record_nan_rows_and_leave_the_velocities_alone():
    set_tuning(**FORMS["single"])
    case = the_case("impulse_flat", E.SOURCE_HARD)
    nodes = centres()[:9]
    cols = columns_of(case["mesh"], nodes)
    plain = make_engine(case, "f64")
    eng = directional_engine(case, "f64", nodes)
    try:
        plain.set_receivers(np.array(cols, dtype=np.uint64))
        for e in (plain, eng):
            assert e.run_steps(4) == (4, 0)
            for _ in range(2):
                assert e.step() == 0
                e.swap()
            assert e.run_steps(6) == (6, 0)
        traces = plain.fetch_receivers(0, 12)
        got = eng.fetch_directional(0, 12)
    finally:
        plain.close()
        eng.close()
    assert np.isnan(traces[4:6]).all() and not np.isnan(traces[[0, 1, 2, 3, 6, 7, 8, 9, 10, 11]]).any()
    kept = np.delete(traces, [4, 5], axis=0)
    for r in range(len(nodes)):
        want = P.directional_receiver(kept[:, 7 * r:7 * r + 7], SPACING, SAMPLE_RATE, DENSITY)
        assert np.isnan(got["intensity"][4:6, r]).all() and np.isnan(got["pressure"][4:6, r]).all()
        assert np.delete(got[:, r], [4, 5]).tobytes() == want.tobytes()
    assert np.abs(np.delete(got, [4, 5], axis=0)["intensity"]).max() > 0


def test_refusals():
    set_tuning(**FORMS["single"])
    case = the_case("impulse_flat", E.SOURCE_HARD)
    mesh = case["mesh"]
    ci = mesh.compute_index
    eng = make_engine(case, "f32")
    text = "Can't place directional_receiver at this node as it is adjacent to a boundary."
    try:
        eng.set_receivers([ci(16, 16, 16), ci(3, 3, 3)])
        assert eng.run_steps(3) == (3, 0)
        for bad in (ci(0, 5, 5), ci(31, 5, 5), ci(5, 0, 5), ci(5, 31, 5), ci(5, 5, 0), ci(5, 5, 31)):
            nodes = np.array([ci(8, 8, 8), bad], dtype=np.uint64)
            assert eng.lib.wv_set_directional_receivers(eng.h, nodes.ctypes.data, 2, SPACING, SAMPLE_RATE, DENSITY) == -1
            assert eng.lib.wv_last_error().decode() == text
        with pytest.raises(E.WaveguideError, match="error -1: .*outside the mesh"):
            eng.set_directional_receivers([mesh.num_nodes], SPACING, SAMPLE_RATE, DENSITY)
        with pytest.raises(E.WaveguideError, match="error -6"):
            eng.fetch_directional(0, 1)
        # the refused calls left the running engine as it was: its two columns go on
        assert eng.n_recv == 2 and eng.run_steps(3) == (3, 0)
        before = eng.fetch_receivers(0, 6)
        want, _ = record(case, "f32", [ci(16, 16, 16), ci(3, 3, 3)], steps=6)
        assert before.tobytes() == want.tobytes() and np.abs(before).max() > 0
        # directional mode: columns are not fetchable; set_receivers gives columns mode back
        eng.set_directional_receivers([ci(8, 8, 8)], SPACING, SAMPLE_RATE, DENSITY)
        assert eng.run_steps(2) == (2, 0) and eng.fetch_directional(6, 2).shape == (2, 1)
        out = np.zeros((2, 7))
        assert eng.lib.wv_fetch_receivers(eng.h, 6, 2, out.ctypes.data) == -6
        eng.set_receivers([ci(16, 16, 16)])
        assert eng.run_steps(2) == (2, 0) and eng.fetch_receivers(8, 2).shape == (2, 1)
        with pytest.raises(E.WaveguideError, match="error -6"):
            eng.fetch_directional(8, 2)
        # ... and so does an empty directional list
        eng.set_directional_receivers([ci(8, 8, 8)], SPACING, SAMPLE_RATE, DENSITY)
        eng.set_directional_receivers([], SPACING, SAMPLE_RATE, DENSITY)
        with pytest.raises(E.WaveguideError, match="error -6"):
            eng.fetch_directional(10, 0)
    finally:
        eng.close()
    layout = SlabLayout(mesh.dims, 0, 2)
    slab = E.Engine(slab_mesh(mesh, layout), precision="f32", ghost_lo=layout.ghost_lo, ghost_hi=layout.ghost_hi)
    try:
        with pytest.raises(E.WaveguideError, match="error -6: .*slab of a chain"):
            slab.set_directional_receivers([slab.mesh.compute_index(8, 8, 4)], SPACING, SAMPLE_RATE, DENSITY)
    finally:
        slab.close()


# ---- the callers' layer ------------------------------------------------------------------------------------------------------------
def test_canonical_many_equals_canonical_per_receiver():
    from wayverb_amd import simulation as W
    set_tuning()
    mesh = M.box_mesh(24, 24, 24, coefficients=np.array([M.flat_coefficients(0.1)], dtype=M.coefficients_dtype))
    vm = W.VoxelsAndMesh(None, None, 0, None, None, mesh, (0.0, 0.0, 0.0))
    env = W.Environment()
    sp = mesh.spacing
    source = (12 * sp, 12 * sp, 12 * sp)
    receivers = [(15 * sp, 12 * sp, 12 * sp), (12 * sp, 12 * sp, 12 * sp), (2 * sp, 3 * sp, 21 * sp), (12 * sp, 13 * sp, 12 * sp),
                 (20 * sp, 20 * sp, 5 * sp)]
    seconds = 39.5 / W.compute_sample_rate(sp, env.speed_of_sound)      # 40 steps
    want = [W.canonical(vm, source, r, env, 100.0, 0.6, seconds, precision="f32") for r in receivers]
    for slabs in (1, 2):
        got = W.canonical_many(vm, source, receivers, env, 100.0, 0.6, seconds, precision="f32", slabs=slabs)
        assert len(got) == len(receivers)
        for g, w in zip(got, want):
            assert len(g) == 1 and g[0][0].shape == (40,) and g[0][0].dtype == P.directional_output_dtype
            assert g[0][0].tobytes() == w[0][0].tobytes() and g[0][1:] == w[0][1:]
    assert np.abs(want[2][0][0]["intensity"]).max() > 0
    assert W.canonical_many(vm, source, receivers, env, 100.0, 0.6, seconds, precision="f32", keep_going=lambda: False) is None
    # canonical's own errors, per receiver (a wall node is not inside the room)
    with pytest.raises(RuntimeError, match="Source/receiver node position appears to be outside mesh."):
        W.canonical(vm, source, (1 * sp, 5 * sp, 5 * sp), env, 100.0, 0.6, seconds)
    with pytest.raises(RuntimeError, match="Source/receiver node position appears to be outside mesh."):
        W.canonical_many(vm, source, receivers + [(1 * sp, 5 * sp, 5 * sp)], env, 100.0, 0.6, seconds)


def test_impulse_responses_of_the_sample_scene():
    import os
    from wayverb_amd import simulation as W
    from wayverb_amd import wayfile
    set_tuning()
    cfg, v, t, absorptions = wayfile.read_way(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample.way"))
    source = cfg["sources"][0]["position"]
    first = tuple(cfg["receivers"][0]["position"])
    second = (first[0] - 3.3, first[1] - 7.1, first[2] + 0.37)
    kw = dict(cutoff=150.0, usable_portion=0.5, simulation_time=0.05, output_sample_rate=8000.0, precision="f32")
    audio, bands, vm = W.impulse_response(v, t, absorptions, source, first, method=P.ATTENUATOR_MICROPHONE, pointing=(0.0, -1.0, 0.0),
                                          shape=0.5, **kw)
    audios, per, positions, vm2 = W.impulse_responses(v, t, absorptions, source, [first, second],
                                                      method=[P.ATTENUATOR_MICROPHONE, P.ATTENUATOR_NULL], pointing=(0.0, -1.0, 0.0),
                                                      shape=[0.5, 0.0], **kw)
    assert vm2.mesh.dims == vm.mesh.dims and len(audios) == len(per) == 2
    assert per[0][0][0].tobytes() == bands[0][0].tobytes() and per[0][0][1:] == bands[0][1:]
    assert audios[0].tobytes() == audio.tobytes() and np.abs(audio).max() > 0
    assert np.abs(audios[1]).max() > 0 and audios[1].tobytes() != audios[0].tobytes()
    # entry 1 listens at the node nearest to the requested point
    sp = np.float32(vm2.mesh.spacing)
    assert np.abs(positions[0] - np.array(first, dtype=np.float32)).max() < 1e-4
    assert np.abs(positions[1] - np.array(second, dtype=np.float32)).max() <= 0.5 * sp * (1 + 1e-5)
    loc = vm2.compute_locator(second)
    assert np.array_equal(positions[1], vm2.min_corner + np.array(loc, dtype=np.float32) * sp)
    alone = W.canonical(vm2, source, second, W.Environment(), 150.0, 0.5, 0.05, precision="f32")
    assert per[1][0][0].tobytes() == alone[0][0].tobytes()

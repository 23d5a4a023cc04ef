"""The engine's multi-slab step on ONE GPU: K engines of this process, joined by
the in-process transport (wv_comm_init_local) and stepped together (wv_run_group), run exactly the
step the one-rank-per-GPU RCCL chain runs -- wait for ghosts, face planes (sweep + boundary nodes),
exchange, interior planes -- only the face planes travel by device-to-device copies instead of
ncclSend/ncclRecv.  Owned planes, filter memories and receiver traces must equal the single-domain
engine bit for bit (and, through tests/test_gpu_parity.py, the oracle)."""
import numpy as np
import pytest

from wayverb_amd import engine as E
from wayverb_amd import mesh as M
from wayverb_amd.slab import SlabLayout, place_source_and_receivers, slab_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["single-steps", "two-step-passes", "two-step-passes-round-3-order", "three-step-passes",
                                      "three-step-passes-over-work-lists"])
def _step_mode(request):
    """Every test of this file runs three times: with the engine's default choice (single steps on meshes this
    small); with two-step passes forced on (wv_tuning::pair = 1), where a slab exchanges its face planes
    twice per pass -- t+1, then t+2 (engine_pair.hip.h, enqueue_pair_a / _b) -- both exchanges under the march, the
    faces' second step on the halo stream (round 4); and with passes in the order of round 3 (wv_tuning::slab_early = 0:
    the second exchange after the march, and the planes around the exchanges in two launches, sweep then boundary nodes:
    wv_tuning::fuse_planes = 0), which is also what a slab with a source within two planes of a cut falls back to.  Slabs with
    fewer than four planes cannot take two-step passes, and then the whole chain falls back together.
    A fourth time with three-step passes forced on (wv_tuning::triple = 1: engine_triple.hip.h, enqueue_triple_slab -- three exchanges per
    pass, the face planes and the planes next to them by plain steps; slabs of fewer than six planes keep the chain on two-step passes),
    and a fifth with the rooms' work lists left on (these small rooms all count as sparse: every slab then marches a list of live units)."""
    old = dict(E.default_tuning)
    for key in ("pair", "slab_early", "fuse_planes", "triple", "tile_lists"):
        E.default_tuning.pop(key, None)
    if request.param == "three-step-passes":
        E.default_tuning.update(pair=1, triple=1, slab_early=1, tile_lists=0)
    if request.param == "three-step-passes-over-work-lists":
        E.default_tuning.update(pair=1, triple=1, slab_early=1)
    if request.param.startswith("two-step-passes"):
        E.default_tuning["pair"] = 1
        E.default_tuning["slab_early"] = 1      # (forced: by default slabs that share a device keep round 3's order)
        if request.param.endswith("round-3-order"):
            E.default_tuning["slab_early"] = 0
            E.default_tuning["fuse_planes"] = 0
    yield "two-step-passes" if request.param.startswith("two-step-passes") else ("three-step-passes" if request.param.startswith("three-step") else request.param)
    E.default_tuning.clear()
    E.default_tuning.update(old)


def materials(rng):
    return np.concatenate([M.passive_peak_filter_coefficients(rng, 4),
                           np.array([M.rigid_coefficients(), M.flat_coefficients(0.2)], dtype=M.coefficients_dtype)])


def global_mesh(dims, room, rng):
    coeffs = materials(rng)
    if room == "box":
        return M.box_mesh(*dims, coefficients=coeffs, surface_of_face=[0, 1, 2, 3, 4, 5])
    mask = M.room_mask((dims[2], dims[1], dims[0]), room, seed=5)
    nodes, counts = E.classify_nodes(mask)
    return M.mesh_from_nodes(dims, nodes, counts, coeffs, surface_of_port=[0, 1, 2, 3, 4, 5])


def single_domain(gmesh, precision, gprev, gcur, kind, source, signal, receivers, steps):
    eng = E.Engine(gmesh, precision=precision)
    eng.write_field(gprev, E.BUF_PREVIOUS)
    eng.write_field(gcur, E.BUF_CURRENT)
    eng.set_source(kind, source, signal)
    eng.set_receivers(receivers)
    done, flag = eng.run_steps(steps)
    out = dict(done=done, flag=flag, trace=eng.fetch_receivers(0, done), cur=eng.read_field(E.BUF_CURRENT),
               prev=eng.read_field(E.BUF_PREVIOUS), bd=[eng.read_boundary_data(d) for d in (1, 2, 3)])
    eng.close()
    return out


def slab_chain(gmesh, world, precision, gprev, gcur, kind, source, signal, receivers, steps, ghost_readers=()):
    """`ghost_readers`: receiver positions that are recorded by EVERY slab that holds the node, ghost
    copies included (what a directional receiver on a slab face does with its +-z neighbour)."""
    engines, layouts, recv_maps = [], [], []
    for r in range(world):
        L = SlabLayout(gmesh.dims, r, world)
        e = E.Engine(slab_mesh(gmesh, L), precision=precision, ghost_lo=L.ghost_lo, ghost_hi=L.ghost_hi)
        plane = L.plane
        e.write_field(gprev[L.zl0 * plane:L.zl1 * plane], E.BUF_PREVIOUS)
        e.write_field(gcur[L.zl0 * plane:L.zl1 * plane], E.BUF_CURRENT)
        src_local, mine = place_source_and_receivers(L, source, receivers)
        for pos in ghost_readers:
            loc = L.to_local(receivers[pos])
            if loc is not None and not L.owns_z(receivers[pos] // plane):
                mine.append((pos, loc))
        if src_local is not None:
            e.set_source(kind, src_local, signal)
        e.set_receivers([idx for _, idx in mine])
        engines.append(e)
        layouts.append(L)
        recv_maps.append(mine)
    group = E.LocalSlabGroup(engines)
    for e in engines:
        e.enable_kernel_timing(True)
    done, flag = group.run_steps(steps)
    # which path ran: time steps per timed launch of the dominant kernel (2 = two-step passes)
    detail = [e.kernel_time_detail() for e in engines]
    trace = np.full((done, len(receivers)), np.nan)
    ghost_trace = {}
    cur, prev, bd = [], [], [[], [], []]
    for e, L, mine in zip(engines, layouts, recv_maps):
        assert e.step_count() == done
        got = e.fetch_receivers(0, done)
        for col, (pos, _) in enumerate(mine):
            if L.owns_z(receivers[pos] // L.plane):
                trace[:, pos] = got[:, col]
            else:
                ghost_trace.setdefault(pos, []).append(got[:, col])
        lo, hi = L.owned_local_range()
        cur.append(e.read_field(E.BUF_CURRENT)[lo:hi])
        prev.append(e.read_field(E.BUF_PREVIOUS)[lo:hi])
        for d in range(3):
            bd[d].append(e.read_boundary_data(d + 1))
    queries = ([e.query(E.Engine.QUERY_PASSES) for e in engines], [e.query(E.Engine.QUERY_EARLY_PASSES) for e in engines],
               [e.query(E.Engine.QUERY_TRIPLE_PASSES) for e in engines])
    group.close()
    return dict(done=done, flag=flag, trace=trace, ghost_trace=ghost_trace, cur=np.concatenate(cur), detail=detail,
                prev=np.concatenate(prev), bd=[np.concatenate(b) for b in bd], queries=queries)


def boundary_rows(gmesh, d):
    """Rows of the global boundary array of dimensionality d, in node order (slabs keep one row per
    boundary node; the global array may also hold the unused rows numbered for re-entrant nodes)."""
    t = gmesh.nodes["boundary_type"]
    pc = sum(((t >> bit) & 1) for bit in range(8))
    is_b = (t & (M.ID_INSIDE | M.ID_REENTRANT)) == 0
    return gmesh.nodes["boundary_index"][(pc == d) & is_b]


def assert_same(got, want, gmesh):
    assert (got["done"], got["flag"]) == (want["done"], want["flag"])
    assert got["cur"].tobytes() == want["cur"].tobytes(), "current differs"
    assert got["prev"].tobytes() == want["prev"].tobytes(), "previous differs"
    assert got["trace"].tobytes() == want["trace"].tobytes(), "receiver traces differ"
    for pos, copies in got["ghost_trace"].items():
        for c in copies:
            assert c.tobytes() == want["trace"][:, pos].tobytes(), "a ghost copy of receiver %d differs" % pos
    for d in range(3):
        rows = boundary_rows(gmesh, d + 1)
        for field in ("filter_memory", "coefficient_index"):
            assert got["bd"][d][field].tobytes() == np.ascontiguousarray(want["bd"][d][rows][field]).tobytes(), \
                "filter state differs (D=%d, %s)" % (d + 1, field)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("world,room,dims", [(2, "box", (16, 14, 24)), (3, "box", (40, 36, 25)), (8, "box", (16, 14, 24)),
                                             (2, "L", (20, 18, 24)), (3, "blob", (24, 22, 26)), (8, "L", (36, 20, 48)),
                                             (2, "box", (1200, 9, 14))])   # rows of 10 waves: several workgroups per row
def test_slab_chain_equals_single_domain(built_library, world, room, dims, precision, _step_mode):
    rng = np.random.default_rng(2024 + world)
    gmesh = global_mesh(dims, room, rng)
    dtype = np.float32 if precision == "f32" else np.float64
    live = gmesh.nodes["boundary_type"] != 0
    gprev = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    gcur = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    steps = 23
    signal = rng.uniform(-0.1, 0.1, steps)
    # the source on a slab face (top owned plane of slab 0): the neighbour's ghost copy must inject too
    L0 = SlabLayout(dims, 0, world)
    inside = (gmesh.nodes["boundary_type"] & M.ID_INSIDE) != 0
    def first_inside(z):
        idx = np.nonzero(inside[z * L0.plane:(z + 1) * L0.plane])[0]
        return int(z * L0.plane + idx[len(idx) // 2])
    source = first_inside(L0.z1 - 1)
    # receivers: the 7 nodes of a directional receiver centred on the bottom owned plane of slab 1
    # (its -z neighbour is slab 1's ghost plane), plus one node per slab
    L1 = SlabLayout(dims, 1, world)
    centre = first_inside(L1.z0)
    receivers = [centre] + [n for n in gmesh.compute_neighbors(centre)]
    assert all(n != 0xFFFFFFFF for n in receivers)
    for r in range(world):
        L = SlabLayout(dims, r, world)
        receivers.append(first_inside(min(max(L.z0, 2), dims[2] - 3)))
    for kind in (E.SOURCE_SOFT, E.SOURCE_HARD):
        want = single_domain(gmesh, precision, gprev, gcur, kind, source, signal, receivers, steps)
        got = slab_chain(gmesh, world, precision, gprev, gcur, kind, source, signal, receivers, steps,
                         ghost_readers=range(7))
        assert want["done"] == steps and want["flag"] == 0
        assert_same(got, want, gmesh)
        assert len(got["ghost_trace"]) >= 1          # at least the -z neighbour was read from a ghost plane
        planes = dims[2] // world
        if _step_mode == "two-step-passes" and planes >= 4:
            # written fields -> two single full sweeps first, then passes of two steps
            assert all(steps_ > launches for _, launches, steps_ in got["detail"] if launches), got["detail"]
        if _step_mode == "three-step-passes" and planes >= 6 and room == "box":
            # ... or of three: a source on a slab face keeps nobody from them (the neighbour adds the samples to its ghost copy itself)
            assert all(t == (steps - 2) // 3 for t in got["queries"][2]), got["queries"]


def test_a_flag_on_one_slab_stops_the_whole_chain(built_library, oracle):
    """SURVEY.md 8(e) "error-flag OR": waveguide.h:100-119 throws on the step that produced the value;
    here every slab must stop there, not only the one that saw it."""
    dims = (16, 14, 24)
    gmesh = M.box_mesh(*dims)
    sig = np.zeros(40)
    sig[0] = 1.0
    sig[17] = np.inf
    source = gmesh.compute_index(8, 7, 3)             # lives on slab 0 of 3
    zeros = np.zeros(gmesh.num_nodes)
    want = single_domain(gmesh, "f64", zeros, zeros, E.SOURCE_HARD, source, sig, [gmesh.compute_index(8, 7, 20)], 40)
    got = slab_chain(gmesh, 3, "f64", zeros, zeros, E.SOURCE_HARD, source, sig, [gmesh.compute_index(8, 7, 20)], 40)
    from helpers import run_oracle
    named = run_oracle(oracle, dict(mesh=gmesh, steps=40, source_kind=E.SOURCE_HARD, source_node=source, signal=sig,
                                    recv=[gmesh.compute_index(8, 7, 20)], init=None), np.float64)
    assert named["steps"] == 17 and named["flag"] & M.ERR_INF
    assert (want["done"], want["flag"]) == (named["steps"], named["flag"])
    assert (got["done"], got["flag"]) == (named["steps"], named["flag"])
    assert got["trace"].tobytes() == want["trace"].tobytes()


def test_grouped_slabs_refuse_to_be_stepped_alone(built_library):
    gmesh = M.box_mesh(12, 12, 12)
    engines = []
    for r in range(2):
        L = SlabLayout(gmesh.dims, r, 2)
        engines.append(E.Engine(slab_mesh(gmesh, L), ghost_lo=L.ghost_lo, ghost_hi=L.ghost_hi))
    group = E.LocalSlabGroup(engines)
    with pytest.raises(E.WaveguideError, match="wv_run_group"):
        engines[0].run_steps(2)
    assert group.run_steps(4) == (4, 0)
    group.close()


def test_exhausted_source_ends_a_chain(built_library):
    gmesh = M.box_mesh(12, 12, 12)
    engines = []
    for r in range(3):
        L = SlabLayout(gmesh.dims, r, 3)
        e = E.Engine(slab_mesh(gmesh, L), ghost_lo=L.ghost_lo, ghost_hi=L.ghost_hi)
        src = L.to_local(gmesh.compute_index(6, 6, 6))
        if src is not None:
            e.set_source(E.SOURCE_HARD, src, np.ones(5))
        engines.append(e)
    group = E.LocalSlabGroup(engines)
    assert group.run_steps(100) == (5, 0)
    group.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("world,room,dims,steps", [(2, "box", (24, 20, 20), 23), (3, "box", (40, 36, 33), 24), (4, "box", (130, 12, 40), 25),
                                                   (2, "L", (20, 18, 24), 23), (3, "blob", (24, 22, 30), 24), (2, "box", (1200, 9, 16), 22),
                                                   (5, "box", (300, 13, 61), 20)])
def test_three_step_passes_on_slab_chains(built_library, world, room, dims, steps, precision, _step_mode):
    """Slabs thick enough for three-step passes, the source inside a slab (not on a face), receivers on faces, next to them, in ghost
    planes and in mid-slab: with three-step passes forced on every slab takes them -- two single sweeps for the written fields, then
    passes of three, then what the step count leaves -- and the chain equals the single domain bit for bit in every mode."""
    rng = np.random.default_rng(3000 + world + dims[0])
    gmesh = global_mesh(dims, room, rng)
    dtype = np.float32 if precision == "f32" else np.float64
    live = gmesh.nodes["boundary_type"] != 0
    gprev = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    gcur = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    signal = rng.uniform(-0.1, 0.1, steps)
    inside = (gmesh.nodes["boundary_type"] & M.ID_INSIDE) != 0
    L0, L1 = SlabLayout(dims, 0, world), SlabLayout(dims, 1, world)

    def an_inside_node(z, k=2):
        idx = np.nonzero(inside[z * L0.plane:(z + 1) * L0.plane])[0]
        return int(z * L0.plane + idx[len(idx) // k])
    source = an_inside_node(L1.z0 + 3)                       # three planes into slab 1
    centre = an_inside_node(L1.z0)                            # a directional receiver's seven nodes around slab 1's bottom face
    receivers = [centre] + [n for n in gmesh.compute_neighbors(centre)]
    assert all(n != 0xFFFFFFFF for n in receivers)
    receivers += [an_inside_node(L0.z1 - 2, 3), an_inside_node(L0.z1 - 3, 3), an_inside_node(L1.z0 + 1, 3), an_inside_node(L1.z0 + 2, 3)]
    for kind in (E.SOURCE_SOFT, E.SOURCE_HARD):
        want = single_domain(gmesh, precision, gprev, gcur, kind, source, signal, receivers, steps)
        got = slab_chain(gmesh, world, precision, gprev, gcur, kind, source, signal, receivers, steps, ghost_readers=range(7))
        assert want["done"] == steps and want["flag"] == 0
        assert_same(got, want, gmesh)
        if _step_mode == "three-step-passes" and room == "box":
            assert all(t == (steps - 2) // 3 for t in got["queries"][2]), got["queries"]


@pytest.mark.parametrize("seed", range(24))
def test_random_slab_chains_equal_the_single_domain(built_library, seed, _step_mode):
    """Seeded random chains: 2-7 slabs of unequal thickness (down to one plane, where the whole chain falls back to
    single steps), box / L / blob rooms, the source anywhere that is not `none` (inside, on a wall, on a slab face),
    receivers anywhere, noise to start with -- against the single-domain engine in the same stepping mode."""
    rng = np.random.default_rng(700 + seed)
    world = int(rng.integers(2, 8))
    room = ["box", "L", "blob"][seed % 3]
    nx = int(rng.choice([rng.integers(14, 40), rng.integers(125, 135)], p=[0.8, 0.2]))
    ny = int(rng.integers(14, 30))
    # (thin slabs -- down to one plane -- most of the time; every third chain thick enough, 8 to 13 planes per slab, for passes that
    # step the faces and the planes next to them ahead of the march)
    per_slab = int(rng.integers(1, 8)) if seed % 3 else int(rng.integers(8, 14))
    nz = int(max(14, world * per_slab + rng.integers(0, world)))
    dims = (nx, ny, nz)
    gmesh = global_mesh(dims, room, rng)
    precision = "f64" if seed % 2 else "f32"
    dtype = np.float64 if precision == "f64" else np.float32
    t = gmesh.nodes["boundary_type"]
    live = t != 0
    gprev = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    gcur = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    steps = int(rng.integers(4, 30))
    signal = rng.uniform(-0.1, 0.1, steps)
    inside = np.nonzero(t & M.ID_INSIDE)[0]
    source = int(rng.choice(inside)) if rng.random() < 0.6 else int(rng.choice(np.nonzero(live)[0]))
    receivers = [int(rng.choice(inside)) if rng.random() < 0.6 else int(rng.integers(0, gmesh.num_nodes))
                 for _ in range(int(rng.integers(1, 6)))]
    kind = int(rng.choice([E.SOURCE_SOFT, E.SOURCE_HARD]))
    want = single_domain(gmesh, precision, gprev, gcur, kind, source, signal, receivers, steps)
    got = slab_chain(gmesh, world, precision, gprev, gcur, kind, source, signal, receivers, steps)
    assert want["done"] == steps and want["flag"] == 0
    assert_same(got, want, gmesh)


@pytest.mark.parametrize("seed", range(200, 236))
def test_more_random_slab_chains_equal_the_single_domain(built_library, seed, _step_mode):
    """tools/extended_fuzz.py's slab-chain family with a fixed budget of fresh seeds (it found the soft-source-on-a-face race of
    round 3 at about one chain in 1 500): the same check as above, in the three stepping modes."""
    test_random_slab_chains_equal_the_single_domain(built_library, seed, _step_mode)


def test_a_group_refuses_slabs_that_are_out_of_step():
    """Exchanges address the neighbour's field buffers by role: a slab that was stepped on its own (wv_step + wv_swap)
    before joining no longer has its buffers in the roles the others have, and wv_run_group says so instead of
    pushing face planes into the wrong field."""
    gmesh = global_mesh((20, 18, 24), "box", np.random.default_rng(3))
    engines = []
    for r in range(2):
        L = SlabLayout(gmesh.dims, r, 2)
        engines.append(E.Engine(slab_mesh(gmesh, L), precision="f64", ghost_lo=L.ghost_lo, ghost_hi=L.ghost_hi))
    engines[1].step()
    engines[1].swap()
    group = E.LocalSlabGroup(engines)
    try:
        with pytest.raises(E.WaveguideError, match="same steps"):
            group.run_steps(4)
    finally:
        group.close()


def test_a_slab_with_a_neighbour_elsewhere_marches_in_two_rounds(_step_mode):
    """The exchange of a slab's t+1 faces is to run under its march, and whatever carries it (RCCL's send / receive
    kernels, the runtime's copy kernels) needs a CU.  A march whose workgroups fill the chip's slots exactly once holds
    every register of every CU until all of them retire together, at its end -- so a slab with a neighbour on another GPU
    (RCCL: here a rank that is its own neighbour) takes the chunking with two rounds where that costs little
    (engine_pair.hip.h, ensure_pair); one domain keeps the single round, and so do slabs of one process that share a device:
    they take turns at the march, nothing could run beside it.  1024 x 1024 rows: 256 strips of 8 waves = the chip's 256
    workgroup slots."""
    from wayverb_amd.slab import box_slab_mesh                  # (meshes this size take two-step passes in either mode)
    n, nz = 1024, 128
    coeffs = M.bench_materials()
    engines = []
    for r in range(2):
        L = SlabLayout((n, n, nz), r, 2)
        engines.append(E.Engine(box_slab_mesh(n, n, nz, L, coefficients=coeffs), precision="f64", ghost_lo=L.ghost_lo, ghost_hi=L.ghost_hi,
                                tuning=dict(triple=0)))                   # (the two-step march's rounds: slabs this big take three-step passes by themselves)
    group = E.LocalSlabGroup(engines)
    try:
        assert all(e.query(E.Engine.QUERY_MARCH_ROUNDS) == 0 for e in engines)      # nothing planned yet
        assert group.run_steps(4) == (4, 0)
        assert [e.query(E.Engine.QUERY_PASSES) for e in engines] == [2, 2]
        assert [e.query(E.Engine.QUERY_MARCH_ROUNDS) for e in engines] == [1, 1]      # two slabs, one device
    finally:
        group.close()

    class Whole:
        zl0, zl1, z0, z1 = 0, nz // 2, 0, nz // 2
        local_dims = (n, n, nz // 2)
        plane = n * n
    single = E.Engine(box_slab_mesh(n, n, nz // 2, Whole, coefficients=coeffs), precision="f64", tuning=dict(triple=0))
    try:
        assert single.run_steps(4) == (4, 0)
        assert single.query(E.Engine.QUERY_MARCH_ROUNDS) == 1
    finally:
        single.close()
    # a middle rank over RCCL (its own neighbour on both sides): two rounds
    nodes, counts = E.make_box_nodes(n, n, 8 * 64, z_begin=3 * 64 - 1, z_count=66, number_from=3 * 64, number_to=4 * 64)
    bidx = [(np.arange(counts[d] * (d + 1), dtype=np.uint32) % np.uint32(coeffs.shape[0])).reshape(counts[d], d + 1) for d in range(3)]
    rank = E.Engine(M.Mesh((n, n, 66), nodes, coeffs, *bidx), precision="f64", ghost_lo=True, ghost_hi=True, tuning=dict(triple=0))
    try:
        rank.comm_init(E.Engine.comm_unique_id(), 0, 1)
        assert rank.run_steps(4) == (4, 0)
        assert rank.query(E.Engine.QUERY_PASSES) == 2 and rank.query(E.Engine.QUERY_MARCH_ROUNDS) == 2
    finally:
        rank.close()


def test_soft_source_on_a_slab_face_for_many_steps(_step_mode):
    """A source on a slab face is injected by its owner and by the neighbour that holds a ghost copy of the plane.  The
    owner's exchange of that face plane runs on the halo stream while its compute stream moves on: the next sample must
    not be added before the exchange has read the plane, or the neighbour adds it a second time (soft sources; about one
    random chain in 1 500 hit this before SlabComm::wait_ghosts waited for the slab's own pushes too).  Thin slabs, so
    that a step is over almost before its exchange has started; many steps, several times."""
    rng = np.random.default_rng(11)
    dims = (24, 24, 14)
    gmesh = global_mesh(dims, "box", rng)
    plane = dims[0] * dims[1]
    live = gmesh.nodes["boundary_type"] != 0
    layouts = [SlabLayout(dims, r, 3) for r in range(3)]
    steps = 300
    for rep in range(6):
        z = layouts[1].z1 - 1 if rep % 2 == 0 else layouts[1].z0      # the middle slab's top / bottom face
        source = z * plane + (7 + rep) * dims[0] + 9
        assert gmesh.nodes["boundary_type"][source] & M.ID_INSIDE
        gprev = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0)
        gcur = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0)
        signal = rng.uniform(-0.1, 0.1, steps)
        receivers = [source, source + plane, source - plane]
        want = single_domain(gmesh, "f64", gprev, gcur, E.SOURCE_SOFT, source, signal, receivers, steps)
        got = slab_chain(gmesh, 3, "f64", gprev, gcur, E.SOURCE_SOFT, source, signal, receivers, steps)
        assert want["done"] == steps and want["flag"] == 0
        assert_same(got, want, gmesh)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("dz", [-3, -2, -1, 0, 1, 2])
def test_sources_around_a_cut_and_which_slabs_keep_the_older_order(built_library, precision, dz, _step_mode):
    """Round 4: a slab's pass steps its faces and the planes next to them ahead of the march and the faces once more on the halo
    stream, between the two exchanges -- unless the source lies in its planes g, f, n next to a cut (the sample of step t+1 goes
    in after the march; the faces' second step would read those planes before it).  Sources from three planes below a cut to two
    above it, soft and hard, with receivers on both sides: bit-identical to the single domain, and the slabs that kept the older
    order are exactly the ones that see the source within two planes of the cut."""
    rng = np.random.default_rng(400 + dz)
    dims, world = (36, 20, 45), 3                                  # 15 planes per slab
    gmesh = global_mesh(dims, "box", rng)
    dtype = np.float32 if precision == "f32" else np.float64
    live = gmesh.nodes["boundary_type"] != 0
    gprev = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    gcur = np.where(live, rng.uniform(-0.25, 0.25, gmesh.num_nodes), 0.0).astype(dtype)
    layouts = [SlabLayout(dims, r, world) for r in range(world)]
    plane = dims[0] * dims[1]
    cut = layouts[1].z0                                             # first plane of slab 1
    z = cut + dz
    source = z * plane + 9 * dims[0] + 17
    assert gmesh.nodes["boundary_type"][source] & M.ID_INSIDE
    receivers = [source, source + plane, source - plane, (cut - 1) * plane + 5 * dims[0] + 5, cut * plane + 5 * dims[0] + 5,
                 (layouts[2].z0) * plane + 11 * dims[0] + 30, 3 * plane + 4 * dims[0] + 4]
    steps = 26
    signal = rng.uniform(-0.1, 0.1, steps)
    for kind in (E.SOURCE_SOFT, E.SOURCE_HARD):
        want = single_domain(gmesh, precision, gprev, gcur, kind, source, signal, receivers, steps)
        got = slab_chain(gmesh, world, precision, gprev, gcur, kind, source, signal, receivers, steps)
        assert want["done"] == steps and want["flag"] == 0
        assert_same(got, want, gmesh)
        passes, early, triples = got["queries"]
        if _step_mode == "three-step-passes":
            assert all(t == (steps - 2) // 3 for t in triples), triples     # wherever the source lies: on a face, in a ghost plane, next to them
        if _step_mode == "two-step-passes":
            assert all(p == (steps - 2) // 2 for p in passes), passes
            if E.default_tuning.get("slab_early", -1) == 0:
                assert early == [0, 0, 0]
            else:
                # slab 0 sees planes cut-2, cut-1 (its n, f) and cut (its ghost); slab 1 sees cut-1 (ghost), cut, cut+1 (f, n)
                keeps_old = [cut - 2 <= z <= cut, cut - 1 <= z <= cut + 1, False]
                assert [e == 0 for e in early] == keeps_old, (early, z - cut)
                assert all(e in (0, p) for e, p in zip(early, passes))

"""The table of failing-step cases: a chosen node goes non-finite at a chosen level of a pass, and every stepping form of the engine
has to stop there with the oracle's word (tests/test_failing_step_cases.py proves each case on the CPU, against the oracle alone;
tests/test_gpu_failing_step.py runs the engine's forms through it).  NumPy and the oracle only: nothing here touches a GPU.

The construction: after a healthy prefix of PREFIX steps from quiet noise, a shell of equal finite values V = sign * f * max(Real) is
written into `current` on the live nodes at L1 distance exactly k from the target.  The running sum at the target overflows at the k-th
step from there and nowhere earlier; f is the first rung of LADDER for which the oracle says so -- its k-th step is the first to raise a
flag, the word is exactly ERR_INF, and the target is the only non-finite node.  The written cases put +inf, +inf and -inf, or a NaN on
the target's first live neighbours (port order) instead, and fail at the first step with whatever word the oracle names.

PREFIX = 8 is the two single sweeps a written field costs plus six steps, a multiple of both pass lengths, so the run that follows
starts on a pass boundary and its k-th step is level k of a pass."""
import functools
from collections import namedtuple

import numpy as np

from wayverb_amd import mesh as M

PREFIX = 8
RUN = 9
LADDER = tuple(0.9 * 0.85 ** i for i in range(40))
QUIET_SEED = 5

DTYPE = {"f32": np.float32, "f64": np.float64}

# how: "overflow" (the shell), "inf", "inf-inf", "nan" (written values, k = 1).  seam: tuning the engine needs for the seam to lie where
# the table says.
# slabs: 0 = one domain, 2 = the box cut in two along z (the expectation is the single domain's oracle either way).
Case = namedtuple("Case", "id mesh tag target k sign how seam slabs")


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.oracle import Oracle
    return Oracle()


def _coefficients():
    return np.concatenate([M.passive_peak_filter_coefficients(np.random.default_rng(1), 3),
                           np.array([M.flat_coefficients(0.3)], dtype=M.coefficients_dtype)])


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "box":
        return M.box_mesh(24, 20, 18, coefficients=_coefficients(), surface_of_face=[0, 1, 2, 3, 0, 1])
    if name == "long":
        return M.box_mesh(300, 21, 13, coefficients=_coefficients(), surface_of_face=[0, 1, 2, 3, 0, 1])
    if name == "L":
        mask = M.room_mask((30, 36, 40), "L", seed=3)
        nodes, counts = oracle().classify(mask)
        return M.mesh_from_nodes((40, 36, 30), nodes, counts, _coefficients(), surface_of_port=[0, 1, 2, 3, 0, 1])
    raise ValueError(name)


def engine_kw(case):
    """Engine arguments a case's mesh needs: the L room visits every tile (rooms with work lists keep two-step passes)."""
    return dict(all_tiles=True) if case.mesh == "L" else {}


def quiet_fields(name, tag):
    """(previous, current): uniform(-1e-3, 1e-3) on live nodes, zeros outside."""
    mesh = mesh_of(name)
    live = mesh.nodes["boundary_type"] != 0
    rng = np.random.default_rng(QUIET_SEED)
    out = []
    for _ in range(2):
        f = np.zeros(mesh.num_nodes)
        f[live] = rng.uniform(-1e-3, 1e-3, int(live.sum()))
        out.append(f.astype(DTYPE[tag]))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def prefix_state(name, tag):
    """The oracle's state after the healthy prefix: (previous, current, [bd1, bd2, bd3], history), history[s] = `current` at step s
    (what a receiver records at step s).  Callers copy before they change anything."""
    mesh = mesh_of(name)
    prev, cur = quiet_fields(name, tag)
    bd = [mesh.boundary_data(d) for d in (1, 2, 3)]
    history = []
    for _ in range(PREFIX):
        history.append(cur.copy())
        assert oracle().step(prev, cur, mesh, bd, threads=2) == 0
        prev, cur = cur, prev
    return prev, cur, bd, np.array(history)


def locator(mesh, index):
    return tuple(int(c) for c in mesh.compute_locator(index))


def live_neighbours(mesh, target):
    """The target's live neighbours, as node indices in port order."""
    t = mesh.nodes["boundary_type"]
    return [n for n in mesh.compute_neighbors(mesh.compute_index(*target)) if n != 0xFFFFFFFF and t[n] != 0]


def shell_nodes(mesh, target, k):
    """Live nodes at L1 distance exactly k from the target, in node order."""
    nx, ny, nz = mesh.dims
    tx, ty, tz = target
    t = mesh.nodes["boundary_type"]
    out = []
    for dz in range(-k, k + 1):
        for dy in range(-(k - abs(dz)), k - abs(dz) + 1):
            rest = k - abs(dz) - abs(dy)
            for dx in sorted({-rest, rest}):
                x, y, z = tx + dx, ty + dy, tz + dz
                if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and t[mesh.compute_index(x, y, z)] != 0:
                    out.append(mesh.compute_index(x, y, z))
    return sorted(out)


def _written(case, mesh):
    nb = live_neighbours(mesh, case.target)
    if case.how == "inf":
        return [(nb[0], np.inf)]
    if case.how == "inf-inf":
        return [(nb[0], np.inf), (nb[1], -np.inf)]
    if case.how == "nan":
        return [(nb[0], np.nan)]
    raise ValueError(case.how)


def first_flag(case, prev, cur, bd):
    """Steps the oracle from (prev, cur, bd), all changed in place, until a flag is raised or k steps are through.  Returns (steps taken before
    the flagged one, word, non-finite nodes after the flagged step), word 0 and no nodes where none was raised."""
    mesh = mesh_of(case.mesh)
    for s in range(case.k):
        flag = oracle().step(prev, cur, mesh, bd, threads=2)
        if flag:
            return s, flag, np.nonzero(~np.isfinite(prev))[0]
        prev, cur = cur, prev
    return case.k, 0, np.zeros(0, dtype=np.int64)


def qualifies(case, s, flag, bad):
    """The rule a case is held to (the CPU test asserts the same, from the fields): the k-th step is the first to fail, the word is
    exactly ERR_INF, the target is the only non-finite node."""
    target = mesh_of(case.mesh).compute_index(*case.target)
    return s == case.k - 1 and flag == M.ERR_INF and bad.tolist() == [target]


@functools.lru_cache(maxsize=None)
def placements(case):
    """[(node, value)] to write into `current` after the prefix; for the shell, calibrated against the oracle on the prefix's fields.
    Raises where no rung of the ladder qualifies: that is a finding, not a case to drop."""
    mesh = mesh_of(case.mesh)
    if case.how != "overflow":
        return tuple(_written(case, mesh))
    dtype = DTYPE[case.tag]
    shell = shell_nodes(mesh, case.target, case.k)
    p0, c0, bd0, _ = prefix_state(case.mesh, case.tag)
    for f in LADDER:
        value = dtype(case.sign * f * float(np.finfo(dtype).max))
        prev, cur, bd = p0.copy(), c0.copy(), [b.copy() for b in bd0]
        cur[shell] = value
        if qualifies(case, *first_flag(case, prev, cur, bd)):
            return tuple((n, float(value)) for n in shell)
    raise AssertionError("no rung of the ladder makes %s fail at step %d alone" % (case.id, case.k))


def poisoned_fields(case):
    """(previous, current, bd) after the prefix with the case's values in place: fresh copies."""
    p0, c0, bd0, _ = prefix_state(case.mesh, case.tag)
    prev, cur, bd = p0.copy(), c0.copy(), [b.copy() for b in bd0]
    for node, value in placements(case):
        cur[node] = value
    return prev, cur, bd


def receivers(case):
    """One on the target, one on a neighbour, one far away (a live node more than eight steps from the target)."""
    mesh = mesh_of(case.mesh)
    nx, ny, nz = mesh.dims
    t = mesh.nodes["boundary_type"]
    far = [(3, 3, 3), (nx - 4, 3, nz - 4), (3, 3, nz - 4), (nx - 4, 3, 3)]
    far = [c for c in far if sum(abs(a - b) for a, b in zip(c, case.target)) > 8 and t[mesh.compute_index(*c)] != 0]
    return [mesh.compute_index(*case.target), live_neighbours(mesh, case.target)[-1], mesh.compute_index(*far[0])]


def expected(case):
    """What the oracle's run loop says of the RUN steps after the prefix: (steps done, word, receiver rows of the whole run up to the
    failing step -- the prefix's rows and the rows of the steps done)."""
    mesh = mesh_of(case.mesh)
    recv = receivers(case)
    prev, cur, bd = poisoned_fields(case)
    done, flag, out = oracle().run(prev, cur, mesh, bd, 0, 0, None, RUN, recv, threads=2)
    history = prefix_state(case.mesh, case.tag)[3]
    return done, flag, np.concatenate([history[:, recv], out[:done]])


# ---- the table ---------------------------------------------------------------------------------------------------------------------
BOX_CLASSES = [
    ("deep", (12, 10, 9)),
    ("faced-x", (2, 10, 9)), ("faced-y", (12, 2, 9)), ("faced-z", (12, 10, 2)),
    ("two-from-x", (3, 10, 9)), ("two-from-y", (12, 3, 9)), ("two-from-z", (12, 10, 3)),
    ("wall-x", (1, 10, 9)), ("wall-y", (12, 1, 9)), ("wall-z", (12, 10, 1)), ("wall-x-far", (22, 10, 9)),
    ("edge-xy", (1, 1, 9)), ("edge-yz", (12, 1, 1)), ("edge-xz", (1, 10, 1)),
    ("corner", (1, 1, 1)),
    ("edge-crook", (2, 2, 9)),
    ("corner-crook", (2, 2, 2)),
]
# The only (class, k) pairs the table leaves out: no rung of the ladder leaves the target alone non-finite -- the inside node in a crook
# gathers from wall and edge nodes that gather from the same shell, and those overflow in the same step or a step earlier (at 0.1088 the
# edge-crook shell of k = 3 also takes the edge node (1, 1, 7) and wall nodes beside it over; a rung lower nothing overflows).  The looser
# rule "every other non-finite node is an inside node" does not hold for them either, so they are absent, not relaxed.
OMITTED = {("edge-crook", 3), ("corner-crook", 2), ("corner-crook", 3)}


def _case(name, mesh, tag, target, k, sign=1, how="overflow", seam=(), slabs=0):
    return Case("%s-%s-k%d" % (name, tag, k), mesh, tag, tuple(target), k, sign, how, tuple(sorted(dict(seam).items())), slabs)


def _l_room_targets():
    """A re-entrant node of the L room's inner edge at mid height, and the first inside node beside it (port order)."""
    mesh = mesh_of("L")
    t = mesh.nodes["boundary_type"]
    z = mesh.dims[2] // 2
    plane = mesh.dims[0] * mesh.dims[1]
    re = np.nonzero(t[z * plane:(z + 1) * plane] == M.ID_REENTRANT)[0]
    node = int(z * plane + re[len(re) // 2])
    beside = [n for n in mesh.compute_neighbors(node) if t[n] == M.ID_INSIDE][0]
    return locator(mesh, node), locator(mesh, beside)


def _build():
    out = []
    # a. every node class of the box, both precisions, every level
    for name, target in BOX_CLASSES:
        for tag in ("f32", "f64"):
            for k in (1, 2, 3):
                if (name, k) not in OMITTED:
                    out.append(_case(name, "box", tag, target, k))
    # b. -inf: bad_bits has to see it too
    for name in ("deep", "faced-x", "wall-x"):
        for tag in ("f32", "f64"):
            for k in (1, 2, 3):
                out.append(_case(name + "-negative", "box", tag, dict(BOX_CLASSES)[name], k, sign=-1))
    # c. written values, first step: +inf on one neighbour; +inf and -inf on two (NaN at the target, INF around it); a NaN on one
    for name in ("deep", "faced-x", "wall-x", "edge-xy"):
        for how in ("inf", "inf-inf", "nan"):
            for tag in ("f32", "f64"):
                out.append(_case("%s-written-%s" % (name, how), "box", tag, dict(BOX_CLASSES)[name], 1, how=how))
    # d. seams of the three-step march, targets two or more nodes from every wall.
    #  z-chunks: choose_chunks (march_plan.h) with wv_tuning::triple_chunks = 2 on 18 planes: zc = 9, chunk 0 = planes 0..8, chunk 1 = 9..17
    for z in (8, 9):
        for tag in ("f32", "f64"):
            for k in (1, 2, 3):
                out.append(_case("seam-zchunk-z%d" % z, "box", tag, (12, 10, z), k, seam=dict(triple_chunks=2)))
    #  strips: kTripleRows = 4 rows (triple_kernels.hip.h); ny = 21 is five strips and a sixth of one row.  Rows 15 | 16: the last
    #  interior strip (y0 + 6 < ny) and the first EDGE one (triple_march_kernel's dispatch), whose rows 20..23 lie partly off the grid;
    #  one chunk along z, so that the strip seam is the only one near the target
    for y in (15, 16):
        for tag in ("f32", "f64"):
            for k in (1, 2, 3):
                out.append(_case("seam-strip-y%d" % y, "long", tag, (150, y, 6), k, seam=dict(triple_chunks=1)))
    #  waves: a wave holds 64 lanes of triple_lanes bytes (VecL): with 8-byte lanes 64 doubles / 128 floats, with 16-byte lanes 128 /
    #  256.  Columns 127 | 128 lie on either side of a wave boundary for doubles on both lane widths and floats on 8-byte lanes, 255 | 256
    #  for all four.  Column 296 is the last one two nodes from the wall (nx - 2 = 298); rows are padded to 384 doubles / 512 floats
    #  (engine_setup.hip.h: 64 lanes x 16 B), so the pad begins inside the wave that holds it.
    #  Windows: triple_windows (march_plan.h) cuts a row only when it is longer than triple_max_waves = 12 / 8 waves; 300 columns are at
    #  most 6 waves, so this mesh has no window boundary at either lane width (windows begin at 769 doubles on 8-byte lanes; such rows
    #  are marched by test_triple_path_both_lane_widths_of_the_march, without a failing step).
    for x in (127, 128, 255, 256, 296):
        for lanes in (8, 16):
            for tag in ("f32", "f64"):
                for k in (1, 2, 3):
                    out.append(_case("seam-wave-x%d-lanes%d" % (x, lanes), "long", tag, (x, 10, 6), k, seam=dict(triple_lanes=lanes)))
    # e. the L room: a re-entrant node and an inside node beside it
    re, beside = _l_room_targets()
    for name, target in (("reentrant", re), ("beside-reentrant", beside)):
        for tag in ("f32", "f64"):
            for k in (1, 2, 3):
                out.append(_case(name, "L", tag, target, k))
    # f. the box cut in two along z (SlabLayout: slab 0 owns planes 0..8, slab 1 planes 9..17).  Either side of the cut: the face plane,
    #  the owned plane next to it -- where only the march can supply t+2 (TripleArgs::z2_lo / z2_hi) --, the first plane the march owns
    #  (triple_plan_.z0 / z1: two planes in from a ghost, engine_triple.hip.h)
    for name, z in (("face-lo", 8), ("next-to-face-lo", 7), ("march-lo", 6), ("face-hi", 9), ("next-to-face-hi", 10), ("march-hi", 11)):
        for tag in ("f64",) + (("f32",) if name.startswith("next") else ()):
            for k in (1, 2, 3):
                out.append(_case("slab-" + name, "box", tag, (12, 10, z), k, slabs=2))
    return out


CASES = _build()
assert len({c.id for c in CASES}) == len(CASES)

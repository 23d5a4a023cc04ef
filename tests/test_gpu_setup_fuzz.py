"""The scene -> mesh kernels (node_inside.hip, mesh_setup.hip, boundary_surfaces.hip, scene_mesh.hip) against the restatement, stage
by stage, on the random scenes of tests/setup_scenes.py and on cases aimed at the edges of their launch shapes.

Every stage is fed the RESTATEMENT's output of the stage before it, so a failure names its kernel:
  wv_nodes_inside          on the scene                          against oracle.nodes_inside
  wv_classify_nodes        on the restatement's inside flags     against oracle.classify
  wv_boundary_index_data   on the restatement's node types       against oracle.boundary_index_data
and the chain resident on the device (wv_scene_mesh_create) against the whole restated chain.  No tolerance anywhere: the device
code is built without contraction and with correctly rounded single-precision division, the restatement is single precision in the
reference's expression order, so flags, types, indices and surfaces are equal or wrong."""
import ctypes as C
import os

import numpy as np
import pytest

import setup_scenes as SS
from helpers import unpack_reference_inputs
from wayverb_amd import scene as S

BOUNDARY_1D = [2, 4, 8, 16, 32, 64]
POPCOUNT = np.array([bin(k).count("1") for k in range(256)])


def node_difference(case, got, want, what):
    """Condensed nodes: the first node whose type differs, else the first whose index differs."""
    return (SS.first_difference(case, got["boundary_type"], want["boundary_type"], what + ": boundary_type")
            or SS.first_difference(case, got["boundary_index"], want["boundary_index"], what + ": boundary_index"))


def row_difference(case, nodes, d, got, want, what):
    """Surface arrays [n_d, d + 1]: the first row that differs and the node that owns it."""
    if got.shape != want.shape:
        return "%s: shape %s, want %s\n  %s" % (what, got.shape, want.shape, SS.describe(case))
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    if bad.size == 0:
        return None
    r = int(bad[0])
    bt = nodes["boundary_type"]
    numbered = ((bt & 129) == 0) & (POPCOUNT[bt & 255] == d + 1)
    owner = np.nonzero(numbered & (nodes["boundary_index"] == r))[0]
    where = ""
    if owner.size:
        i = int(owner[0])
        nx, ny, _ = case.dims
        loc = (i % nx, (i // nx) % ny, i // (nx * ny))
        pos = case.min_corner + np.array(loc, dtype=np.float32) * np.float32(case.spacing)
        where = ", node %d at locator %s, position %s" % (i, loc, tuple(float(p) for p in pos))
    return "%s: %d of %d rows differ, first row %d%s: got %s, want %s\n  %s" % (
        what, bad.size, got.shape[0], r, where, got[r].tolist(), want[r].tolist(), SS.describe(case))


def staged_failures(case, stages=("inside", "classify", "surfaces")):
    """The three staged entry points, each on the restatement's output of the stage before it."""
    from wayverb_amd import engine as E
    c, w = case, case.want
    out = []
    if "inside" in stages:
        got = E.nodes_inside(c.dims, c.min_corner, c.spacing, w.vox, c.aabb, c.side, c.triangles, c.vertices)
        out.append(SS.first_difference(c, got, w.mask, "wv_nodes_inside (node_inside_kernel)"))
    if "classify" in stages:
        nodes, counts = E.classify_nodes(w.mask)
        out.append(node_difference(c, nodes, w.first, "wv_classify_nodes (node_boundary_type_kernel)"))
        if counts != w.counts_first:
            out.append("wv_classify_nodes: counts %s, want %s\n  %s" % (counts, w.counts_first, SS.describe(c)))
    if "surfaces" in stages:
        nodes = w.first.copy()
        nodes["boundary_index"] = 0xdeadbeef          # must be ignored on input
        b = E.boundary_index_data(c.dims, c.min_corner, c.spacing, nodes, c.triangles, c.vertices)
        out.append(node_difference(c, nodes, w.nodes, "wv_boundary_index_data: nodes after renumbering"))
        for d in range(3):
            out.append(row_difference(c, w.nodes, d, b[d], w.b[d], "wv_boundary_index_data: %d-D surfaces (%s)" % (
                d + 1, "nearest_surface_kernel" if d == 0 else "gather_surfaces_kernel")))
    return [x for x in out if x]


def chain_failures(case):
    """wv_scene_mesh_create: all of it on the device, nothing from the restatement but the voxel lists."""
    from wayverb_amd import engine as E
    c, w = case, case.want
    sm = E.SceneMesh(c.dims, c.min_corner, c.spacing, w.vox, c.aabb, c.side, c.triangles, c.vertices)
    try:
        nodes, b = sm.fetch()
        counts = sm.counts
    finally:
        sm.close()
    out = [node_difference(c, nodes, w.nodes, "wv_scene_mesh_create: nodes")]
    if counts != w.counts:
        out.append("wv_scene_mesh_create: counts %s, want %s\n  %s" % (counts, w.counts, SS.describe(c)))
    else:
        for d in range(3):
            out.append(row_difference(c, w.nodes, d, b[d], w.b[d], "wv_scene_mesh_create: %d-D surfaces" % (d + 1)))
    return [x for x in out if x]


def check(case, staged=True, chain=True, stages=("inside", "classify", "surfaces")):
    failures = (staged_failures(case, stages) if staged else []) + (chain_failures(case) if chain else [])
    assert not failures, "\n".join(failures)


# ---- the random scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SS.SEEDS))
def test_random_scene_stage_by_stage_and_chained(built_library, seed):
    check(SS.scene_case(seed))


# ---- aimed cases ---------------------------------------------------------------------------------------------------------
def box_in_grid(name, dims, seed, spacing=0.1, side=8, fill=0.22, triangles=None):
    """A rotated box in the middle of a mesh grid of the given dims (the voxel box is the grid's extent): all three boundary classes
    and re-entrant nodes, whatever the dims."""
    rng = np.random.default_rng(seed)
    mc = np.array([-0.35, 0.2, 1.0], dtype=np.float32)
    extent = (np.array(dims) - 1) * spacing
    v, t = SS.rotated_box(mc + extent / 2 + rng.uniform(-0.3, 0.3, 3) * spacing, np.maximum(fill * extent, 1.7 * spacing),
                          SS.rotation(rng))
    t[:, 0] = np.arange(t.shape[0]) % 5
    if triangles is not None:
        v, t = triangles(v, t)
    return SS.custom_case(name, v, t, spacing, dims, mc, SS.grid_extent(dims, mc, spacing), side)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(9, 9, 9), (7, 6, 5), (16, 16, 16), (8, 16, 32), (11, 19, 49), (17, 23, 55)],
                         ids=lambda d: "x".join(str(k) for k in d))
def test_numbering_scan_at_the_edges_of_its_chunks(built_library, dims):
    """scene_mesh.hip numbers 1 024 nodes per workgroup: fewer nodes than one chunk (729, 210), whole chunks exactly (4 096, both
    ways), and whole chunks plus one node (11*19*49 = 10 * 1 024 + 1, 17*23*55 = 21 * 1 024 + 1)."""
    n = dims[0] * dims[1] * dims[2]
    assert n < 1024 or n % 1024 in (0, 1)
    case = box_in_grid("scan edge", dims, seed=n)
    types = case.want.nodes["boundary_type"]
    assert min(case.want.counts) > 0 and np.count_nonzero(types == 128) > 0, "the case lost what it is for"
    check(case)


def padded_list(count, reverse):
    """Brings a triangle list to exactly `count` triangles with small triangles far outside the mesh grid (other surfaces, never the
    nearest); reversed, the scene's own triangles come last, in the last and short stage of the search."""
    def edit(v, t):
        extra = count - t.shape[0]
        assert extra >= 0
        far = np.zeros((3 * extra, 4), dtype=np.float32)
        tris = np.zeros((extra, 4), dtype=np.uint32)
        for k in range(extra):
            p = np.array([90.0 + 0.5 * (k % 37), 120.0 + 0.5 * (k // 37), -75.0])
            far[3 * k:3 * k + 3, :3] = p + np.array([[0, 0, 0], [0.2, 0, 0.1], [0, 0.2, 0.1]])
            tris[k] = (5 + k % 6, v.shape[0] + 3 * k, v.shape[0] + 3 * k + 1, v.shape[0] + 3 * k + 2)
        v, t = np.concatenate([v, far]), np.concatenate([t, tris])
        return v, (t[::-1] if reverse else t)
    return edit


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True], ids=["as_is", "reversed"])
@pytest.mark.parametrize("count", [12, 511, 512, 513, 1024, 1025])
def test_triangle_counts_at_the_edges_of_the_search_stages(built_library, count, reverse):
    """nearest_surface_kernel stages 512 triangles per round through LDS: lists of one short stage, one full stage, full stages plus
    one triangle; the winners in the first stage (as is) and in the last (reversed).  Staged and chained."""
    case = box_in_grid("%d triangles" % count, (17, 14, 20), seed=count, fill=0.26, triangles=padded_list(count, reverse))
    assert case.triangles.shape[0] == count and min(case.want.counts) > 0
    assert len(np.unique(case.want.b[0])) > 1 and case.want.b[0].max() < 5, "a far triangle won, or one surface took all"
    check(case)


@pytest.mark.gpu
def test_a_single_triangle_takes_every_boundary_node(built_library):
    """One triangle encloses nothing, so the node types come from a box scene; the search then has a list of one."""
    from wayverb_amd import engine as E
    box = box_in_grid("one triangle", (17, 14, 20), seed=1, fill=0.26)
    one = box.triangles[5:6].copy()
    one[0, 0] = 3
    want_nodes = box.want.first.copy()
    want = SS.oracle().boundary_index_data(want_nodes, box.dims, box.min_corner, box.spacing, one, box.vertices)
    nodes = box.want.first.copy()
    nodes["boundary_index"] = 0xdeadbeef
    got = E.boundary_index_data(box.dims, box.min_corner, box.spacing, nodes, one, box.vertices)
    assert node_difference(box, nodes, want_nodes, "nodes") is None
    for d in range(3):
        assert np.array_equal(got[d], want[d]) and np.all(got[d] == 3) and got[d].shape[0] > 0


@pytest.mark.gpu
def test_second_trip_of_the_grid_stride_loops(built_library):
    """node_inside_kernel and node_boundary_type_kernel run at most 65 536 workgroups of 256 lanes: 512 x 256 x 129 nodes are one
    plane of 131 072 more than that, so the whole top plane is the second trip's.  The box reaches through the top of the grid, so
    that plane holds inside nodes, walls and edges -- nothing a kernel that never got there could have left right."""
    dims = (512, 256, 129)
    assert dims[0] * dims[1] * (dims[2] - 1) == 65536 * 256
    spacing = 0.1
    v, t = S.box_scene((0.33, 0.27, 0.41), (50.9, 25.3, 20.0))
    t[:, 0] = np.arange(12) % 5
    case = SS.custom_case("grid stride", v, t, spacing, dims, (0.0, 0.0, 0.0), S.padded_aabb(v, 0.1), 8)
    top = case.want.nodes["boundary_type"][-dims[0] * dims[1]:]
    assert np.count_nonzero(top == 1) > 100000 and np.count_nonzero(np.isin(top, BOUNDARY_1D)) > 1000 and min(case.want.counts) > 0
    check(case, stages=("inside", "classify"))


def refusal_cases():
    v, t = S.box_scene((-5.0, -5.0, -5.0), (5.03, 5.03, 5.03))
    t[:, 0] = np.arange(12) % 4
    return {"all_inside": (v, t, (12, 10, 14), (-0.5, -0.4, -0.6)),      # the mesh grid lies wholly inside the box
            "one_wall": (v, t, (12, 10, 14), (-0.5, -0.4, 4.45))}        # ... or across one wall: 1-D nodes, no edges, no corners


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all_inside", "one_wall"])
def test_no_boundaries_is_refused_with_the_restatements_counts(built_library, name):
    """init_buffer's "No boundaries." (boundary_coefficient_finder.cpp:30-33) from both entry points, the counts they report, and
    an ordinary call right after."""
    from wayverb_amd import engine as E
    v, t, dims, mc = refusal_cases()[name]
    case = SS.custom_case(name, v, t, 0.1, dims, mc, S.padded_aabb(v, 0.1), 8)
    w = case.want
    assert min(w.counts_first) == 0 and w.counts_first == ((0, 0, 0) if name == "all_inside" else (120, 0, 0))
    assert w.counts == w.counts_first and np.count_nonzero(w.mask) == (w.mask.size if name == "all_inside" else 6 * 120)
    check(case, stages=("inside", "classify"), chain=False)
    lib = E.load_library()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    nodes = w.first.copy()
    nodes["boundary_index"] = 0xdeadbeef
    with pytest.raises(E.WaveguideError, match="No boundaries."):
        E.boundary_index_data(case.dims, case.min_corner, case.spacing, nodes, case.triangles, case.vertices)
    counts = (C.c_uint64 * 3)(7, 7, 7)
    nodes = w.first.copy()
    rc = lib.wv_boundary_index_data(*case.dims, ptr(case.min_corner), case.spacing, ptr(nodes), ptr(case.triangles),
                                    case.triangles.shape[0], ptr(case.vertices), case.vertices.shape[0], None, 0, None, 0, None, 0,
                                    counts)
    assert rc != 0 and b"No boundaries." in lib.wv_last_error()
    assert tuple(int(x) for x in counts) == w.counts

    with pytest.raises(E.WaveguideError, match="No boundaries."):
        E.SceneMesh(case.dims, case.min_corner, case.spacing, w.vox, case.aabb, case.side, case.triangles, case.vertices)
    counts = (C.c_uint64 * 3)(7, 7, 7)
    handle = C.c_void_p()
    rc = lib.wv_scene_mesh_create(*case.dims, ptr(case.min_corner), case.spacing, ptr(w.vox), w.vox.shape[0], ptr(case.aabb[0]),
                                  ptr(case.aabb[1]), case.side, ptr(case.triangles), case.triangles.shape[0], ptr(case.vertices),
                                  case.vertices.shape[0], -1, C.byref(handle), counts)
    assert rc != 0 and b"No boundaries." in lib.wv_last_error() and not handle.value
    assert tuple(int(x) for x in counts) == w.counts

    check(box_in_grid("after a refusal", (13, 12, 11), seed=3))      # nothing was left half-built


@pytest.mark.gpu
@pytest.mark.parametrize("model,spacing", [("bedroom", 0.1), ("echo_tunnel", 0.5), ("vault", 0.2)])
def test_reference_models_on_the_device(built_library, model, spacing, tmp_path):
    """The reference's demo models, laid out as tests/test_mesh_setup.py::test_setup_chain_on_reference_models lays them out for the
    reference's own kernels (voxel box = bounding box padded by 0.1, octree depth 5), through the device kernels."""
    models = unpack_reference_inputs(tmp_path, "models")
    v, t, names = S.read_obj(os.path.join(models, model + ".obj"))
    lo, hi = S.padded_aabb(v, 0.1)
    dims = tuple(int(d) for d in ((hi - lo) / np.float32(spacing)).astype(np.int32))
    case = SS.custom_case(model, v, t, spacing, dims, lo, (lo, hi), 32)
    assert 0.05 < case.want.mask.mean() < 0.95 and min(case.want.counts) > 0
    if len(names) > 1:
        assert len(np.unique(case.want.b[0])) > 1
    check(case)

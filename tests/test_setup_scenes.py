"""The random scenes of tests/setup_scenes.py, checked without a GPU before tests/test_gpu_setup_fuzz.py relies on them:
  - a tally over the seeds the GPU file uses: do the scenes reach the paths they are drawn for (ray directions after the first,
    nodes outside the voxel box, chunks of the numbering scan where re-entrant nodes outnumber 1-D nodes, exact distance ties)?
  - the host voxeliser and the kernel's voxel walk against a walk that needs neither: one voxel that lists every triangle
  - the restatement's ray diagnostic against the restatement itself."""
import numpy as np
import pytest

import setup_scenes as SS

BOUNDARY_1D = [2, 4, 8, 16, 32, 64]


def nodes_outside_voxel_box(case):
    """How many nodes the voxel walk drops at once: cell index (floor((p - c0) / cell), single precision) outside [0, side)."""
    p = SS.node_positions(case.dims, case.min_corner, case.spacing)
    c0, c1 = case.aabb
    cell = (c1 - c0) / np.float32(case.side)
    ind = np.floor((p - c0) / cell)
    return int(np.count_nonzero(np.any((ind < 0) | (ind >= case.side), axis=1)))


def reentrant_heavy_chunks(types, chunk=1024):
    """Chunks of the numbering scan (scene_mesh.hip: 1 024 nodes per workgroup) with more re-entrant than true 1-D nodes."""
    n = -(-types.shape[0] // chunk) * chunk
    t = np.zeros(n, dtype=types.dtype)
    t[:types.shape[0]] = types
    re = (t == 128).reshape(-1, chunk).sum(axis=1)
    one = np.isin(t, BOUNDARY_1D).reshape(-1, chunk).sum(axis=1)
    return int(np.count_nonzero(re > one))


@pytest.fixture(scope="module")
def survey(built_library):
    """One pass over the seeds: what each case holds, and the voxel-walk invariant's outcome on it."""
    rows = []
    o = SS.oracle()
    for seed in range(SS.SEEDS):
        case = SS.scene_case(seed, rays=True)
        w = case.want
        types = w.nodes["boundary_type"]
        row = dict(seed=seed, family=case.family, side=case.side, voxel_box=case.voxel_box, copies=case.copies,
                   reversed=case.reversed, translated=case.translated, nodes=types.shape[0], triangles=case.triangles.shape[0],
                   counts=w.counts, counts_first=w.counts_first, reentrant=int(np.count_nonzero(types == 128)),
                   ray1=int(np.count_nonzero(w.ray >= 1)), ray2=int(np.count_nonzero(w.ray >= 2)),
                   ray3=int(np.count_nonzero(w.ray >= 3)), unsure=int(np.count_nonzero(w.ray == 32)),
                   outside_voxels=nodes_outside_voxel_box(case), heavy_chunks=reentrant_heavy_chunks(types),
                   describe=SS.describe(case))
        # the diagnostic shares the loop: its flags are the plain call's
        plain = o.nodes_inside(case.dims, case.min_corner, case.spacing, w.vox, case.aabb, case.side, case.triangles, case.vertices)
        row["diagnostic_differs"] = int(np.count_nonzero(plain != w.mask))
        # one voxel that lists every triangle: no voxeliser, no walk
        whole = o.nodes_inside(case.dims, case.min_corner, case.spacing, SS.whole_list_voxels(case.triangles.shape[0]), case.aabb, 1,
                               case.triangles, case.vertices)
        row["walk_differs"] = SS.first_difference(case, w.mask, whole, "voxel lists at side %d against one voxel with every triangle" % case.side)
        if case.copies > 1:
            # the copies swapped round: every 1-D node must now take the surface of another copy, or it had no tie
            third = case.triangles.shape[0] // case.copies
            rolled = np.ascontiguousarray(np.roll(case.triangles, -third, axis=0))
            b = o.boundary_index_data(w.first.copy(), case.dims, case.min_corner, case.spacing, rolled, case.vertices)
            row["untied"] = int(np.count_nonzero(b[0] == w.b[0]))
            row["copy_of_winner"] = np.unique(w.b[0] // case.n_surfaces).tolist()
        rows.append(row)
    return rows


def test_tally_of_the_seed_range(survey):
    fam = {f: sum(r["family"] == f for r in survey) for f in SS.FAMILIES}
    sides = {s: sum(r["side"] == s for r in survey) for s in SS.SIDES}
    boxes = {k: sum(r["voxel_box"] == k for r in survey) for k in ("grid", "padded", "shifted")}
    total = lambda key: sum(r[key] for r in survey)  # noqa: E731
    print("\nset-up scenes, seeds 0..%d: %d nodes, %d triangles" % (SS.SEEDS - 1, total("nodes"), total("triangles")))
    print("  families %s\n  sides %s\n  voxel boxes %s" % (fam, sides, boxes))
    print("  translated %d, list reversed %d, list in three copies %d" % (
        sum(r["translated"] for r in survey), sum(r["reversed"] for r in survey), sum(r["copies"] > 1 for r in survey)))
    print("  nodes decided by direction >= 1: %d, >= 2: %d, >= 3: %d, by none (all unsure): %d" % (
        total("ray1"), total("ray2"), total("ray3"), total("unsure")))
    print("  seeds with nodes outside their voxel box: %d (%d nodes)" % (sum(r["outside_voxels"] > 0 for r in survey), total("outside_voxels")))
    print("  re-entrant nodes %d; seeds with a 1 024-node chunk holding more re-entrant than 1-D nodes: %d (%d chunks)" % (
        total("reentrant"), sum(r["heavy_chunks"] > 0 for r in survey), total("heavy_chunks")))
    print("  boundary nodes 1-D %d, 2-D %d, 3-D %d" % tuple(sum(r["counts"][d] for r in survey) for d in range(3)))
    assert all(fam[f] == SS.SEEDS // len(SS.FAMILIES) for f in SS.FAMILIES)
    assert all(sides[s] > 0 for s in SS.SIDES)
    assert boxes["padded"] > 0 and boxes["shifted"] > 0
    assert total("ray1") >= 100
    assert total("ray2") >= 20
    assert any(r["outside_voxels"] > 0 for r in survey)
    assert all((r["outside_voxels"] > 0) == (r["voxel_box"] != "grid") for r in survey)
    assert any(r["heavy_chunks"] > 0 for r in survey)
    assert any(r["translated"] for r in survey) and any(r["reversed"] for r in survey)
    copied = [r for r in survey if r["copies"] > 1]
    assert copied
    for r in copied:
        assert r["untied"] == 0, r["describe"]
        # ... and the winner sits in the copy that comes first in the list
        assert r["copy_of_winner"] == [r["copies"] - 1 if r["reversed"] else 0], r["describe"]
    for r in survey:
        assert min(r["counts"]) > 0 and min(r["counts_first"]) > 0, r["describe"]


@pytest.mark.parametrize("seed", range(SS.SEEDS))
def test_voxel_lists_and_walk_equal_one_voxel_with_every_triangle(survey, seed):
    """oracle.nodes_inside through the product's voxel lists at the seed's `side` against the same call with a single voxel that
    lists every triangle: a triangle missing from a voxel, or a voxel the walk skips, flips a flag.  Exact equality."""
    assert survey[seed]["walk_differs"] is None, survey[seed]["walk_differs"]


def test_ray_diagnostic_shares_the_loop(survey):
    assert all(r["diagnostic_differs"] == 0 for r in survey)
    d = SS.oracle().ray_directions()
    assert d.shape == (32, 3) and np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-5)
    assert len({tuple(row) for row in d.tolist()}) == 32


def test_scene_case_is_a_function_of_the_seed():
    attempt = SS.scene_case(7).attempt
    a = SS._draw(7, attempt)
    b = SS._draw(7, attempt)
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.triangles.tobytes() == b.triangles.tobytes()
    assert a.dims == b.dims and a.side == b.side and a.min_corner.tobytes() == b.min_corner.tobytes()

"""Random triangle scenes for the scene -> mesh kernels (node_inside.hip, mesh_setup.hip, boundary_surfaces.hip, scene_mesh.hip),
with no GPU in it: `scene_case(seed)` draws a scene, its mesh grid and its voxel box; `restate(case)` is the restatement's chain on it
(oracle/node_inside_oracle.c, mesh_setup_oracle.c, boundary_surfaces_oracle.c), stage by stage, which tests/test_gpu_setup_fuzz.py
holds the device to.  tests/test_setup_scenes.py checks on the CPU that the cases reach the paths they are drawn for.

A case:
  family               one of FAMILIES, seed % len(FAMILIES)
  vertices, triangles  float32 [n, 4], uint32 [m, 4] = {surface, v0, v1, v2}
  spacing, dims, min_corner   the mesh grid: node (x, y, z) sits at min_corner + (x, y, z) * spacing
  aabb, side           the voxel box and its cells per axis
  voxel_box            "grid" (the voxel box is the mesh grid's extent), "padded" (the geometry's bounding box padded, the mesh grid
                       reaches beyond it) or "shifted" (the mesh grid has extra layers of nodes on one side of the voxel box)
  translated, reversed, copies, n_surfaces   how the scene and its triangle list were edited

The triangle list of one seed in four holds every triangle THREE times, the copies with other surface ids, so that the nearest-triangle
search meets an exact tie at every node and the earliest copy has to win.  (Two copies would do for the tie, but then every ray crosses
every wall twice: all crossing counts are even, no node is inside and the mesh has no boundary at all.)"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle.oracle import Oracle
from wayverb_amd import scene as S

FAMILIES = ("rotated_box", "aligned_box", "icosphere", "xor", "prism", "retry")
SPACINGS = (0.25, 0.17, 0.125, 0.1, 0.07)
SIDES = (1, 3, 8, 32)
SEEDS = 120
MAX_NODES = 80000
RETRY_NODES = 300          # nodes of a "retry" scene that get triangles across their first rays
RETRY_REACH = 0.05         # how far along the ray such a triangle sits
RETRY_SIZE = 0.02          # and how large it is

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = Oracle()
    return _oracle


def rotation(rng):
    """A random rotation matrix."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _f32(verts, tris):
    v = np.zeros((len(verts), 4), dtype=np.float32)
    v[:, :3] = np.asarray(verts, dtype=np.float64).astype(np.float32)
    return v, np.ascontiguousarray(tris, dtype=np.uint32)


def _join(a, b):
    """Two scenes in one vertex / triangle list."""
    (va, ta), (vb, tb) = a, b
    tb = tb.copy()
    tb[:, 1:] += va.shape[0]
    return np.concatenate([va, vb]), np.concatenate([ta, tb])


def rotated_box(centre, half, rot):
    v, t = S.box_scene(tuple(-np.asarray(half, dtype=np.float64)), tuple(np.asarray(half, dtype=np.float64)))
    return _f32(v[:, :3].astype(np.float64) @ rot.T + centre, t)


def grid_for(vertices, spacing, anchor=None):
    """What compute_voxels_and_mesh does (as tests/test_mesh_setup.py::_grid_for): the adjusted boundary around the geometry with
    a node at the anchor (default: the centroid), mesh dimensions = extent / spacing, truncated."""
    lo = vertices[:, :3].min(axis=0)
    hi = vertices[:, :3].max(axis=0)
    if anchor is None:
        anchor = vertices[:, :3].mean(axis=0)
    c0, c1 = S.compute_adjusted_boundary(lo, hi, anchor, spacing)
    dims = tuple(int(d) for d in ((c1 - c0) / np.float32(spacing)).astype(np.int32))
    return c0, c1, dims


def node_positions(dims, min_corner, spacing):
    """float32 [n, 3]: compute_node_position as the kernels evaluate it, min_corner + float(locator) * spacing in single precision."""
    nx, ny, nz = dims
    mc = np.asarray(min_corner, dtype=np.float32)
    s = np.float32(spacing)
    ax = [mc[k] + np.arange(d, dtype=np.float32) * s for k, d in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


def retry_triangles(rng, positions, lo, hi, directions):
    """The forced-retry construction: for up to RETRY_NODES nodes p well inside the box [lo, hi], and for each of the first
    1 + n % 3 ray directions d of the n-th of them, a small open triangle whose v1-v2 edge passes through h = p + RETRY_REACH * d:
    v0 = h + w, v1 = h + e, v2 = h - e with e, w perpendicular to d.  The ray from p along d then meets the triangle where
    u + v = 1 up to rounding, which `is_degenerate` calls unsure about half the time.  Computed in double, rounded to float."""
    margin = 2 * (RETRY_REACH + RETRY_SIZE)
    p64 = positions.astype(np.float64)
    ok = np.all((p64 > lo + margin) & (p64 < hi - margin), axis=1)
    chosen = rng.permutation(np.nonzero(ok)[0])[:RETRY_NODES]
    verts, tris = [], []
    for n, i in enumerate(chosen):
        for k in range(1 + n % 3):
            d = directions[k].astype(np.float64)
            h = p64[i] + RETRY_REACH * d
            e = np.cross(d, rng.normal(size=3))
            e *= RETRY_SIZE / np.linalg.norm(e)
            w = np.cross(d, e)
            w *= RETRY_SIZE / np.linalg.norm(w)
            base = len(verts)
            verts += [h + w, h + e, h - e]
            tris.append((0, base, base + 1, base + 2))
    return _f32(verts, tris)


def _draw(seed, attempt):
    rng = np.random.default_rng([seed, attempt])
    family = FAMILIES[seed % len(FAMILIES)]
    # attributes first, so that they do not depend on what the family draws
    spacing = SPACINGS[int(rng.integers(len(SPACINGS)))]
    side = SIDES[int(rng.integers(len(SIDES)))]
    voxel_box = "grid" if rng.integers(3) else ("padded", "shifted")[int(rng.integers(2))]
    pad = float(rng.uniform(0.02, 0.12))
    shift_axis, shift_layers, shift_low = int(rng.integers(3)), int(rng.integers(1, 3)), bool(rng.integers(2))
    translated = not rng.integers(4)
    offset = rng.uniform(-60.0, 60.0, 3) if translated else np.zeros(3)
    n_surfaces = int(rng.integers(1, 12))
    reversed_list = not rng.integers(4)
    copies = 1 if rng.integers(4) else 3

    centre = rng.uniform(-1.0, 1.0, 3) + offset
    anchor = None
    box = None
    if family == "rotated_box":
        v, t = rotated_box(centre, rng.integers(10, 27, 3) * spacing / 2, rotation(rng))
    elif family == "aligned_box":
        # faces on planes of nodes: the anchor is a node, the faces lie whole cells from it (float32 arithmetic, as the grid's)
        anchor = centre.astype(np.float32)
        lo = anchor - rng.integers(5, 18, 3).astype(np.float32) * np.float32(spacing)
        hi = anchor + rng.integers(5, 18, 3).astype(np.float32) * np.float32(spacing)
        v, t = S.box_scene(tuple(lo), tuple(hi))
    elif family == "icosphere":
        v, t = S.icosphere_scene(tuple(centre), float(rng.integers(10, 37) * spacing / 2 * rng.uniform(0.9, 1.0)), int(rng.integers(4)))
    elif family == "xor":
        half = rng.integers(12, 33, 3) * spacing / 2
        a = rotated_box(centre, half, np.eye(3))
        where = centre + half * rng.uniform(-1.0, 1.0, 3)
        if rng.integers(2):
            b = S.icosphere_scene(tuple(where), float(half.min() * rng.uniform(0.6, 1.0)), int(rng.integers(1, 3)))
        else:
            b = rotated_box(where, half * rng.uniform(0.4, 0.9, 3), rotation(rng) if rng.integers(2) else np.eye(3))
        v, t = _join(a, b)
    elif family == "prism":
        n = int(rng.integers(5, 10))
        angle = np.sort(rng.uniform(0, 2 * np.pi, n))
        while np.diff(np.concatenate([angle, [angle[0] + 2 * np.pi]])).max() > 0.9 * np.pi:   # keep the centre inside
            angle = np.sort(rng.uniform(0, 2 * np.pi, n))
        radius = rng.uniform(0.35, 1.0, n) * int(rng.integers(14, 37)) * spacing / 2
        polygon = [(float(centre[0] + r * np.cos(a)), float(centre[1] + r * np.sin(a))) for r, a in zip(radius, angle)]
        height = int(rng.integers(8, 25)) * spacing
        v, t = S.prism_scene(polygon, float(centre[2] - height / 2), float(centre[2] + height / 2))
    else:
        half = rng.integers(12, 31, 3) * spacing / 2
        v, t = rotated_box(centre, half, np.eye(3))
        box = (v[:, :3].min(axis=0).astype(np.float64), v[:, :3].max(axis=0).astype(np.float64))
        anchor = v[:, :3].mean(axis=0)

    c0, c1, dims = grid_for(v, spacing, anchor)
    min_corner, aabb = c0, (c0, c1)
    if voxel_box == "padded":
        aabb = S.padded_aabb(v, pad)
    elif voxel_box == "shifted":
        dims = tuple(d + (shift_layers if k == shift_axis else 0) for k, d in enumerate(dims))
        if shift_low:
            min_corner = c0.copy()
            min_corner[shift_axis] = c0[shift_axis] - np.float32(shift_layers) * np.float32(spacing)
    if dims[0] * dims[1] * dims[2] > MAX_NODES:
        return None
    if box is not None:   # the grid is settled: put the small triangles across the rays of its nodes
        v, t = _join((v, t), retry_triangles(rng, node_positions(dims, min_corner, spacing), box[0], box[1], oracle().ray_directions()))

    t = t.copy()
    t[:, 0] = np.arange(t.shape[0]) % n_surfaces
    if copies > 1:
        parts = []
        for c in range(copies):
            part = t.copy()
            part[:, 0] += c * n_surfaces
            parts.append(part)
        t = np.concatenate(parts)
    if reversed_list:
        t = t[::-1]
    return SimpleNamespace(seed=seed, family=family, vertices=np.ascontiguousarray(v), triangles=np.ascontiguousarray(t),
                           spacing=spacing, dims=dims, min_corner=np.ascontiguousarray(min_corner, dtype=np.float32),
                           aabb=(np.ascontiguousarray(aabb[0], dtype=np.float32), np.ascontiguousarray(aabb[1], dtype=np.float32)),
                           side=side, voxel_box=voxel_box, translated=translated, reversed=reversed_list, copies=copies,
                           n_surfaces=n_surfaces)


def whole_list_voxels(n_triangles):
    """A voxel array of one cell (side = 1) that lists every triangle."""
    return np.concatenate([[1, n_triangles], np.arange(n_triangles)]).astype(np.uint32)


def restate(case, voxel_index=None, rays=False):
    """The restatement's chain on a case, every stage fed by the one before it:
      vox             the product's host voxeliser's lists (E.voxelise; pinned by test_setup_scenes.py), unless given
      mask (, ray)    oracle.nodes_inside
      first, counts_first   oracle.classify: node types and the first numbering, (1-D + re-entrant, 2-D, 3-D)
      nodes, b, counts      oracle.boundary_index_data: the final numbering, the three surface arrays and their lengths"""
    from wayverb_amd import engine as E
    o = oracle()
    c = case
    vox = E.voxelise(c.vertices, c.triangles, c.aabb, c.side) if voxel_index is None else voxel_index
    got = o.nodes_inside(c.dims, c.min_corner, c.spacing, vox, c.aabb, c.side, c.triangles, c.vertices, rays=rays)
    mask, ray = got if rays else (got, None)
    first, counts_first = o.classify(mask.astype(bool))
    nodes = first.copy()
    b = o.boundary_index_data(nodes, c.dims, c.min_corner, c.spacing, c.triangles, c.vertices)
    return SimpleNamespace(vox=vox, mask=mask, ray=ray, first=first, counts_first=counts_first, nodes=nodes, b=b,
                           counts=tuple(x.shape[0] for x in b))


@functools.lru_cache(maxsize=2)
def scene_case(seed, rays=False):
    """The case of a seed, with the restatement's chain on it as `.want`.  A draw with more than MAX_NODES nodes, or with none of
    one boundary class (the refusal's business, not this generator's), is dropped and drawn again."""
    for attempt in range(64):
        case = _draw(seed, attempt)
        if case is None:
            continue
        want = restate(case, rays=rays)
        if min(want.counts_first) > 0 and want.counts[0] > 0:
            case.want = want
            case.attempt = attempt
            return case
    raise AssertionError("seed %d: no usable scene in 64 draws" % seed)


def custom_case(name, vertices, triangles, spacing, dims, min_corner, aabb, side, restated=True):
    """A hand-made case in the generator's form (seed -1), with the restatement's chain on it unless told otherwise."""
    case = SimpleNamespace(seed=-1, family=name, vertices=np.ascontiguousarray(vertices, dtype=np.float32),
                           triangles=np.ascontiguousarray(triangles, dtype=np.uint32), spacing=spacing,
                           dims=tuple(int(d) for d in dims), min_corner=np.ascontiguousarray(min_corner, dtype=np.float32),
                           aabb=(np.ascontiguousarray(aabb[0], dtype=np.float32), np.ascontiguousarray(aabb[1], dtype=np.float32)),
                           side=side, voxel_box="custom", translated=False, reversed=False, copies=1, n_surfaces=0, attempt=0)
    if restated:
        case.want = restate(case)
    return case


def grid_extent(dims, min_corner, spacing):
    """The box a mesh grid covers, as a voxel box."""
    mc = np.asarray(min_corner, dtype=np.float32)
    return mc, mc + np.asarray(dims, dtype=np.float32) * np.float32(spacing)


def describe(case):
    return "seed %d (%s, draw %d): dims %s, spacing %g, side %d, voxel box %s, %d triangles%s%s%s" % (
        case.seed, case.family, case.attempt, case.dims, case.spacing, case.side, case.voxel_box, case.triangles.shape[0],
        ", translated" if case.translated else "", ", list reversed" if case.reversed else "",
        ", %d copies" % case.copies if case.copies > 1 else "")


def first_difference(case, got, want, what):
    """None when the per-node arrays are equal, else a line naming the case and the first node that differs, with its position."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    nx, ny, _ = case.dims
    loc = (i % nx, (i // nx) % ny, i // (nx * ny))
    pos = case.min_corner + np.array(loc, dtype=np.float32) * np.float32(case.spacing)
    return "%s: %d of %d nodes differ, first node %d at locator %s, position %s: got %s, want %s\n  %s" % (
        what, bad.size, got.size, i, loc, tuple(float(p) for p in pos), got[i], want[i], describe(case))

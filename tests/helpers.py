"""Shared test plumbing: run a golden case through the oracle or the engine."""
import hashlib
import os
import tarfile

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def unpack_reference_inputs(dest, prefix):
    """The members of tests/golden/reference_inputs.tar.xz under `prefix` (data files of the reference tree: demo project bundles,
    demo models, boundary_test plots; tests/golden/README.md) unpacked into the directory `dest`.  Returns dest/prefix."""
    with tarfile.open(os.path.join(GOLDEN, "reference_inputs.tar.xz")) as t:
        members = [m for m in t.getmembers() if m.name == prefix or m.name.startswith(prefix + "/")]
        if hasattr(tarfile, "data_filter"):
            t.extractall(dest, members=members, filter="data")
        else:
            t.extractall(dest, members=members)
    return os.path.join(str(dest), prefix)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def set_tuning(**fields):
    """Tuning (wv_tuning fields of include/wayverb_amd.h, plus stream_variant) of every engine created from now on, through
    wayverb_amd.engine.default_tuning -> wv_options::tuning.  No arguments: the library's defaults."""
    from wayverb_amd import engine as E
    E.default_tuning.clear()
    E.default_tuning.update({k: int(v) for k, v in fields.items()})


def initial_fields(case, dtype):
    n = case["mesh"].num_nodes
    if case["init"] is None:
        return np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    return case["init"][0].astype(dtype), case["init"][1].astype(dtype)


def run_oracle(oracle, case, dtype, threads=1):
    mesh = case["mesh"]
    prev, cur = initial_fields(case, dtype)
    bd = [mesh.boundary_data(d) for d in (1, 2, 3)]
    steps, flag, out = oracle.run(prev, cur, mesh, bd, case["source_kind"], case["source_node"],
                                  case["signal"], case["steps"], case["recv"], threads=threads)
    final_cur, final_prev = (cur, prev) if steps % 2 == 0 else (prev, cur)
    return dict(steps=steps, flag=flag, trace=out, current=final_cur, previous=final_prev, bd=bd)


def run_engine(case, precision, **engine_kw):
    from wayverb_amd import engine as E
    mesh = case["mesh"]
    dtype = np.float32 if precision == "f32" else np.float64
    eng = E.Engine(mesh, precision=precision, **engine_kw)
    try:
        if case["init"] is not None:
            prev, cur = initial_fields(case, dtype)
            eng.write_field(prev, E.BUF_PREVIOUS)
            eng.write_field(cur, E.BUF_CURRENT)
        steps, out = E.run_fast(eng, case["source_kind"], case["source_node"], case["signal"], case["recv"])
        return dict(steps=steps, flag=0, trace=out.astype(dtype),
                    current=eng.read_field(E.BUF_CURRENT), previous=eng.read_field(E.BUF_PREVIOUS),
                    bd=[eng.read_boundary_data(d) for d in (1, 2, 3)],
                    passes=eng.query(E.Engine.QUERY_PASSES), triple_passes=eng.query(E.Engine.QUERY_TRIPLE_PASSES),
                    xwall_entries=eng.query(E.Engine.QUERY_XWALL_ENTRIES))
    finally:
        eng.close()


def box_boundary_rows_below(nx, ny, nz, z, d):
    """Number of D-dimensional boundary nodes of an nx*ny*nz box in planes [0, z) = the boundary_index
    of the first such node of plane z (set_boundary_index numbers them in node order)."""
    per_face_plane = {1: (nx - 4) * (ny - 4), 2: 2 * (nx - 4) + 2 * (ny - 4), 3: 4}[d]
    per_mid_plane = {1: 2 * (nx - 4) + 2 * (ny - 4), 2: 4, 3: 0}[d]
    total = 0
    if z > 1:
        total += per_face_plane
    total += per_mid_plane * max(0, min(z, nz - 2) - 2)
    if z > nz - 2:
        total += per_face_plane
    return total


def canonical_parameters():
    """What canonical() passes on: a float spacing for the 200 Hz / 0.6 waveguide, its sample rate, core::environment's density."""
    from wayverb_amd import simulation as W
    env = W.Environment()
    spacing = float(np.float32(W.grid_spacing(env.speed_of_sound, 1.0 / W.compute_sampling_frequency(200.0, 0.6))))
    return spacing, W.compute_sample_rate(spacing, env.speed_of_sound), env.ambient_density


def subsample(planes, plan, dims):
    """What the plan takes of a whole field [nz, ny, nx]."""
    (x0, y0, z0), extent = plan.get("box", "mesh") if plan.get("box", "mesh") != "mesh" else ((0, 0, 0), None)
    extent = extent or (None, None, None)
    ex, ey, ez = [dims[a] - o if e is None else e for a, (o, e) in enumerate(zip((x0, y0, z0), extent))]
    stride = plan.get("stride", 1)
    sx, sy, sz = (stride,) * 3 if np.isscalar(stride) else stride
    return planes[z0:z0 + ez:sz, y0:y0 + ey:sy, x0:x0 + ex:sx]


def numpy_fold(snaps, steps, freqs):
    """The definition of a field spectrum: re[k] = re[k] + p_j * c(j, k), im[k] = im[k] - p_j * s(j, k), j in capture order, in double."""
    from wayverb_amd import engine as E
    shape = (len(freqs),) + tuple(snaps.shape[1:])
    re, im = np.zeros(shape), np.zeros(shape)
    for p, step in zip(snaps, steps):
        p = p.astype(np.float64)
        for k, f in enumerate(freqs):
            c, s = E.spectrum_twiddle(f, int(step))
            re[k] = re[k] + p * c
            im[k] = im[k] - p * s
    out = np.empty(shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def numpy_bins(snaps, n_bins, bin_captures):
    """The definition of a decay map: capture j goes to bin min(j // W, n_bins - 1); E[b] = E[b] + p_j * p_j in capture order, in
    double, from +0.0."""
    out = np.zeros((n_bins,) + tuple(snaps.shape[1:]))
    for j, p in enumerate(snaps):
        p = p.astype(np.float64)
        b = min(j // bin_captures, n_bins - 1)
        out[b] = out[b] + p * p
    return out

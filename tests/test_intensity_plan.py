"""Intensity maps, the parts that need no GPU: the planning header (wayverb_amd/csrc/intensity_plan.h) against hand-derived cases, the
new entry points and wv_intensity_plan's layout, both kernels' text run on the host against the NumPy definition, their resource
usage as the build reported it, the Python layer's box -> shape, and the definition held to physics on the CPU oracle's field.
(An engine needs a device: what wv_set_intensity does with a plan is tests/test_gpu_intensity.py's.)"""
import ctypes
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from wayverb_amd import intensity as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")

NEW = ("wv_set_intensity", "wv_intensity_count", "wv_fetch_intensity", "wv_fetch_intensity_velocity", "wv_fetch_directional_velocity")


def test_intensity_planning_header_against_hand_derived_cases():
    """tests/cpp/intensity_plan_test.cpp: every WV_E_INVALID_ARGUMENT case of a plan -- n_bins, bin_captures, strides, period, the
    three physical constants (zero, negative, infinite, NaN), a box that leaves the mesh, and a taken node with a neighbour off the
    grid on each of the six sides at stride 1 and at stride 3, with the reference's sentence -- and the sizes and the traffic model."""
    src = os.path.join(ROOT, "tests", "cpp", "intensity_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "intensity_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "INTENSITY PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    # the plan's header is host code: no HIP in it; the engine file keeps no stage bookkeeping of its own; one launch site per kernel
    assert "hip" not in open(os.path.join(CSRC, "intensity_plan.h")).read().split("#pragma once")[1].lower()
    text = open(os.path.join(CSRC, "engine_intensity.hip.h")).read()
    for word in ("spectrum_good_captures", "steps.push_back", "hipEventElapsedTime", "plan_batch_end(", "begin_run("):
        assert word not in text, word
    shared = open(os.path.join(CSRC, "engine_staged.hip.h")).read()   # (the life cycle's one copy, on capture_stage.h's bookkeeping)
    assert ".st." in shared and "launch_intensity_gather(" in shared and "spectrum_good_captures" not in shared and "steps.push_back" not in shared
    for kernel, where in (("intensity_gather_kernel", "engine_snapshot.hip.h"), ("intensity_fold_kernel", "engine_intensity.hip.h")):
        launches = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip")) and
                    re.search(r"hipLaunchKernelGGL\(\(?wv::%s\b" % kernel, open(os.path.join(CSRC, name)).read())]
        assert launches == [where]


def test_intensity_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_intensity", "intensity_count", "fetch_intensity", "fetch_intensity_velocity", "fetch_directional_velocity"):
        assert callable(getattr(E.Engine, method))
    for fn in ("hull_box", "intensity_bins", "net_intensity", "arrival_direction", "diffuseness"):
        assert callable(getattr(I, fn))
    assert (E.Engine.QUERY_INTENSITY_CAPTURES, E.Engine.QUERY_INTENSITY_FOLDS, E.Engine.QUERY_INTENSITY_NS,
            E.Engine.QUERY_INTENSITY_GATHER_NS, E.Engine.QUERY_INTENSITY_GATHERS) == (32, 33, 34, 35, 36)


def test_intensity_plan_struct_has_the_documented_size_and_offsets():
    """wv_intensity_plan as a C compiler lays the header's declaration out: wv_decay_plan's 64 bytes, field for field, then three
    doubles -- 88 bytes -- and the ctypes mirror agrees; wv_decay_plan itself is unchanged; the query ids follow 31."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_bins", "bin_captures",
              "spacing", "sample_rate", "ambient_density"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu %zu\", sizeof(wv_intensity_plan), sizeof(wv_decay_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_intensity_plan, %s));' % f for f in fields) + \
        "".join('printf(" %%zu", offsetof(wv_decay_plan, %s));' % f for f in fields[:13]) + \
        'printf(" %d %d %d %d %d", WV_QUERY_INTENSITY_CAPTURES, WV_QUERY_INTENSITY_FOLDS, WV_QUERY_INTENSITY_NS, ' \
        'WV_QUERY_INTENSITY_GATHER_NS, WV_QUERY_INTENSITY_GATHERS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60]
    assert got == [88, 64] + offsets + [64, 72, 80] + offsets + [32, 33, 34, 35, 36]
    assert [ctypes.sizeof(E.WvIntensityPlan)] + [getattr(E.WvIntensityPlan, f).offset for f in fields] == [88] + offsets + [64, 72, 80]


def kernel_names(block):
    return block.split()[0]


def test_both_kernels_need_no_scratch_and_spill_nothing(built_library):
    """The compiler's resource metadata for intensity_gather_kernel (one instance per field precision) and intensity_fold_kernel,
    written beside the library by wayverb_amd.build: ScratchSize 0, no VGPR and no SGPR spill, no LDS, at most the 128 VGPRs that
    keep four waves per SIMD.  profiles/r12/intensity_kernel_resources.txt records what a build for gfx950 reported."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "intensity_" in kernel_names(b)]
    assert sorted("gather" if "intensity_gather_kernel" in kernel_names(b) else "fold" for b in blocks) == ["fold", "gather", "gather"]
    for b in blocks:
        for what in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill", r"LDS Size \[bytes/block\]"):
            assert int(re.search(what + r": (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 128, b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 4, b
    recorded = open(os.path.join(ROOT, "profiles", "r12", "intensity_kernel_resources.txt")).read()
    assert recorded.count("Function Name:") == 3 and recorded.count("ScratchSize [bytes/lane]: 0") == 3
    assert recorded.count("VGPRs Spill: 0") == 3 and recorded.count("SGPRs Spill: 0") == 3


# (B = nx ny nz taken, strides) x (n_bins, W) x Real; captures 37 = 16 + 16 + 5; a short first fold and a small grid (stride loops) once each
KERNEL_BOXES = [((10, 9, 7), (1, 1, 1)), ((9, 9, 7), (1, 1, 1)), ((1, 1, 1), (1, 1, 1)), ((257, 1, 1), (1, 1, 1)),
                ((10, 9, 7), (1, 2, 3)), ((9, 9, 7), (1, 2, 3)), ((1, 1, 1), (1, 2, 3)), ((257, 1, 1), (1, 2, 3))]
KERNEL_LAYOUTS = [(33, 1), (7, 5), (2, 17), (1, 1)]


@pytest.fixture(scope="module")
def kernel_host():
    exe = os.path.join(ROOT, "tests", "cpp", "intensity_kernel_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "intensity_kernel_host.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("real", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("taken,stride", KERNEL_BOXES, ids=["B%d-stride%d%d%d" % ((t[0] * t[1] * t[2],) + s) for t, s in KERNEL_BOXES])
def test_the_kernels_text_on_the_host_reproduces_the_definition_bytewise(kernel_host, tmp_path, taken, stride, real):
    """tests/cpp/intensity_kernel_host.cpp: both kernels' text compiled for the host, one call per lane, a capture per field and a fold
    per 16 captures, against intensity.intensity_bins: bins AND velocities bytewise for B = 630 / 567 / 1 / 257, strides (1, 1, 1) and
    (1, 2, 3), four bin layouts, float and double fields with padded rows whose padding holds NaN.  The box sits at (2, 1, 3) of a
    mesh that is its hull plus a margin, so a wrong neighbour offset reads a wrong value, not the same one."""
    rng = np.random.default_rng(taken[0] * 7 + stride[2])
    origin = (2, 1, 3)
    hull, box_in_hull = I.hull_box((origin, taken), stride)
    mesh = tuple(o + e + m for o, e, m in zip(hull[0], hull[1], (1, 2, 0)))          # (x, y, z)
    pitch = mesh[0] + 5
    T = 37
    smooth = rng.standard_normal((T, 1, 1, 1)) * 10.0 ** rng.integers(-30, 3, (T, 1, 1, 1))
    fields = np.full((T, mesh[2], mesh[1], pitch), np.nan, dtype=real)
    fields[..., :mesh[0]] = (smooth * (1.0 + 1e-2 * rng.standard_normal((T,) + mesh[::-1]))).astype(real)
    spacing, k = 0.0567, 1.225 * 10573.0
    region = tuple(slice(o, o + e) for o, e in zip(hull[0][::-1], hull[1][::-1]))
    snaps = np.ascontiguousarray(fields[(slice(None),) + region].astype(np.float32))
    nodes = taken[0] * taken[1] * taken[2]
    for case, (n_bins, w) in enumerate(KERNEL_LAYOUTS):
        first_fold, grid = (13, (1, 2)) if case == 1 else (16, (0, 0))
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<19Q2d", np.dtype(real).itemsize, mesh[1], mesh[2], pitch, *origin, *taken, *stride, n_bins, w, T, first_fold,
                                *grid, spacing, k) + fields.tobytes())
        subprocess.run([kernel_host, fin, fout], check=True, timeout=300)
        raw = np.fromfile(fout)
        assert raw.shape == (4 * n_bins * nodes + 3 * nodes,)
        want, want_v = I.intensity_bins(snaps, box_in_hull, spacing, 10573.0, 1.225, n_bins, w, return_velocity=True)
        assert want.shape == (4, n_bins) + taken[::-1]
        assert raw[:4 * n_bins * nodes].tobytes() == want.tobytes(), (n_bins, w)
        assert raw[4 * n_bins * nodes:].tobytes() == want_v.tobytes(), (n_bins, w)
        assert all(np.abs(want[a]).max() > 0 for a in range(4)) and np.isfinite(want).all() and np.abs(want_v).min() > 0


def test_python_box_and_stride_to_shape():
    """Engine.set_intensity turns (origin, extent, stride) into nodes taken per axis as set_snapshots does, (4, n_bins) in front; with
    no box it takes the mesh's interior; the three constants go into the plan as doubles."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_intensity(self, handle, plan):
            self.plan = plan._obj if plan is not None else None
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    const = dict(spacing=0.05, sample_rate=4000.0, ambient_density=1.225)
    assert eng.set_intensity(12, 4, **const) == (4, 12, 26, 18, 22)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz) == (1, 1, 1, 22, 18, 26, 1, 1, 1)
    assert eng.set_intensity(4096, 17, box=((1, 1, 2), (21, 18, 24)), stride=(1, 2, 3), first_step=5, period=7, **const) == (4, 4096, 8, 9, 21)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.n_bins, p.bin_captures) == \
        (1, 1, 2, 21, 9, 8, 1, 2, 3, 5, 7, 4096, 17)
    assert (p.spacing, p.sample_rate, p.ambient_density) == (0.05, 4000.0, 1.225)
    assert eng.fetch_intensity_velocity.__doc__ and eng.intensity_shape == (4, 4096, 8, 9, 21)
    assert eng.set_intensity(None) is None and eng.lib.plan is None and eng.intensity_shape is None
    eng.h = None


def test_canonical_fills_in_the_plan():
    """simulation.intensity_plan_arguments: a plane in metres becomes that plane less its rim; the bins are bin_seconds long or the run
    in n_bins bins; spacing, sample_rate / every and the environment's density are filled in; a plane on the floor is refused."""
    from wayverb_amd import simulation as W

    class Mesh:
        dims, spacing, min_corner = (24, 20, 28), 0.05, (0.0, -0.5, 1.0)

    env = W.Environment()
    plan = W.intensity_plan_arguments(dict(plane=1.55, every=3, n_bins=5), Mesh, 12000.0, env, 40 / 12000.0)
    assert plan == dict(n_bins=5, bin_captures=3, box=((1, 1, 11), (22, 18, 1)), stride=1, first_step=0, period=3, spacing=0.05,
                        sample_rate=4000.0, ambient_density=env.ambient_density)          # 40 steps: captures of 0, 3, .., 39 = 14
    plan = W.intensity_plan_arguments(dict(box=((1, 1, 1), (4, 4, 4)), bin_seconds=0.001), Mesh, 12000.0, env, 0.01)
    assert (plan["n_bins"], plan["bin_captures"], plan["period"], plan["sample_rate"], plan["box"]) == (11, 12, 1, 12000.0, ((1, 1, 1), (4, 4, 4)))
    assert W.intensity_plan_arguments(dict(plane=1.5, bin_seconds=1e-6), Mesh, 12000.0, env, 1.0)["n_bins"] == 4096
    for bad in (dict(plane=1.0), dict(plane=2.35), dict(), dict(plane=1.5, box=((1, 1, 1), (2, 2, 2))), dict(plane=1.5, window=3), dict(plane=1.5, every=0)):
        with pytest.raises(ValueError):
            W.intensity_plan_arguments(bad, Mesh, 12000.0, env, 0.01)


def test_a_ricker_pulse_in_a_box_carries_its_energy_outwards(oracle):
    """The definition held to physics, on the CPU oracle's field: a 48^3 box mesh, a soft source at the centre node with the Ricker
    signal (1 - 2 a^2) exp(-a^2), a = pi 0.08 (n - 12), 40 steps (the front has not reached a wall), every step captured, one bin.
    Over every node 5 <= r <= 10 spacings from the source the net intensity points outwards -- cosine with the radial vector >= 0.999:
    the sign of the velocity and the axis order of the ports -- and rho c |sum I| / sum E lies in [0.8, 1.0]: the constants k and
    spacing (short of 1 by the integrator's half-step phase and the near field; measured 0.870 .. 0.937 over 3 684 nodes)."""
    from test_receiver_arrays_host import canonical_parameters
    from wayverb_amd import mesh as M
    from wayverb_amd import simulation as W
    spacing, rate, density = canonical_parameters()
    mesh = M.box_mesh(48, 48, 48, spacing=spacing)
    n = np.arange(40)
    a = np.pi * 0.08 * (n - 12)
    signal = (1.0 - 2.0 * a * a) * np.exp(-a * a)
    src = mesh.compute_index(24, 24, 24)
    prev, cur = np.zeros(mesh.num_nodes), np.zeros(mesh.num_nodes)
    bd = [mesh.boundary_data(d) for d in (1, 2, 3)]
    origin, taken = (13, 13, 13), (23, 23, 23)                 # every node within 10 spacings, and one more
    hull, box_in_hull = I.hull_box((origin, taken))
    region = tuple(slice(o, o + e) for o, e in zip(hull[0][::-1], hull[1][::-1]))
    snaps = np.zeros((41,) + hull[1][::-1], dtype=np.float32)
    for s in range(40):
        snaps[s] = cur.reshape(48, 48, 48)[region]             # the capture of step s: before the source's sample of step s goes in
        cur[src] += signal[s]
        assert oracle.step(prev, cur, mesh, bd) == 0
        prev, cur = cur, prev
    snaps[40] = cur.reshape(48, 48, 48)[region]
    bins = I.intensity_bins(snaps, box_in_hull, spacing, rate, density, 1, 1)
    total, mag, direction = I.net_intensity(bins)
    z, y, x = np.meshgrid(*(np.arange(13, 36) - 24,) * 3, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    ring = (r >= 5) & (r <= 10)
    assert ring.sum() == 3684
    cosine = ((direction[0] * x + direction[1] * y + direction[2] * z) / np.where(r > 0, r, 1))[ring]
    ratio = 1.0 - I.diffuseness(bins, W.Environment().speed_of_sound, density)[ring]
    print("cosine min %.17g; rho c |I| / E %.4f .. %.4f" % (cosine.min(), ratio.min(), ratio.max()))
    assert cosine.min() >= 0.999
    assert ratio.min() >= 0.8 and ratio.max() <= 1.0

"""Field spectra, the parts that need no GPU: the planning header (wayverb_amd/csrc/spectrum_plan.h) against hand-derived cases, the
new entry points and wv_spectrum_plan's layout, the twiddle function against NumPy, the fold kernel's resource usage, and the Python
layer's box / stride -> shape, Hz -> cycles per step and alias refusal."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spectrum_planning_header_against_hand_derived_cases():
    """tests/cpp/spectrum_plan_test.cpp: free slots -> captures of a batch, when a fold is due, whole runs around the stage size
    (1, 16, 17, 33 captures), the good captures after a stop at step f, the table's size and indexing, B and byte counts with
    overflow-safe 64-bit arithmetic, the traffic bound's figures.  The header needs nothing but the standard library."""
    src = os.path.join(ROOT, "tests", "cpp", "spectrum_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "spectrum_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "wayverb_amd", "csrc"), src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "SPECTRUM PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    header = open(os.path.join(ROOT, "wayverb_amd", "csrc", "spectrum_plan.h")).read()
    assert sorted(re.findall(r"#include [<\"]([^>\"]+)[>\"]", header)) == ["cstdint", "limits"]


def test_spectrum_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    for name in ("wv_set_spectrum", "wv_spectrum_count", "wv_fetch_spectrum", "wv_spectrum_twiddle"):
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_spectrum", "spectrum_count", "fetch_spectrum"):
        assert callable(getattr(E.Engine, method))
    assert callable(E.spectrum_twiddle)
    assert (E.Engine.QUERY_SPECTRUM_CAPTURES, E.Engine.QUERY_SPECTRUM_FOLDS, E.Engine.QUERY_SPECTRUM_NS) == (26, 27, 28)


def test_spectrum_plan_struct_has_the_documented_size_and_offsets():
    """wv_spectrum_plan as a C compiler lays the header's declaration out: 64 bytes, nine int32 from 0, first_step at 40 (8-aligned
    behind them), period at 48, n_freqs at 56, reserved at 60 -- and the ctypes mirror agrees; the query ids are the documented ones."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_freqs", "reserved"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_spectrum_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_spectrum_plan, %s));' % f for f in fields) + \
        'printf(" %d %d %d", WV_QUERY_SPECTRUM_CAPTURES, WV_QUERY_SPECTRUM_FOLDS, WV_QUERY_SPECTRUM_NS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [64, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 26, 27, 28]
    assert [ctypes.sizeof(E.WvSpectrumPlan)] + [getattr(E.WvSpectrumPlan, f).offset for f in fields] == got[:14]


@pytest.mark.parametrize("f", [0.0, 0.5, 0.125, 0.0371, 1.0 / 3.0])
def test_twiddle_against_numpy_evaluating_the_same_three_operations(built_library, f):
    """x = f * step; x -= floor(x); cos / sin of 2 pi x.  The argument is the same double on both sides; the library's libm and NumPy
    are each within an ulp of the true value, and |value| <= 1, so they differ by 2^-51 at the most.  f = 0 gives exactly (1, 0)."""
    from wayverb_amd import engine as E
    steps = np.unique(np.concatenate([np.arange(0, 300), np.arange(999_700, 1_000_001), np.arange(0, 1_000_001, 977)])).astype(np.uint64)
    x = np.float64(f) * steps.astype(np.float64)
    x = x - np.floor(x)
    angle = 2.0 * np.pi * x
    want_c, want_s = np.cos(angle), np.sin(angle)
    got = np.array([E.spectrum_twiddle(f, int(s)) for s in steps])
    worst = max(np.abs(got[:, 0] - want_c).max(), np.abs(got[:, 1] - want_s).max())
    print("f = %r: largest difference %g over %d steps" % (f, worst, len(steps)))
    assert worst <= 2.0 ** -51
    assert np.abs(got).max() <= 1.0
    if f == 0.0:
        assert (got[:, 0] == 1.0).all() and (got[:, 1] == 0.0).all() and not np.signbit(got[:, 1]).any()


def test_fold_kernel_needs_neither_scratch_nor_lds(built_library):
    """The compiler's account of spectrum_fold_kernel (both instances: one or two nodes per lane; the kernel does not depend on the
    field's precision, so the one library holds what both precisions run), written beside the library by wayverb_amd.build.  The tuned
    form (frequency chunk 4) comes out at 62 VGPRs with one node per lane and 106 with two: the cap is the 128 that keep four waves
    per SIMD, the margin test_snapshot_plan.py leaves its kernel."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "spectrum_fold_kernel" in b.split()[0]]
    assert len(blocks) == 2
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 128, b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 4, b


def test_python_box_and_stride_to_shape():
    """Engine.set_spectrum turns (origin, extent, stride) into nodes taken per axis as set_snapshots does, K in front."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_spectrum(self, handle, plan, freqs):
            self.plan = plan._obj if plan is not None else None
            self.freqs = None if freqs is None else np.ctypeslib.as_array(ctypes.cast(freqs, ctypes.POINTER(ctypes.c_double)), (self.plan.n_freqs,)).copy()
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    assert eng.set_spectrum([0.1, 0.2]) == (2, 28, 20, 24)
    assert eng.set_spectrum([0.25], box="mesh", stride=3) == (1, 10, 7, 8)
    assert eng.set_spectrum([0.0, 0.5, 0.125], box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3), first_step=5, period=7) == (3, 9, 10, 21)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.n_freqs) == (1, 0, 2, 21, 10, 9, 1, 2, 3, 5, 7, 3)
    assert list(eng.lib.freqs) == [0.0, 0.5, 0.125]
    assert eng.set_spectrum([0.3], box=((0, 0, 5), (None, None, 1))) == (1, 1, 20, 24)
    assert eng.set_spectrum(None) is None and eng.lib.plan is None and eng.spectrum_shape is None
    eng.h = None


def test_hz_to_cycles_per_step_and_the_alias_refusal():
    """simulation.spectrum_plan_arguments: freqs_hz / sample_rate, everything else passed through; a frequency above half the sample
    rate divided by the period is refused with the frequency it would alias to."""
    from wayverb_amd import simulation as W
    plan = W.spectrum_plan_arguments(dict(freqs_hz=[0.0, 100.0, 2000.0], box="mesh", stride=2, period=2), 8000.0)
    assert list(plan["freqs"]) == [0.0, 100.0 / 8000.0, 0.25] and plan["box"] == "mesh" and plan["stride"] == 2 and plan["period"] == 2
    assert "freqs_hz" not in plan
    assert list(W.spectrum_plan_arguments(dict(freqs_hz=4000.0), 8000.0)["freqs"]) == [0.5]
    with pytest.raises(ValueError, match=r"aliases to 1900 Hz"):
        W.spectrum_plan_arguments(dict(freqs_hz=[100.0, 2100.0], period=2), 8000.0)     # sampled at 4000 Hz: 2100 -> 1900
    with pytest.raises(ValueError, match=r"aliases to 3999 Hz"):
        W.spectrum_plan_arguments(dict(freqs_hz=[4001.0]), 8000.0)
    with pytest.raises(ValueError):
        W.spectrum_plan_arguments(dict(freqs_hz=[-1.0]), 8000.0)
    with pytest.raises(ValueError, match="nan is not a frequency"):
        W.spectrum_plan_arguments(dict(freqs_hz=[100.0, float("nan")]), 8000.0)
    with pytest.raises(ValueError, match="inf is not a frequency"):
        W.spectrum_plan_arguments(dict(freqs_hz=[float("inf")]), 8000.0)
    with pytest.raises(ValueError):
        W.spectrum_plan_arguments(dict(box="mesh"), 8000.0)

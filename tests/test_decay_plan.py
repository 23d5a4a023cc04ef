"""Energy decay maps, the parts that need no GPU: the planning header (wayverb_amd/csrc/decay_plan.h) and the shared stage bookkeeping
(capture_stage.h) against hand-derived cases, the new entry points and wv_decay_plan's layout, the fold kernel's resource usage, and
the Python layer's box / stride -> shape."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")


def test_decay_planning_header_against_hand_derived_cases():
    """tests/cpp/decay_plan_test.cpp: the bin of a capture for W = 1, 5, 16, 17, the open-ended last bin, B and byte counts with
    overflow-safe 64-bit arithmetic, the distinct bins of a fold and the traffic model's figures, and the stage bookkeeping the
    spectrum and the decay plan share.  decay_plan.h needs nothing but the standard library; the stage's integer rules are
    spectrum_plan.h's, which capture_stage.h takes as they are."""
    src = os.path.join(ROOT, "tests", "cpp", "decay_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "decay_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DECAY PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    includes = lambda name: sorted(re.findall(r"#include [<\"]([^>\"]+)[>\"]", open(os.path.join(CSRC, name)).read()))   # noqa: E731
    assert includes("decay_plan.h") == ["cstdint", "limits"]
    assert includes("capture_stage.h") == ["cstdint", "snapshot_plan.h", "spectrum_plan.h", "vector"]
    # one copy of the stage's bookkeeping and of the life cycle around it: no plan's engine file keeps staged steps or a committed count
    # of its own, times a fold, cuts a batch or enters a run; engine_staged.hip.h makes every call into the stage's bookkeeping
    for name in ("engine_spectrum.hip.h", "engine_decay.hip.h", "engine_intensity.hip.h", "engine_arrival.hip.h", "engine_lateral.hip.h"):
        text = open(os.path.join(CSRC, name)).read()
        for word in ("spectrum_good_captures", "steps.push_back", "hipEventElapsedTime", "plan_batch_end(", "begin_run("):
            assert word not in text, (name, word)
    shared = open(os.path.join(CSRC, "engine_staged.hip.h")).read()
    for call in (".st.start(", ".st.full()", ".st.slot()", ".st.staged(", ".st.drop_uncommitted()", ".st.fold_due()", ".st.plan_batch_end(", ".st.begin_run(",
                 ".st.commit(", ".st.all_folded()", ".st.captures()", ".st.rollback("):
        assert call in shared, call
    assert "spectrum_good_captures" not in shared and "steps.push_back" not in shared
    # ... and one launch site of the capture kernel
    launches = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip")) and
                "hipLaunchKernelGGL((wv::snapshot_gather_kernel" in open(os.path.join(CSRC, name)).read()]
    assert launches == ["engine_snapshot.hip.h"]


def test_decay_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in ("wv_set_decay", "wv_decay_count", "wv_fetch_decay"):
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_decay", "decay_count", "fetch_decay"):
        assert callable(getattr(E.Engine, method))
    assert (E.Engine.QUERY_DECAY_CAPTURES, E.Engine.QUERY_DECAY_FOLDS, E.Engine.QUERY_DECAY_NS) == (29, 30, 31)


def test_decay_plan_struct_has_the_documented_size_and_offsets():
    """wv_decay_plan as a C compiler lays the header's declaration out: 64 bytes, nine int32 from 0, first_step at 40 (8-aligned
    behind them), period at 48, n_bins at 56, bin_captures at 60 -- and the ctypes mirror agrees; the query ids follow 28."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_bins", "bin_captures"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_decay_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_decay_plan, %s));' % f for f in fields) + \
        'printf(" %d %d %d", WV_QUERY_DECAY_CAPTURES, WV_QUERY_DECAY_FOLDS, WV_QUERY_DECAY_NS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [64, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 29, 30, 31]
    assert [ctypes.sizeof(E.WvDecayPlan)] + [getattr(E.WvDecayPlan, f).offset for f in fields] == got[:14]


def test_fold_kernel_needs_neither_scratch_nor_lds(built_library):
    """The compiler's account of decay_fold_kernel (both instances: one or two nodes per lane; the kernel does not depend on the
    field's precision), written beside the library by wayverb_amd.build: no scratch, no LDS, at most the 128 VGPRs that keep four
    waves per SIMD -- the bar tests/test_spectrum_plan.py holds the spectrum fold to, which has the same 16 staged values per lane.
    profiles/r10/decay_kernel_resources.txt records what the build reported (24 VGPRs with one node per lane, 74 with two)."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "decay_fold_kernel" in b.split()[0]]
    assert len(blocks) == 2
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 128, b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 4, b


def test_python_box_and_stride_to_shape():
    """Engine.set_decay turns (origin, extent, stride) into nodes taken per axis as set_snapshots does, n_bins in front."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_decay(self, handle, plan):
            self.plan = plan._obj if plan is not None else None
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    assert eng.set_decay(12, 4) == (12, 28, 20, 24)
    assert eng.set_decay(3, 1, box="mesh", stride=3) == (3, 10, 7, 8)
    assert eng.set_decay(4096, 17, box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3), first_step=5, period=7) == (4096, 9, 10, 21)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.n_bins, p.bin_captures) == \
        (1, 0, 2, 21, 10, 9, 1, 2, 3, 5, 7, 4096, 17)
    assert eng.set_decay(2, 2, box=((0, 0, 5), (None, None, 1))) == (2, 1, 20, 24)
    assert eng.set_decay(None) is None and eng.lib.plan is None and eng.decay_shape is None
    eng.h = None

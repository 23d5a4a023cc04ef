"""Field snapshots, the parts that need no GPU: the planning header (wayverb_amd/csrc/snapshot_plan.h) against hand-derived cases, the
new entry points and wv_snapshot_plan's layout, the capture kernel's resource usage."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_snapshot_planning_header_against_hand_derived_cases():
    """tests/cpp/snapshot_plan_test.cpp: the first step is included when equal to the current count; batch cuts land exactly on snapshot
    steps for periods 1, 2, 3, 7, 64 and for batches longer and shorter than the period; box validation at every mesh face; output
    shapes with strides that do and do not divide the box.  The header needs nothing but the standard library."""
    src = os.path.join(ROOT, "tests", "cpp", "snapshot_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "snapshot_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "wayverb_amd", "csrc"), src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "SNAPSHOT PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    header = open(os.path.join(ROOT, "wayverb_amd", "csrc", "snapshot_plan.h")).read()
    assert sorted(re.findall(r"#include [<\"]([^>\"]+)[>\"]", header)) == ["cstdint", "limits"]


def test_snapshot_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    for name in ("wv_set_snapshots", "wv_snapshot_count", "wv_fetch_snapshots"):
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_snapshots", "snapshot_count", "fetch_snapshots"):
        assert callable(getattr(E.Engine, method))
    assert (E.Engine.QUERY_SNAPSHOT_NS, E.Engine.QUERY_SNAPSHOT_BYTES, E.Engine.QUERY_SNAPSHOTS_TAKEN) == (21, 22, 23)


def test_snapshot_plan_struct_has_the_documented_size_and_offsets():
    """wv_snapshot_plan as a C compiler lays the header's declaration out: 64 bytes, nine int32 from 0, first_step at 40 (8-aligned
    behind them), period at 48, keep at 56, reserved at 60 -- and the ctypes mirror agrees; the query ids are the documented ones."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "keep", "reserved"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_snapshot_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_snapshot_plan, %s));' % f for f in fields) + \
        'printf(" %d %d %d", WV_QUERY_SNAPSHOT_NS, WV_QUERY_SNAPSHOT_BYTES, WV_QUERY_SNAPSHOTS_TAKEN);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [64, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 21, 22, 23]
    assert [ctypes.sizeof(E.WvSnapshotPlan)] + [getattr(E.WvSnapshotPlan, f).offset for f in fields] == got[:14]


def test_capture_kernel_needs_neither_scratch_nor_lds(built_library):
    """The compiler's account of snapshot_gather_kernel (all four instances: float / double fields, one or four nodes per lane), written
    beside the library by wayverb_amd.build."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "snapshot_gather_kernel" in b.split()[0]]
    assert len(blocks) == 4
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 32, b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) == 8, b


def test_python_box_and_stride_to_shape():
    """Engine.set_snapshots turns (origin, extent, stride) into nodes taken per axis: ceil(extent / stride), the first node included."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_snapshots(self, handle, plan):
            self.plan = plan._obj if plan is not None else None
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    assert eng.set_snapshots() == (28, 20, 24)
    assert eng.set_snapshots(box="mesh", stride=3) == (10, 7, 8)
    assert eng.set_snapshots(box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3), first_step=5, period=7, keep=2) == (9, 10, 21)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.keep) == (1, 0, 2, 21, 10, 9, 1, 2, 3, 5, 7, 2)
    assert eng.set_snapshots(box=((0, 0, 5), (None, None, 1))) == (1, 20, 24)
    assert eng.set_snapshots(None) is None and eng.lib.plan is None
    eng.h = None

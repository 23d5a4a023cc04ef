"""Modulation maps, the parts that need no GPU: the planning header (wayverb_amd/csrc/modulation_plan.h) against hand-derived cases,
the new entry points and wv_modulation_plan's layout, the fold kernel's resource usage, where the plan touches the engine's sources,
and the Python layer's box / stride -> shape."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")


def test_modulation_planning_header_against_hand_derived_cases():
    """tests/cpp/modulation_plan_test.cpp: validity limits, byte counts and offsets of E, the sums and the filter states inside the
    plan's two blocks, the overflow answers, the twiddle table's indices and the traffic model's figures.  modulation_plan.h needs
    nothing but the standard library and decay_plan.h."""
    src = os.path.join(ROOT, "tests", "cpp", "modulation_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "modulation_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "MODULATION PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    includes = sorted(re.findall(r"#include [<\"]([^>\"]+)[>\"]", open(os.path.join(CSRC, "modulation_plan.h")).read()))
    assert includes == ["cstdint", "decay_plan.h", "limits"]


def test_modulation_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in ("wv_set_modulation", "wv_modulation_count", "wv_fetch_modulation"):
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_modulation", "modulation_count", "fetch_modulation"):
        assert callable(getattr(E.Engine, method))
    assert (E.Engine.QUERY_MODULATION_CAPTURES, E.Engine.QUERY_MODULATION_FOLDS, E.Engine.QUERY_MODULATION_NS) == (45, 46, 47)


def test_modulation_plan_struct_has_the_documented_size_and_offsets():
    """wv_modulation_plan as a C compiler lays the header's declaration out: 64 bytes, nine int32 from 0, first_step at 40, period at
    48, n_freqs at 56, reserved at 60 -- and the ctypes mirror agrees; the query ids follow the lateral plan's 44."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_freqs", "reserved"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_modulation_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_modulation_plan, %s));' % f for f in fields) + \
        'printf(" %d %d %d", WV_QUERY_MODULATION_CAPTURES, WV_QUERY_MODULATION_FOLDS, WV_QUERY_MODULATION_NS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [64, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 45, 46, 47]
    assert [ctypes.sizeof(E.WvModulationPlan)] + [getattr(E.WvModulationPlan, f).offset for f in fields] == got[:14]


def test_fold_kernel_needs_neither_scratch_nor_lds(built_library):
    """The compiler's account of modulation_fold_kernel's four instances (1 .. 4 sections), written beside the library by
    wayverb_amd.build: no scratch, no spills, no LDS, at most the 128 VGPRs that keep four waves per SIMD -- the bar the other folds
    with 16 staged values per lane are held to.  profiles/r16/modulation_kernel_resources.txt records what the build reported."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "modulation_fold_kernel" in b.split()[0]]
    assert len(blocks) == 4
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 128, b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 4, b


def test_the_plan_touches_no_other_plans_file():
    """DESIGN.md 4.15's list for a sixth plan: its own files, one launch site of its kernel, one case in each of the two switches and
    one refusal row in engine_staged.hip.h; the other plans' files do not name it."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip"))}
    launches = [name for name, t in text.items() if "wv::modulation_fold_kernel<" in t]
    assert launches == ["engine_modulation.hip.h"] and text["engine_modulation.hip.h"].count("hipLaunchKernelGGL((wv::modulation_fold_kernel") == 1
    for name in ("engine_spectrum.hip.h", "engine_decay.hip.h", "engine_intensity.hip.h", "engine_arrival.hip.h", "engine_lateral.hip.h",
                 "engine_snapshot.hip.h", "engine_io.hip.h", "engine_setup.hip.h", "capture_stage.h", "decay_plan.h", "spectrum_plan.h"):
        assert "odulation" not in text[name], name
    own = text["engine_modulation.hip.h"]
    for word in ("spectrum_good_captures", "steps.push_back", "hipEventElapsedTime", "plan_batch_end(", "begin_run(", "std::cos", "std::sin"):
        assert word not in own, word
    for word in ("cos(", "sin(", "sincos", "__shared__", "atomic"):
        assert word not in text["modulation_kernels.hip.h"].split("#pragma once")[1], word
    staged = text["engine_staged.hip.h"]
    assert staged.count("Modulation&>(p)") == 2 and staged.count("kModulationRow") == 1
    assert "a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it); the plans exclude each other" in staged


def test_python_box_and_stride_to_shape():
    """Engine.set_modulation turns (origin, extent, stride) into nodes taken per axis as set_snapshots does, bands and frequencies in
    front, and hands the library the arrays as they lie."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_modulation(self, handle, plan, freqs, sections, n_bands, n_sections):
            self.plan = plan._obj if plan is not None else None
            self.counts = (n_bands, n_sections)
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    bands = np.zeros((3, 4, 5))
    assert eng.set_modulation([0.001] * 14, bands) == (3, 14, 28, 20, 24) and eng.lib.counts == (3, 4)
    assert eng.set_modulation([0.0], bands[:1, :1], box="mesh", stride=3) == (1, 1, 10, 7, 8) and eng.lib.counts == (1, 1)
    assert eng.set_modulation(np.linspace(0, 0.5, 16), bands, box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3), first_step=5, period=7) == (3, 16, 9, 10, 21)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period, p.n_freqs, p.reserved) == (1, 0, 2, 21, 10, 9, 1, 2, 3, 5, 7, 16, 0)
    assert eng.set_modulation([0.1], bands, box=((0, 0, 5), (None, None, 1))) == (3, 1, 1, 20, 24)
    try:
        eng.set_modulation([0.1], np.zeros((3, 5)))
        raise AssertionError("a 2-D bands array was taken")
    except ValueError as err:
        assert "float64[K][S][5]" in str(err)
    assert eng.set_modulation(None, None) is None and eng.lib.plan is None and eng.modulation_shape is None
    eng.h = None

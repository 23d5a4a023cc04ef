"""Waterfall maps, the parts that need no GPU: the planning header (wayverb_amd/csrc/waterfall_plan.h) against hand-derived cases, the
new entry points and wv_waterfall_plan's layout, the fold kernel's resource usage as the build reported it, where the plan touches
the engine's sources, and the Python layer's arguments.  (The kernel's text on the host is tests/test_waterfall_host.py's; what
wv_set_waterfall does with a plan is tests/test_gpu_waterfall.py's.)"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")
NEW = ("wv_set_waterfall", "wv_waterfall_count", "wv_fetch_waterfall")
SENTENCE = "a waterfall plan is active (wv_set_waterfall(e, NULL, NULL) stops it); the plans exclude each other"
OLD_SENTENCES = ("a snapshot plan is active (wv_set_snapshots(e, NULL) stops it)", "a spectrum plan is active (wv_set_spectrum(e, NULL, NULL) stops it)",
                 "a banded decay plan is active (wv_set_decay_bands(e, NULL, NULL, 0, 0) stops it)", "a decay plan is active (wv_set_decay(e, NULL) stops it)",
                 "an intensity plan is active (wv_set_intensity(e, NULL) stops it)", "an arrival plan is active (wv_set_arrival(e, NULL, NULL) stops it)",
                 "a lateral plan is active (wv_set_lateral(e, NULL, NULL) stops it)",
                 "a modulation plan is active (wv_set_modulation(e, NULL, NULL, NULL, 0, 0) stops it)",
                 "a banded arrival plan is active (wv_set_arrival_bands(e, NULL, NULL, NULL, 0, 0) stops it)")


def test_planning_header_against_hand_derived_cases():
    """tests/cpp/waterfall_plan_test.cpp: the cap on K * n_bins at and on either side of 4096; the bin of a capture equal to decay_bin
    throughout; sizes and places of the sums with their overflow answers; the tables; the distinct bins of a fold and the traffic
    model, which at one bin is the spectrum fold's.  The header is host code: no HIP."""
    src = os.path.join(ROOT, "tests", "cpp", "waterfall_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "waterfall_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "WATERFALL PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    header = open(os.path.join(CSRC, "waterfall_plan.h")).read()
    assert "hip" not in header.split("#pragma once")[1].lower()
    assert sorted(re.findall(r"#include [<\"]([^>\"]+)[>\"]", header)) == ["cstdint", "decay_plan.h", "limits", "spectrum_plan.h"]
    assert "return decay_bin(j, bin_captures, n_bins);" in header      # the bin of a capture is decay_plan.h's, not a copy of it


def test_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import engine as E
    from wayverb_amd import simulation as W
    from wayverb_amd import waterfall as WF
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for method in ("set_waterfall", "waterfall_count", "fetch_waterfall"):
        assert callable(getattr(E.Engine, method)) and getattr(E.Engine, method).__doc__
    for fn in ("waterfall_fold", "cumulative_spectral_decay", "short_time_level_db", "csd_level_db", "modal_decay_time", "waterfall_maps"):
        assert callable(getattr(WF, fn))
    assert (E.Engine.QUERY_WATERFALL_CAPTURES, E.Engine.QUERY_WATERFALL_FOLDS, E.Engine.QUERY_WATERFALL_NS) == (51, 52, 53)
    assert E.PLAN_NAMES[-1] == "waterfall" and list(E._PLAN_CALLS)[-1] == "waterfall"
    assert W.PLANS[-1][0] == "waterfall" and list(W.SLABS_REFUSALS)[-1] == "waterfall" and callable(W.waterfall_plan_arguments)


def test_plan_struct_has_the_documented_size_and_offsets():
    """wv_waterfall_plan as a C compiler lays the header's declaration out: the box and the cadence where every plan has them, n_freqs
    at 56 (where the spectrum plan has it), n_bins at 60, bin_captures at 64, reserved at 68 -- 72 bytes, as the header's comment says
    -- and the ctypes mirror agrees; the query ids follow the banded arrival plan's 50."""
    from wayverb_amd import engine as E
    fields = ["x0", "y0", "z0", "nx", "ny", "nz", "sx", "sy", "sz", "first_step", "period", "n_freqs", "n_bins", "bin_captures", "reserved"]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu\", sizeof(wv_waterfall_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_waterfall_plan, %s));' % f for f in fields) + \
        'printf(" %d %d %d", WV_QUERY_WATERFALL_CAPTURES, WV_QUERY_WATERFALL_FOLDS, WV_QUERY_WATERFALL_NS);return 0;}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60, 64, 68]
    assert got == [72] + offsets + [51, 52, 53]
    assert [ctypes.sizeof(E.WvWaterfallPlan)] + [getattr(E.WvWaterfallPlan, f).offset for f in fields] == [72] + offsets
    assert E.WvWaterfallPlan.n_freqs.offset == E.WvSpectrumPlan.n_freqs.offset
    comment = open(os.path.join(ROOT, "include", "wayverb_amd.h")).read()
    assert "The struct is 72 bytes" in comment and "bin_captures at 64, reserved at 68" in comment


def test_the_fold_kernel_needs_neither_scratch_nor_lds(built_library):
    """The compiler's account of waterfall_fold_kernel's two instances (one and two nodes per lane), written beside the library by
    wayverb_amd.build: no scratch, no VGPR or SGPR spill, no LDS, at most the 128 VGPRs that keep four waves per SIMD -- what the
    spectrum fold, whose registers it has, is reported with.  profiles/r22/waterfall_kernel_resources.txt records what a build for
    gfx950 reported."""
    from wayverb_amd import build as B
    all_blocks = re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:]
    blocks = [b for b in all_blocks if "waterfall_fold_kernel" in b.split()[0]]
    assert len(blocks) == 2
    for b in blocks:
        for what in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill", r"LDS Size \[bytes/block\]"):
            assert int(re.search(what + r": (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 128, b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 4, b
    recorded = open(os.path.join(ROOT, "profiles", "r22", "waterfall_kernel_resources.txt")).read()
    assert recorded.count("Function Name:") == 2 and recorded.count("ScratchSize [bytes/lane]: 0") == 2
    assert recorded.count("VGPRs Spill: 0") == 2 and recorded.count("SGPRs Spill: 0") == 2 and recorded.count("LDS Size [bytes/block]: 0") == 2


def test_the_plan_touches_no_other_plans_file():
    """DESIGN.md 4.15's list for an eighth staged plan: its own three files, one launch site of its kernel, one case in each of the two
    switches and one refusal row in engine_staged.hip.h; the other plans' files do not name it; its sentence stands once in all of
    the sources, and each of the nine existing sentences still stands once."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip", ".cpp"))}
    assert [name for name, t in text.items() if "waterfall_fold_kernel<" in t] == ["engine_waterfall.hip.h", "waterfall_kernels.hip.h"]
    assert text["engine_waterfall.hip.h"].count("hipLaunchKernelGGL(") == 1
    others = [name for name in text if name.startswith(("engine_", "capture_stage")) or name.endswith(("_plan.h", "_kernels.hip.h")) or name == "fold_parts.hip.h"]
    shared = ("engine_staged.hip.h", "engine_batch.hip.h", "engine_slab.hip.h", "engine_base.h", "engine_waterfall.hip.h", "waterfall_plan.h", "waterfall_kernels.hip.h")
    assert len(others) > 40
    for name in others:
        if name not in shared:
            assert "waterfall" not in text[name].lower(), name
    own = text["engine_waterfall.hip.h"]
    for word in ("spectrum_good_captures", "steps.push_back", "hipEventElapsedTime", "plan_batch_end(", "begin_run(", "plan is active (", "std::cos", "std::sin"):
        assert word not in own, word
    assert own.count("plan_refused(") == 1 and own.count("bin_table_write(") == 1 and own.count("twiddle_table_write(") == 1
    kernel = text["waterfall_kernels.hip.h"].split("#pragma once")[1].split("namespace wv {")[1]
    for word in ("__shared__", "atomic", " / ", " % ", "cos(", "sin("):
        assert word not in kernel, word
    assert kernel.count("* __restrict__ ") == 4      # stage, sums and both tables: separate arguments
    staged = text["engine_staged.hip.h"]
    assert staged.count("Waterfall&>(p)") == 2 and staged.count("kWaterfallRow") == 1 and "kWaterfallStage == kSpectrumStage" in staged
    assert sum(t.count(SENTENCE) for t in text.values()) == 1 and SENTENCE in staged
    for old in OLD_SENTENCES:
        assert old not in SENTENCE
        assert sum(t.count(old + "; the plans exclude each other") for t in text.values()) == 1, old


def test_python_arguments_to_plan():
    """Engine.set_waterfall turns (origin, extent, stride) into nodes taken per axis as set_snapshots does, the frequencies into
    float64[K] and n_freqs, the bins into their two words; None stops; a fetch without a plan asks the library with an empty array."""
    from wayverb_amd import engine as E

    class Lib:
        def wv_set_waterfall(self, handle, plan, freqs):
            self.plan = plan._obj if plan is not None else None
            self.freqs = None if freqs is None else np.ctypeslib.as_array(ctypes.cast(freqs, ctypes.POINTER(ctypes.c_double)), (self.plan.n_freqs,)).copy()
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    eng._plan_state()
    assert eng.waterfall_shape is None and "waterfall_shape" not in vars(eng)
    assert eng.set_waterfall([0.0, 0.25, 0.5], 7, 3) == (7, 3, 28, 20, 24) == eng.waterfall_shape
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period) == (0, 0, 0, 24, 20, 28, 1, 1, 1, 0, 1)
    assert (p.n_freqs, p.n_bins, p.bin_captures, p.reserved) == (3, 7, 3, 0) and list(eng.lib.freqs) == [0.0, 0.25, 0.5]
    assert eng.set_waterfall(0.125, 2, 5, box=((1, 2, 3), (10, 9, 7)), stride=(1, 2, 3), first_step=4, period=6) == (2, 1, 3, 5, 10)
    p = eng.lib.plan
    assert (p.x0, p.y0, p.z0, p.nx, p.ny, p.nz, p.sx, p.sy, p.sz, p.first_step, p.period) == (1, 2, 3, 10, 5, 3, 1, 2, 3, 4, 6)
    assert (p.n_freqs, p.n_bins, p.bin_captures) == (1, 2, 5)
    assert eng.set_waterfall(None, None, None) is None and eng.lib.plan is None and eng.waterfall_shape is None
    with pytest.raises(TypeError):
        eng.set_waterfall([0.1])      # n_bins and bin_captures have no defaults

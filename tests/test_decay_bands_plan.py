"""Band-limited decay maps, the parts of the plan that need no GPU: the new entry points and wv_biquad's layout, the fold kernel's
resource usage as the build reported it, and the Python layer's bands -> shape.  (An engine needs a device: what wv_set_decay_bands
refuses is tests/test_gpu_decay_bands.py's.)"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("wv_set_decay_bands", "wv_fetch_decay_bands", "wv_biquad_run", "wv_butterworth_bandpass", "wv_bandpass_biquad")


def test_band_entry_points_are_exported_and_bound(built_library):
    lib = ctypes.CDLL(built_library)
    from wayverb_amd import decay as D
    from wayverb_amd import engine as E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wayverb_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), "include/wayverb_amd.h does not declare %s" % name
        assert hasattr(lib, name), "libwayverb_amd.so does not export %s" % name
        assert name in E.EXPORTS
    for fn in ("octave_band_edges", "butterworth_bandpass", "bandpass_biquad", "biquad_cascade", "banded_bins", "band_decay_maps"):
        assert callable(getattr(D, fn))


def test_biquad_struct_is_five_doubles_and_the_plan_is_unchanged():
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"wayverb_amd.h\"\nint main(void){printf(\"%zu %zu\", sizeof(wv_biquad), sizeof(wv_decay_plan));" + \
        "".join('printf(" %%zu", offsetof(wv_biquad, %s));' % f for f in ("b0", "b1", "b2", "a1", "a2")) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [40, 64, 0, 8, 16, 24, 32]


def test_banded_fold_kernel_needs_no_scratch_and_spills_nothing(built_library):
    """One instance per section count 1 .. 4 (the kernel does not depend on the field's precision): ScratchSize 0, no VGPR and no SGPR
    spill, no LDS -- the state and the coefficients stay in registers.  profiles/r11/decay_bands_kernel_resources.txt records what the
    build reported."""
    from wayverb_amd import build as B
    blocks = [b for b in re.split(r"remark: Function Name: ", open(B.RESOURCES).read())[1:] if "decay_bands_fold_kernel" in b.split()[0]]
    assert len(blocks) == 4
    for b in blocks:
        for what in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill", r"LDS Size \[bytes/block\]"):
            assert int(re.search(what + r": (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 128, b
    recorded = open(os.path.join(ROOT, "profiles", "r11", "decay_bands_kernel_resources.txt")).read()
    assert recorded.count("Function Name:") == 4 and recorded.count("ScratchSize [bytes/lane]: 0") == 4
    assert recorded.count("VGPRs Spill: 0") == 4 and recorded.count("SGPRs Spill: 0") == 4


def test_python_bands_to_shape_and_the_call_that_is_made():
    """Engine.set_decay(bands=float64[K][S][5]) goes to wv_set_decay_bands with K and S from the array's shape and returns
    (K, n_bins, nz, ny, nx); bands=None goes to wv_set_decay as before; fetch_decay follows the kind of plan."""
    from wayverb_amd import engine as E

    class Lib:
        calls = []

        def wv_set_decay(self, handle, plan):
            self.calls.append(("plain", None if plan is None else plan._obj.n_bins))
            return 0

        def wv_set_decay_bands(self, handle, plan, sections, n_bands, n_sections):
            got = np.ctypeslib.as_array(ctypes.cast(sections, ctypes.POINTER(ctypes.c_double)), (n_bands * n_sections * 5,)).copy()
            self.calls.append(("bands", plan._obj.n_bins, plan._obj.bin_captures, plan._obj.period, n_bands, n_sections, got))
            return 0

        def wv_fetch_decay(self, handle, dst, captures):
            self.calls.append(("fetch plain",))
            return 0

        def wv_fetch_decay_bands(self, handle, dst, captures):
            self.calls.append(("fetch bands",))
            return 0

    class Mesh:
        dims = (24, 20, 28)

    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = Lib(), None, Mesh()
    bands = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)[:, ::-1]     # not float64, not contiguous
    assert eng.set_decay(7, 5, box=((1, 0, 2), (21, 20, 25)), stride=(1, 2, 3), period=3, bands=bands) == (2, 7, 9, 10, 21)
    call = eng.lib.calls[-1]
    assert call[:6] == ("bands", 7, 5, 3, 2, 3) and call[6].tobytes() == np.ascontiguousarray(bands, dtype=np.float64).tobytes()
    assert eng.fetch_decay()[0].shape == (2, 7, 9, 10, 21) and eng.lib.calls[-1] == ("fetch bands",)
    assert eng.set_decay(4, 2) == (4, 28, 20, 24) and eng.lib.calls[-1] == ("plain", 4)
    assert eng.fetch_decay()[0].shape == (4, 28, 20, 24) and eng.lib.calls[-1] == ("fetch plain",)
    eng.fetch_decay(banded=True)
    assert eng.lib.calls[-1] == ("fetch bands",)
    assert eng.set_decay(3, 1, bands=np.zeros((0, 4, 5))) == (0, 3, 28, 20, 24) and eng.lib.calls[-1][4:6] == (0, 4)   # (the library's to refuse)
    for bad in (np.zeros((2, 5)), np.zeros((1, 4, 6)), np.zeros(5)):
        with pytest.raises(ValueError):
            eng.set_decay(3, 1, bands=bad)
    assert eng.set_decay(None) is None and eng.lib.calls[-1] == ("plain", None) and eng.decay_shape is None
    eng.h = None


def test_cpp_header_designs_the_sections_of_octave_bands(built_library):
    """include/wayverb_amd/setup.h, octave_band_decay_sections: plain C++14 over the C ABI; per band the four sections of
    wv_butterworth_bandpass at sample_rate / period, and std::invalid_argument for a band the captured series cannot carry."""
    from wayverb_amd import decay as D
    prog = r'''
#include <cstdio>
#include "wayverb_amd/setup.h"
int main() {
    const auto s = wayverb::waveguide::octave_band_decay_sections({125.0, 250.0, 500.0}, 12000.0, 3);
    std::printf("%zu\n", s.size());
    for (const auto& c : s) std::printf("%a %a %a %a %a\n", c.b0, c.b1, c.b2, c.a1, c.a2);
    try {
        wayverb::waveguide::octave_band_decay_sections({1500.0}, 12000.0, 3);
        std::printf("not refused\n");
    } catch (const std::invalid_argument& e) {
        std::printf("refused: %s\n", e.what());
    }
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "sections.cpp"), os.path.join(tmp, "sections")
        open(src, "w").write(prog)
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                               "-L", os.path.join(ROOT, "wayverb_amd"), "-lwayverb_amd", "-Wl,-rpath," + os.path.join(ROOT, "wayverb_amd")])
        lines = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout.splitlines()
    assert lines[0] == "12" and lines[13].startswith("refused: wv_butterworth_bandpass")
    got = np.array([[float.fromhex(v) for v in line.split()] for line in lines[1:13]]).reshape(3, 4, 5)
    want = np.stack([D.butterworth_bandpass(lo, hi, 12000.0 / 3) for lo, hi in D.octave_band_edges([125.0, 250.0, 500.0])])
    assert got.tobytes() == want.tobytes()

"""Waterfall maps, host side (no GPU): the text of waterfall_fold_kernel compiled for the host against the NumPy definition
waterfall.waterfall_fold, byte for byte (tests/cpp/waterfall_kernel_host.cpp), both lane widths, and once more under the address and
undefined-behaviour sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

from wayverb_amd import engine as E
from wayverb_amd import waterfall as WF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", os.path.join(ROOT, "wayverb_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "waterfall_kernel_host.cpp")]


def series(rng, t, nodes):
    """float32 captures over 47 orders of magnitude, subnormal floats among them."""
    return (rng.standard_normal((t, nodes)) * 10.0 ** rng.integers(-44, 3, (t, nodes))).astype(np.float32)


def freqs_of(rng, k):
    f = rng.uniform(0.0, 0.5, k)
    f[0] = 0.0 if k != 4 else 0.5          # both ends of the range are taken
    if k >= 5:
        f[-1] = 0.5
    return f


def run_host(exe, tmp_path, snaps, steps, freqs, n_bins, bin_captures, first_fold=16, first_capture=0, wide=False):
    t, nodes = snaps.shape
    k = len(freqs)
    tw = np.array([[E.spectrum_twiddle(f, int(n)) for f in freqs] for n in steps], dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8Q", nodes, k, n_bins, bin_captures, t, first_fold, first_capture, int(wide)) + tw.tobytes() + snaps.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=300)
    raw = np.fromfile(fout)
    assert raw.size == n_bins * k * 2 * nodes
    block = raw.reshape(n_bins, k, 2, nodes)
    sums = np.empty((n_bins, k, nodes), np.complex128)
    sums.real, sums.imag = block[:, :, 0], block[:, :, 1]
    return sums


# (B, K, captures, n_bins, bin_captures, first fold, first capture).  B of 1 / 2 / 255 / 256 / 257 / 630; K on either side of the kernel's
# chunk of 4; t of 1 / 15 / 16.  Where the bin edges fall among the staged captures: 16 captures from capture 0 in bins of 16 -- the whole
# fold inside one bin; from capture 3 in bins of 3 -- an edge AT the first capture; bins of 8 -- one in the middle; 16 captures from
# capture 1 in bins of 16 -- an edge at the last; bins of 1 -- at every capture; 33 captures after a first fold of 15 -- two and three
# folds in sequence; more bins than captures; and the open-ended last bin
KERNEL_SHAPES = [(1, 1, 1, 1, 1, 16, 0), (2, 3, 15, 4, 16, 16, 0), (255, 4, 16, 2, 16, 16, 0), (256, 5, 16, 7, 3, 16, 3), (257, 9, 16, 3, 8, 16, 0),
                 (630, 5, 16, 2, 16, 16, 1), (630, 3, 16, 16, 1, 16, 0), (257, 4, 33, 5, 4, 15, 0), (256, 9, 33, 2, 5, 16, 7), (2, 1, 17, 64, 1, 1, 0),
                 (255, 3, 31, 3, 5, 15, 0)]


@pytest.fixture(scope="module")
def host_exe():
    exe = os.path.join(ROOT, "tests", "cpp", "waterfall_kernel_host")
    subprocess.check_call(COMPILE + ["-O2", "-o", exe])
    return exe


def test_the_kernels_text_on_the_host_reproduces_the_definition_bytewise(host_exe, tmp_path):
    """Every sum bytewise, the sums allocated at exactly the plan's byte count, steps 3, 10, 17, ... (period 7); an even B in both lane
    widths, an odd one in the narrow one (the engine's choice)."""
    rng = np.random.default_rng(22)
    seen = set()
    for nodes, k, t, n_bins, w, first_fold, first in KERNEL_SHAPES:
        freqs, snaps = freqs_of(rng, k), series(rng, t, nodes)
        steps = 3 + 7 * (first + np.arange(t))
        want = WF.waterfall_fold(snaps, steps, freqs, n_bins, w, first_capture=first)
        case = (nodes, k, t, n_bins, w, first_fold, first)
        assert np.abs(want).reshape(n_bins, -1).max(axis=1).astype(bool).sum() == len({min((first + j) // w, n_bins - 1) for j in range(t)}), case
        for wide in ((False, True) if nodes % 2 == 0 else (False,)):
            got = run_host(host_exe, tmp_path, snaps, steps, freqs, n_bins, w, first_fold, first, wide)
            assert got.tobytes() == want.tobytes(), (case, wide)
            seen.add(wide)
    assert seen == {False, True}


def test_bins_no_capture_reached_stay_plus_zero(host_exe, tmp_path):
    rng = np.random.default_rng(23)
    snaps = series(rng, 5, 256)
    for wide in (False, True):
        got = run_host(host_exe, tmp_path, snaps, np.arange(5), [0.0, 0.3], 9, 2, wide=wide)
        raw = np.stack([got.real, got.imag])
        assert not raw[:, 3:].any() and not np.signbit(raw[:, 3:]).any() and np.abs(got[:3]).reshape(3, -1).max(axis=1).all()


def test_a_nan_capture_poisons_its_node_and_bin_and_no_other(host_exe, tmp_path):
    rng = np.random.default_rng(24)
    nodes, t = 257, 20
    freqs, snaps = freqs_of(rng, 5), series(rng, t, nodes)
    clean = snaps.copy()
    snaps[6, 100] = np.nan
    got = run_host(host_exe, tmp_path, snaps, np.arange(t), freqs, 4, 5)
    want = WF.waterfall_fold(clean, np.arange(t), freqs, 4, 5)
    assert np.isnan(got[1, :, 100].real).all() and np.isnan(got[1, :, 100].imag).all()
    poisoned = np.zeros(got.shape, bool)
    poisoned[1, :, 100] = True
    assert not np.isnan(got[~poisoned]).any() and got[~poisoned].tobytes() == want[~poisoned].tobytes()


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (-fno-sanitize-recover: a report is a failure) on B = 257
    and, for the wide form, B = 256: the sums, every fold's stage and both of its tables are allocated at exactly their sizes."""
    exe = os.path.join(ROOT, "tests", "cpp", "waterfall_kernel_host_san")
    subprocess.check_call(COMPILE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    rng = np.random.default_rng(25)
    for nodes, k, t, n_bins, w, first_fold, first, wide in ((257, 9, 33, 5, 4, 13, 0, False), (257, 1, 1, 1, 1, 16, 0, False), (256, 5, 17, 7, 3, 16, 3, True)):
        freqs, snaps = freqs_of(rng, k), series(rng, t, nodes)
        steps = 5 + 3 * (first + np.arange(t))
        got = run_host(exe, tmp_path, snaps, steps, freqs, n_bins, w, first_fold, first, wide)
        assert got.tobytes() == WF.waterfall_fold(snaps, steps, freqs, n_bins, w, first_capture=first).tobytes()

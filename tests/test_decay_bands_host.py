"""Band-limited decay maps, host side (no GPU): the biquad cascade and the two band-pass designs (wayverb_amd/csrc/biquad.cpp through
wayverb_amd.decay) against values recorded from the reference's own functions, tests/golden/biquad_reference.npz (its .md says how
the file was made); the NumPy definition decay.biquad_cascade / banded_bins against the same; and tests/cpp/decay_bands_test.cpp."""
import os
import subprocess

import numpy as np
import pytest

from wayverb_amd import decay as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(ROOT, "tests", "golden", "biquad_reference.npz")) as f:
        out = {k: f[k] for k in f.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def signals(ref):
    names = sorted(k for k in ref if k.startswith("signal_"))
    assert len(names) == 4
    return [(int(n.split("_")[1]), ref[n]) for n in names]


def test_the_fixture_is_what_its_description_says(ref):
    t = ref["triples"]
    assert t.shape == (13, 3) and ref["butterworth"].shape == (13, 4, 5) and ref["bandpass"].shape == (13, 5)
    assert (t[:, 1] == t[:, 2] / 4).any()                                   # a band whose edge sits at sample_rate / 4
    assert t[:, 2].min() == 1333.0 and t[:, 2].max() == 12000.0
    assert list(ref["output_triples"]) == [0, 1]
    sig = dict(signals(ref))
    assert sig[1][0] == 1.0 and not sig[1][1:].any()                        # the impulse
    assert np.abs(sig[2]).max() < 1e-305                                    # scaled so that states and outputs go subnormal
    y = ref["series4_2"]
    assert ((y != 0) & (np.abs(y) < np.finfo(np.float64).tiny)).mean() > 0.5
    assert not sig[3][-300:].any() and sig[3][:-300].all()                  # ends in 300 zeros
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "biquad_reference.npz")) < 100 * 1024


def test_wv_biquad_run_equals_the_reference_bytewise(ref, built_library):
    """series_biquads<4> and a single biquad, run_one_pass, on the four signals: only + - x, so every bit."""
    for k in ref["output_triples"]:
        for i, x in signals(ref):
            got4 = D.biquad_run(ref["butterworth"][k], x)
            got1 = D.biquad_run(ref["bandpass"][k][None, :], x)
            assert got4.tobytes() == ref["series4_%d" % i][k].tobytes(), (k, i, np.abs(got4 - ref["series4_%d" % i][k]).max())
            assert got1.tobytes() == ref["single_%d" % i][k].tobytes(), (k, i)
            assert np.abs(got4).max() > 0 and np.abs(got1).max() > 0


def test_the_numpy_definition_equals_the_reference_bytewise(ref):
    """decay.biquad_cascade on each signal, and once more with the four signals (cut to the shortest) as columns, which covers the
    node axis."""
    for k in ref["output_triples"]:
        for i, x in signals(ref):
            y4, z4 = D.biquad_cascade(ref["butterworth"][k], x)
            y1, z1 = D.biquad_cascade(ref["bandpass"][k], x)
            assert y4.tobytes() == ref["series4_%d" % i][k].tobytes() and y1.tobytes() == ref["single_%d" % i][k].tobytes()
            assert z4.shape == (4, 2) and z1.shape == (1, 2)
    # a node axis: the four signals cut to the shortest, as columns
    n = min(len(x) for _, x in signals(ref))
    cols = np.stack([x[:n] for _, x in signals(ref)], axis=1)
    y, z = D.biquad_cascade(ref["butterworth"][0], cols)
    for c, (i, _) in enumerate(signals(ref)):
        assert y[:, c].tobytes() == ref["series4_%d" % i][0][:n].tobytes()
    assert z.shape == (4, 2, 4)


def test_two_halves_with_the_state_carried_equal_one_call(ref, built_library):
    sections = ref["butterworth"][1]
    for i, x in signals(ref):
        whole_state = np.zeros((4, 2))
        whole = D.biquad_run(sections, x, whole_state)
        for cut in (1, len(x) // 2, len(x) - 1):
            state = np.zeros((4, 2))
            halves = np.concatenate([D.biquad_run(sections, x[:cut], state), D.biquad_run(sections, x[cut:], state)])
            assert halves.tobytes() == whole.tobytes() == ref["series4_%d" % i][1].tobytes()
            assert state.tobytes() == whole_state.tobytes()
        # ... and the NumPy definition carries the same state
        y, z = D.biquad_cascade(sections, x[:7])
        y2, z2 = D.biquad_cascade(sections, x[7:], state=z)
        assert np.concatenate([y, y2]).tobytes() == whole.tobytes() and z2.tobytes() == whole_state.tobytes()


def test_design_functions_against_the_fixture(ref, built_library):
    """Bitwise equality is what the same libm and the same expression order give; the limit is an absolute 2e-14 per coefficient:
    |coefficient| <= 2, intermediates <= 4, one libm call within 1 ulp and at most 8 rounded operations behind it, so about
    16 * 2^-52 * 4.  (Observed maximum where the fixture was made: 0, tests/golden/biquad_reference.md.)"""
    worst = 0.0
    for (lo, hi, sr), bw, bp in zip(ref["triples"], ref["butterworth"], ref["bandpass"]):
        got_bw, got_bp = D.butterworth_bandpass(lo, hi, sr), D.bandpass_biquad(lo, hi, sr)
        assert got_bw.shape == (4, 5) and got_bp.shape == (1, 5)
        worst = max(worst, np.abs(got_bw - bw).max(), np.abs(got_bp[0] - bp).max())
    print("largest coefficient difference from the reference: %g" % worst)
    assert worst <= 2e-14
    assert np.abs(ref["butterworth"]).max() <= 2 and np.abs(ref["butterworth"]).max() > 1


def test_design_functions_refuse_what_is_no_band(built_library):
    from wayverb_amd import engine as E
    for lo, hi, sr in ((100, 100, 4000), (200, 100, 4000), (0, 100, 4000), (100, 2000, 4000), (100, 200, 0), (np.nan, 200, 4000)):
        with pytest.raises(E.WaveguideError, match="error -1: .*lo_hz < hi_hz < sample_rate / 2"):
            D.butterworth_bandpass(lo, hi, sr)
        with pytest.raises(E.WaveguideError, match="error -1: .*lo_hz < hi_hz < sample_rate / 2"):
            D.bandpass_biquad(lo, hi, sr)


def test_octave_band_edges():
    edges = D.octave_band_edges([125, 250, 500])
    assert [e[1] / e[0] for e in edges] == pytest.approx([2.0] * 3, rel=1e-15)
    assert [np.sqrt(e[0] * e[1]) for e in edges] == pytest.approx([125, 250, 500], rel=1e-15)
    assert edges[0][1] == pytest.approx(edges[1][0], rel=1e-15)
    assert D.octave_band_edges(63.0) == [(63.0 / np.sqrt(2.0), 63.0 * np.sqrt(2.0))]


def plain_bins(snaps, n_bins, bin_captures):
    out = np.zeros((n_bins,) + snaps.shape[1:])
    for j, p in enumerate(snaps):
        p = p.astype(np.float64)
        b = min(j // bin_captures, n_bins - 1)
        out[b] = out[b] + p * p
    return out


def test_banded_bins_with_the_identity_section_are_the_plain_bins(ref):
    rng = np.random.default_rng(5)
    snaps = (rng.standard_normal((37, 3, 5)) * 10.0 ** rng.integers(-30, 3, (37, 3, 5))).astype(np.float32)
    identity = np.array([[[1.0, 0, 0, 0, 0]]])
    for n_bins, w in ((37, 1), (7, 5), (2, 40), (1, 1), (4, 3)):
        got = D.banded_bins(snaps, identity, n_bins, w)
        assert got.shape == (1, n_bins, 3, 5) and got[0].tobytes() == plain_bins(snaps, n_bins, w).tobytes() and got.max() > 0
    # bands are independent and ordered; the state comes back per band
    sections = np.stack([ref["butterworth"][0], ref["butterworth"][1]])
    both, state = D.banded_bins(snaps, sections, 7, 5, return_state=True)
    for k in range(2):
        assert both[k].tobytes() == D.banded_bins(snaps, sections[k][None], 7, 5)[0].tobytes()
        y, z = D.biquad_cascade(sections[k], snaps.astype(np.float64))
        assert state[k].tobytes() == z.tobytes() and both[k].sum() == pytest.approx((y * y).sum(), rel=1e-12)
    assert both[0].tobytes() != both[1].tobytes()


def test_band_decay_maps_is_decay_maps_per_band():
    rng = np.random.default_rng(9)
    t = np.arange(40)[:, None, None]
    bins = np.stack([10.0 ** (-t / 8.0) * rng.uniform(0.5, 1.5, (40, 2, 3)), 10.0 ** (-t / 3.0) * rng.uniform(0.5, 1.5, (40, 2, 3))])
    maps = D.band_decay_maps(bins, 4, 1, 2000.0)
    for k in range(2):
        one = D.decay_maps(bins[k], 4, 1, 2000.0)
        assert sorted(one) == sorted(maps)
        for name in one:
            assert maps[name][k].tobytes() == one[name].tobytes()
    assert maps["t20_s"].shape == (2, 2, 3) and maps["edc_db"].shape == (2, 40, 2, 3)
    assert (maps["t20_s"][0] > 2 * maps["t20_s"][1]).all()


def test_host_functions_stand_alone_program(tmp_path):
    """tests/cpp/decay_bands_test.cpp: wv_biquad_run, the designs and decay_plan.h's sizes for a banded plan against hand-derived
    cases, its own main, nothing but the standard library and the two host files."""
    exe = os.path.join(ROOT, "tests", "cpp", "decay_bands_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "wayverb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "decay_bands_test.cpp"),
                           os.path.join(ROOT, "wayverb_amd", "csrc", "biquad.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DECAY BANDS OK" in p.stdout, p.stdout[-4000:] + p.stderr


KERNEL_SHAPES = [(567, 7, 3, 4, 21, 3, 16), (630, 33, 8, 4, 33, 1, 16), (1, 2, 2, 3, 33, 40, 16), (300, 1, 1, 1, 17, 1, 16), (257, 4, 2, 2, 30, 3, 13)]


def test_the_kernels_text_on_the_host_reproduces_the_definition_bytewise(tmp_path):
    """tests/cpp/decay_bands_kernel_host.cpp: decay_bands_fold_kernel's text compiled for the host (one call per lane, fold after fold
    of 16 captures at the most) against decay.banded_bins: bins AND states bytewise for B = 567 / 630 / 1 / 300 / 257, 1 .. 4 sections,
    1 .. 8 bands, W = 1 / 3 / 40, a short first fold; snapshots span 1e-44 .. 1e3 (subnormal floats among them)."""
    import struct
    exe = os.path.join(ROOT, "tests", "cpp", "decay_bands_kernel_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"),
                           "-I", os.path.join(ROOT, "wayverb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "decay_bands_kernel_host.cpp"), "-o", exe])
    rng = np.random.default_rng(3)
    for nodes, n_bins, k, s, t, w, first_fold in KERNEL_SHAPES:
        edges = D.octave_band_edges([0.2 / 2 ** i for i in range(k)])
        sections = np.stack([D.bandpass_biquad(lo, hi, 1.0) for lo, hi in edges]) if s == 1 else \
            np.stack([D.butterworth_bandpass(lo, hi, 1.0)[4 - s:] for lo, hi in edges])
        snaps = (rng.standard_normal((t, nodes)) * 10.0 ** rng.integers(-44, 3, (t, nodes))).astype(np.float32)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<7Q", nodes, n_bins, k, s, t, w, first_fold) + sections.tobytes() + snaps.tobytes())
        subprocess.run([exe, fin, fout], check=True, timeout=300)
        raw = np.fromfile(fout)
        bins, state = raw[:k * n_bins * nodes].reshape(k, n_bins, nodes), raw[k * n_bins * nodes:].reshape(k, s, 2, nodes)
        want, want_state = D.banded_bins(snaps, sections, n_bins, w, return_state=True)
        assert bins.tobytes() == want.tobytes() and state.tobytes() == want_state.tobytes(), (nodes, n_bins, k, s, t, w)
        assert (want.reshape(k, -1).max(axis=1) > 0).all()

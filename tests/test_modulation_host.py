"""Modulation maps, host side (no GPU): the text of modulation_fold_kernel compiled for the host against the NumPy definition
modulation.modulation_fold, byte for byte (tests/cpp/modulation_kernel_host.cpp), once more under the address and undefined-behaviour
sanitizers; identities of the definition; the closed forms of an exponential decay; and the arithmetic of the speech transmission
index."""
import os
import struct
import subprocess

import numpy as np
import pytest

from wayverb_amd import decay as D
from wayverb_amd import engine as E
from wayverb_amd import modulation as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", os.path.join(ROOT, "wayverb_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "modulation_kernel_host.cpp")]
IDENTITY = np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]]])


def band_sections(k, s):
    """k octave bands below 0.2 cycles per capture, s sections each: one constant-skirt section, or the last s of the Butterworth four."""
    edges = D.octave_band_edges([0.2 / 2 ** i for i in range(k)])
    if s == 1:
        return np.stack([D.bandpass_biquad(lo, hi, 1.0) for lo, hi in edges])
    return np.stack([D.butterworth_bandpass(lo, hi, 1.0)[4 - s:] for lo, hi in edges])


def series(rng, t, nodes):
    """float32 captures over 47 orders of magnitude, subnormal floats among them."""
    snaps = (rng.standard_normal((t, nodes)) * 10.0 ** rng.integers(-44, 3, (t, nodes))).astype(np.float32)
    assert ((snaps != 0) & (np.abs(snaps) < np.finfo(np.float32).tiny)).any() or nodes * t < 50
    return snaps


def freqs_of(rng, m):
    f = rng.uniform(0.0, 0.5, m)
    f[0] = 0.0 if m != 4 else 0.5          # both ends of the range are taken
    if m >= 5:
        f[-1] = 0.5
    return f


def run_host(exe, tmp_path, snaps, steps, freqs, sections, first_fold):
    t, nodes = snaps.shape
    k, s, m = sections.shape[0], sections.shape[1], len(freqs)
    tw = np.array([[E.spectrum_twiddle(f, int(n)) for f in freqs] for n in steps], dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6Q", nodes, k, s, m, t, first_fold) + np.ascontiguousarray(sections, np.float64).tobytes() + tw.tobytes() + snaps.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=300)
    raw = np.fromfile(fout)
    n_sums = k * (1 + 2 * m) * nodes
    assert raw.size == n_sums + k * s * 2 * nodes
    block = raw[:n_sums].reshape(k, 1 + 2 * m, nodes)
    sums = np.empty((k, m, nodes), np.complex128)
    sums.real, sums.imag = block[:, 1::2], block[:, 2::2]
    return block[:, 0].copy(), sums, raw[n_sums:].reshape(k, s, 2, nodes)


# (B, n_bands, S, M, captures, first fold): B of 1 / 255 / 256 / 257 / 630, S of 1 .. 4, 1 / 3 / 8 bands, M on either side of the
# kernel's chunk of 4 and at both limits, 1 / 16 / 17 / 33 captures, short first folds
KERNEL_SHAPES = [(1, 1, 1, 1, 1, 16), (255, 3, 2, 4, 16, 16), (256, 8, 4, 5, 17, 16), (257, 3, 3, 14, 33, 13), (630, 8, 4, 16, 33, 16),
                 (630, 1, 1, 14, 17, 5), (300, 3, 4, 1, 33, 1)]


@pytest.fixture(scope="module")
def host_exe():
    exe = os.path.join(ROOT, "tests", "cpp", "modulation_kernel_host")
    subprocess.check_call(COMPILE + ["-O2", "-o", exe])
    return exe


def test_the_kernels_text_on_the_host_reproduces_the_definition_bytewise(host_exe, tmp_path):
    """E, Re, Im AND filter states bytewise, the blocks allocated at exactly the plan's byte counts, steps 3, 10, 17, ... (period 7)."""
    rng = np.random.default_rng(16)
    for nodes, k, s, m, t, first_fold in KERNEL_SHAPES:
        sections, freqs, snaps = band_sections(k, s), freqs_of(rng, m), series(rng, t, nodes)
        steps = 3 + 7 * np.arange(t)
        energy, sums, state = run_host(host_exe, tmp_path, snaps, steps, freqs, sections, first_fold)
        want_e, want_s, want_z = M.modulation_fold(snaps, steps, freqs, sections, return_state=True)
        case = (nodes, k, s, m, t, first_fold)
        assert energy.tobytes() == want_e.tobytes(), case
        assert sums.tobytes() == want_s.tobytes(), case
        assert state.tobytes() == want_z.tobytes(), case
        assert (want_e.reshape(k, -1).max(axis=1) > 0).all() and (np.abs(want_s).reshape(k, m, -1).max(axis=2) > 0).all(), case


def test_a_nan_capture_poisons_its_node_and_no_other(host_exe, tmp_path):
    rng = np.random.default_rng(17)
    nodes, k, s, m, t = 257, 3, 2, 5, 20
    sections, freqs, snaps = band_sections(k, s), freqs_of(rng, m), series(rng, t, nodes)
    clean = snaps.copy()
    snaps[6, 100] = np.nan
    energy, sums, state = run_host(host_exe, tmp_path, snaps, np.arange(t), freqs, sections, 16)
    assert np.isnan(energy[:, 100]).all() and np.isnan(sums[:, :, 100].real).all() and np.isnan(sums[:, :, 100].imag).all() and np.isnan(state[:, :, :, 100]).all()
    others = np.arange(nodes) != 100
    want_e, want_s, want_z = M.modulation_fold(clean, np.arange(t), freqs, sections, return_state=True)
    assert not np.isnan(energy[:, others]).any() and not np.isnan(sums[:, :, others]).any()
    assert energy[:, others].tobytes() == want_e[:, others].tobytes() and sums[:, :, others].tobytes() == want_s[:, :, others].tobytes()
    assert state[..., others].tobytes() == want_z[..., others].tobytes()
    # the definition says the same of the poisoned series
    got_e, got_s = M.modulation_fold(snaps, np.arange(t), freqs, sections)
    assert np.isnan(got_e[:, 100]).all() and np.isnan(got_s[:, :, 100]).all() and not np.isnan(got_e[:, others]).any()


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (-fno-sanitize-recover: a report is a failure).  Sums,
    states, every fold's stage and every fold's twiddle table are allocated at exactly their sizes."""
    exe = os.path.join(ROOT, "tests", "cpp", "modulation_kernel_host_san")
    subprocess.check_call(COMPILE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    rng = np.random.default_rng(18)
    for nodes, k, s, m, t, first_fold in ((257, 3, 4, 14, 33, 13), (1, 8, 1, 16, 17, 16), (255, 1, 3, 5, 1, 16)):
        sections, freqs, snaps = band_sections(k, s), freqs_of(rng, m), series(rng, t, nodes)
        steps = 5 + 3 * np.arange(t)
        energy, sums, state = run_host(exe, tmp_path, snaps, steps, freqs, sections, first_fold)
        want_e, want_s, want_z = M.modulation_fold(snaps, steps, freqs, sections, return_state=True)
        assert energy.tobytes() == want_e.tobytes() and sums.tobytes() == want_s.tobytes() and state.tobytes() == want_z.tobytes()


# ---- identities of the definition ----------------------------------------------------------------------------------------------

def test_identity_section_at_zero_frequency_is_the_plain_decay_sum():
    rng = np.random.default_rng(5)
    snaps = (rng.standard_normal((37, 3, 5)) * 10.0 ** rng.integers(-30, 3, (37, 3, 5))).astype(np.float32)
    energy, sums = M.modulation_fold(snaps, np.arange(37) * 3, [0.0], IDENTITY)
    plain = np.zeros((3, 5))
    for p in snaps:
        p = p.astype(np.float64)
        plain = plain + p * p
    assert energy.shape == (1, 3, 5) and sums.shape == (1, 1, 3, 5)
    assert energy[0].tobytes() == plain.tobytes() == np.ascontiguousarray(sums[0, 0].real).tobytes()
    assert not sums.imag.any() and plain.min() > 0
    assert energy[0].tobytes() == D.banded_bins(snaps, IDENTITY, 1, 1)[0, 0].tobytes()


def test_the_sums_are_spectrum_sums_of_the_filtered_squares():
    """Re / Im of band k equal the spectrum plan's definition applied to the series e_j = y_j^2, E the decay plan's single bin."""
    rng = np.random.default_rng(6)
    snaps = rng.standard_normal((29, 7)).astype(np.float32)
    sections, freqs, steps = band_sections(2, 3), [0.0, 0.013, 0.25, 0.5], 4 + 5 * np.arange(29)
    energy, sums = M.modulation_fold(snaps, steps, freqs, sections)
    for k in range(2):
        y, _ = D.biquad_cascade(sections[k], snaps.astype(np.float64))
        e = y * y
        re, im = np.zeros((4, 7)), np.zeros((4, 7))
        for ej, step in zip(e, steps):
            for i, f in enumerate(freqs):
                c, s = E.spectrum_twiddle(f, int(step))
                re[i] = re[i] + ej * c
                im[i] = im[i] - ej * s
        assert np.ascontiguousarray(sums[k].real).tobytes() == re.tobytes() and np.ascontiguousarray(sums[k].imag).tobytes() == im.tobytes()
        assert energy[k].tobytes() == D.banded_bins(snaps, sections[k][None], 1, 1)[0, 0].tobytes()
    assert energy[0].tobytes() != energy[1].tobytes()


def test_two_halves_with_state_and_sums_carried_equal_one_call():
    rng = np.random.default_rng(7)
    snaps = rng.standard_normal((21, 4, 3)).astype(np.float32)
    sections, freqs, steps = band_sections(3, 2), [0.001, 0.1], np.arange(21) * 2
    whole = M.modulation_fold(snaps, steps, freqs, sections, return_state=True)
    for cut in (1, 10, 20):
        e, s, z = M.modulation_fold(snaps[:cut], steps[:cut], freqs, sections, return_state=True)
        kept = (e.copy(), s.copy(), z.copy())
        e2, s2, z2 = M.modulation_fold(snaps[cut:], steps[cut:], freqs, sections, state=z, sums=(e, s), return_state=True)
        assert e2.tobytes() == whole[0].tobytes() and s2.tobytes() == whole[1].tobytes() and z2.tobytes() == whole[2].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(kept, (e, s, z)))   # what is carried is not modified


# ---- closed forms ----------------------------------------------------------------------------------------------------------------

def exponential_decay(t60, fs, n):
    r = np.exp(-6.9078 / (t60 * fs))
    return r, (r ** np.arange(n)).astype(np.float32)


def test_mtf_of_an_exponential_decay_against_the_closed_forms():
    """p_j = float32(r^j): the finite geometric series within 2^-22 (each p is rounded to float32, relative 2^-24; squaring doubles
    that, and the ratio doubles it again), and Schroeder's continuous form within 1e-5 (the difference is the discretisation)."""
    fs, t60, n = 8000.0, 0.8, 12800
    r, p = exponential_decay(t60, fs, n)
    f = M.cycles_per_step(M.STI_MODULATION_HZ, fs)
    energy, sums = M.modulation_fold(p, np.arange(n), f, IDENTITY)
    m = M.mtf(energy, sums)[0]
    assert m.shape == (14,)
    q, w = r * r, 2 * np.pi * f
    series_form = np.abs((1 - q ** n * np.exp(-1j * w * n)) / (1 - q * np.exp(-1j * w))) * (1 - q) / (1 - q ** n)
    print("largest difference from the finite geometric series: %g" % np.abs(m - series_form).max())
    print("largest difference from Schroeder's form: %g" % np.abs(m - M.schroeder_mtf(M.STI_MODULATION_HZ, t60)).max())
    assert np.abs(m - series_form).max() <= 2.0 ** -22
    assert np.abs(m - M.schroeder_mtf(M.STI_MODULATION_HZ, t60)).max() <= 1e-5
    assert (np.diff(m) < 0).all() and 0 < m[-1] < m[0] < 1


def test_sti_of_an_exponential_decay_falls_with_the_reverberation_time():
    fs, values = 500.0, []
    f = M.cycles_per_step(M.STI_MODULATION_HZ, fs)
    for t60 in (0.3, 0.6, 1.2, 2.4):
        n = int(5 * t60 * fs)
        _, p = exponential_decay(t60, fs, n)
        energy, sums = M.modulation_fold(p, np.arange(n), f, IDENTITY)
        index = M.mti(M.mtf(energy, sums))[0]
        values.append(float(M.sti({c: index for c in M.STI_OCTAVE_HZ})))
    assert all(a > b for a, b in zip(values, values[1:])), values
    assert 0 < values[-1] and values[0] < 1


# ---- STI arithmetic ----------------------------------------------------------------------------------------------------------------

def test_constants_are_the_standards():
    assert len(M.STI_MODULATION_HZ) == 14 and M.STI_MODULATION_HZ[0] == 0.63 and M.STI_MODULATION_HZ[-1] == 12.5
    assert all(abs(b / a - 10 ** 0.1) < 0.03 for a, b in zip(M.STI_MODULATION_HZ, M.STI_MODULATION_HZ[1:]))   # third-octave steps
    assert M.STI_OCTAVE_HZ == (125, 250, 500, 1000, 2000, 4000, 8000)
    assert M.STI_ALPHA == (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173) and M.STI_BETA == (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)
    assert sum(M.STI_ALPHA) - sum(M.STI_BETA) == pytest.approx(1.0, abs=1e-15)
    assert M.cycles_per_step([8.0, 12.5], 8000.0).tolist() == [0.001, 12.5 / 8000.0]


def test_sti_of_constant_transfer_values():
    for value, want in ((1.0, 1.0), (0.5, 0.5), (0.0, 0.0)):
        m = np.full((7, 14, 2, 3), value)
        index = M.mti(m)
        assert index.shape == (7, 2, 3) and (index == want).all()
        got = M.sti(dict(zip(M.STI_OCTAVE_HZ, index)))
        assert got.shape == (2, 3) and np.abs(got - want).max() <= 4e-16   # (float addition of thirteen weights)
    assert (M.transmission_index([1.5, 1.0, -0.1]) == [1.0, 1.0, 0.0]).all() and np.isnan(M.transmission_index(np.nan))


def test_the_clip_engages_at_fifteen_decibels():
    hi, lo = 1 / (1 + 10 ** -1.5), 1 / (1 + 10 ** 1.5)
    assert M.transmission_index(hi) == pytest.approx(1.0, abs=1e-12) and M.transmission_index(lo) == pytest.approx(0.0, abs=1e-12)
    assert M.transmission_index(hi + 1e-3) == 1.0 and M.transmission_index(0.999999) == 1.0
    assert M.transmission_index(lo - 1e-3) == 0.0 and M.transmission_index(1e-9) == 0.0
    assert 0.99 < M.transmission_index(hi - 1e-3) < 1.0 and 0.0 < M.transmission_index(lo + 1e-3) < 0.01
    assert M.transmission_index(0.5) == 0.5


def test_mtf_is_nan_where_there_is_no_energy():
    energy = np.array([[0.0, 2.0]])
    sums = np.array([[[0.0 + 0.0j, 1.0 - 1.0j]]])
    m = M.mtf(energy, sums)
    assert m.shape == (1, 1, 2) and np.isnan(m[0, 0, 0]) and m[0, 0, 1] == np.sqrt(2.0) / 2.0


def test_missing_bands_are_named_and_rest_completes_them():
    low = {125: 0.6, 250: 0.5, 500: 0.4}
    with pytest.raises(ValueError, match="1000 Hz"):
        M.sti(low)
    with pytest.raises(ValueError, match="8000 Hz"):
        M.sti(low, rest={1000: 0.5, 2000: 0.5, 4000: 0.5})
    rest = {1000: 0.5, 2000: 0.45, 4000: 0.4, 8000: 0.35}
    bands = [0.6, 0.5, 0.4, 0.5, 0.45, 0.4, 0.35]
    want = sum(a * v for a, v in zip(M.STI_ALPHA, bands)) - sum(b * np.sqrt(x * y) for b, x, y in zip(M.STI_BETA, bands, bands[1:]))
    assert float(M.sti(low, rest=rest)) == pytest.approx(want, abs=1e-15)
    # maps in the mesh's bands, scalars for the rest; one scalar for every band the mesh does not carry
    maps = {c: np.full((2, 2), v) for c, v in low.items()}
    got = M.sti(maps, rest=rest)
    assert got.shape == (2, 2) and np.abs(got - want).max() <= 1e-15
    assert float(M.sti(low, rest=0.5)) == pytest.approx(float(M.sti(low, rest={c: 0.5 for c in (1000, 2000, 4000, 8000)})), abs=0)
    assert float(M.sti({c: 0.7 for c in M.STI_OCTAVE_HZ})) == pytest.approx(0.7, abs=1e-15)

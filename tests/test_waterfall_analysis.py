"""wayverb_amd/waterfall.py on the CPU: identities of the definition, the cumulative spectral decay against the one-bin sum within the
bound of two recursive summations, and the decay time of a single synthetic mode."""
import numpy as np
import pytest

from helpers import numpy_fold
from wayverb_amd import decay as D
from wayverb_amd import waterfall as WF


def noise(seed, shape):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 2, shape)).astype(np.float32)


def test_one_bin_is_the_spectrum_definition_bytewise(built_library):
    snaps, steps, freqs = noise(1, (37, 3, 5)), 4 + 3 * np.arange(37), [0.0, 0.013, 0.25, 0.5]
    for bin_captures in (1, 7, 100):
        got = WF.waterfall_fold(snaps, steps, freqs, 1, bin_captures)
        assert got.shape == (1, 4, 3, 5) and got[0].tobytes() == numpy_fold(snaps, steps, freqs).tobytes()
    assert np.abs(got).max() > 0


def test_every_bin_is_the_spectrum_of_its_own_captures_and_untouched_bins_are_plus_zero(built_library):
    snaps, steps, freqs = noise(2, (23, 6)), 2 * np.arange(23), [0.0, 0.1, 0.37]
    got = WF.waterfall_fold(snaps, steps, freqs, 9, 4)
    for b in range(5):
        assert got[b].tobytes() == numpy_fold(snaps[4 * b:4 * b + 4], steps[4 * b:4 * b + 4], freqs).tobytes()
    assert got[5].tobytes() == numpy_fold(snaps[20:], steps[20:], freqs).tobytes()
    raw = np.stack([got[6:].real, got[6:].imag])
    assert not raw.any() and not np.signbit(raw).any()
    # the last bin is open-ended
    short = WF.waterfall_fold(snaps, steps, freqs, 3, 4)
    assert short[:2].tobytes() == got[:2].tobytes() and short[2].tobytes() == numpy_fold(snaps[8:], steps[8:], freqs).tobytes()


def test_two_halves_with_the_sums_carried_equal_one_call(built_library):
    snaps, steps, freqs = noise(3, (21, 4, 3)), 5 + 2 * np.arange(21), [0.001, 0.1]
    whole = WF.waterfall_fold(snaps, steps, freqs, 4, 3)
    for cut in (1, 10, 20):
        first = WF.waterfall_fold(snaps[:cut], steps[:cut], freqs, 4, 3)
        kept = first.copy()
        both = WF.waterfall_fold(snaps[cut:], steps[cut:], freqs, 4, 3, first_capture=cut, sums=first)
        assert both.tobytes() == whole.tobytes() and first.tobytes() == kept.tobytes()      # what is carried is not modified
    with pytest.raises(ValueError, match="one step per snapshot"):
        WF.waterfall_fold(snaps, steps[:-1], freqs, 4, 3)


def test_the_first_edge_of_the_csd_is_the_whole_run_spectrum_within_the_summation_bound(built_library):
    """Y[0] sums the same rounded products p_j * c as the one-bin sum, in another order: both are recursive summations of n terms, each
    within (n - 1) u sum|p c| (1 + O(u)) of the exact sum, u = 2^-53, and the products carry one rounding each -- so the two differ by
    no more than 2 (n + 2) 2^-53 sum_j |p_j| per node and frequency, |c|, |s| <= 1."""
    for seed, n, w, n_bins in ((4, 200, 7, 12), (5, 64, 1, 64), (6, 333, 50, 3)):
        snaps, steps = noise(seed, (n, 17)), 3 * np.arange(n)
        freqs = [0.0, 0.02, 0.1234, 0.5]
        bins = WF.waterfall_fold(snaps, steps, freqs, n_bins, w)
        csd = WF.cumulative_spectral_decay(bins)
        whole = numpy_fold(snaps, steps, freqs)
        bound = 2 * (n + 2) * 2.0 ** -53 * np.abs(snaps.astype(np.float64)).sum(axis=0)
        assert csd.shape == bins.shape and csd[-1].tobytes() == bins[-1].tobytes()
        for part in (csd[0].real - whole.real, csd[0].imag - whole.imag):
            assert (np.abs(part) <= bound).all(), (seed, np.abs(part).max(), bound.min())
        assert np.abs(whole).max() > 0 and bound.min() > 0
        # and every edge is the spectrum of what is still to come
        edge = n_bins // 2
        tail = numpy_fold(snaps[edge * w:], steps[edge * w:], freqs)
        assert (np.abs(csd[edge].real - tail.real) <= bound).all() and (np.abs(csd[edge].imag - tail.imag) <= bound).all()
    assert WF.cumulative_spectral_decay(np.zeros((0, 2, 3), np.complex128)).shape == (0, 2, 3)


def mode(f0, delta, period, n_steps=8192):
    steps = np.arange(0, n_steps, period)
    return steps, np.float32(np.exp(-delta * steps) * np.cos(2 * np.pi * f0 * steps + 0.3)).reshape(-1, 1)


MODES = [(0.05, 0.002, 1), (0.05, 0.002, 4), (0.0173, 0.001, 2), (0.11, 0.004, 1)]


@pytest.mark.parametrize("f0,delta,period", MODES)
def test_modal_decay_time_of_a_single_mode_within_one_percent(built_library, f0, delta, period):
    """p = float32(exp(-delta n) cos(2 pi f0 n + 0.3)) at n = 0, period, ... < 8192, bins 64 steps long, folded at f0: |Y[b]|^2 falls by
    exp(-2 delta) per step, so the line reaches -60 dB after 3 ln 10 / delta steps.  Within 1 %."""
    steps, p = mode(f0, delta, period)
    bin_captures = 64 // period
    n_bins = -(-len(steps) // bin_captures)
    bins = WF.waterfall_fold(p, steps, [f0, 1.5 * f0], n_bins, bin_captures)
    rate = 1000.0
    got = WF.modal_decay_time(bins, bin_captures, period, rate)
    want = 3.0 * np.log(10.0) / delta / rate
    error = abs(float(got[0, 0]) - want) / want
    print("f0 %g delta %g period %d: %.6g s against %.6g s, off by %.3f %%" % (f0, delta, period, got[0, 0], want, 100 * error))
    assert got.shape == (2, 1) and error <= 0.01
    # a frequency off the mode sits lower at bin 0 than the mode does
    level = WF.short_time_level_db(bins, reference=1.0)
    assert level[0, 1, 0] < level[0, 0, 0] and np.isfinite(level[0]).all()
    csd = WF.csd_level_db(bins)
    assert (csd[0] == 0).all() and csd[n_bins // 2, 0, 0] < -20


def test_modal_decay_time_is_nan_without_three_points_and_for_silence(built_library):
    steps, p = mode(0.05, 0.002, 1)
    bins = WF.waterfall_fold(p, steps, [0.05], 128, 64)
    assert np.isnan(WF.modal_decay_time(bins[:2], 64, 1, 1000.0)).all()                     # two edges
    assert np.isnan(WF.modal_decay_time(bins, 64, 1, 1000.0, lo_db=-5.0, hi_db=-6.0)).all()  # one edge in the range: -5.56 dB
    assert np.isnan(WF.modal_decay_time(np.zeros((16, 2, 3), np.complex128), 4, 1, 1000.0)).all()
    maps = WF.waterfall_maps(bins, 64, 1, 1000.0)
    assert sorted(maps) == ["csd", "csd_db", "decay_s", "short_time_db", "times_s"]
    assert maps["times_s"].tolist() == (D.bin_times(128, 64, 1) / 1000.0).tolist() and maps["csd"].shape == bins.shape
    assert maps["decay_s"].tobytes() == WF.modal_decay_time(bins, 64, 1, 1000.0).tobytes()
    assert maps["short_time_db"].max() == 0.0

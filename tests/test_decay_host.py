"""wayverb_amd/decay.py on the CPU: the energy decay curve on hand-made bins, the decay times against values recorded from the
reference's own rt20 / rt30 / edt (tests/golden/schroeder_reference.npz, recipe in tests/golden/schroeder_reference.md), the reference's
known-answer test (src/core/tests/schroeder.cpp) on binned noise, and NaN where the reference throws."""
import os

import numpy as np
import pytest

from wayverb_amd import decay as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_energy_decay_curve_on_hand_made_bins():
    bins = np.array([[1.0, 0.0, 4.0], [2.0, 0.0, 0.0], [0.5, 0.0, 0.25]])
    curve = D.energy_decay_curve(bins)
    assert curve.tolist() == [[3.5, 0.0, 4.25], [2.5, 0.0, 0.25], [0.5, 0.0, 0.25]]
    # the order of summation is backward: S[b] = S[b+1] + E[b], which 1 + 2^-53 + 2^-53 tells from the forward order
    tiny = 2.0 ** -53
    assert D.energy_decay_curve(np.array([1.0, tiny, tiny]))[0] == 1.0 + 2 * tiny
    assert (1.0 + tiny) + tiny == 1.0
    assert D.energy_decay_curve(np.zeros((0, 4))).shape == (0, 4)
    assert D.energy_decay_curve(np.ones((5, 2, 3)))[:, 1, 2].tolist() == [5.0, 4.0, 3.0, 2.0, 1.0]
    assert D.bin_times(4, 5, 3).tolist() == [0.0, 15.0, 30.0, 45.0]


def test_decay_times_agree_with_the_reference_on_recorded_signals():
    """Six seeded double signals and what the reference's rt20 / rt30 / edt return for them.  With one capture per bin and a capture
    every step decay.py sees the reference's numbers and mirrors its arithmetic: the same backward sums, float32 points, float32
    products in the five double sums.  What may differ is libm's log10 against NumPy's, an ulp of a double, ahead of the rounding to
    float32: 1e-12 relative."""
    with np.load(os.path.join(ROOT, "tests", "golden", "schroeder_reference.npz")) as f:
        want = f["results"]
        signals = [f["signal_%d" % i] for i in range(want.shape[0])]
    assert want.shape == (6, 3, 2)
    for signal, rows in zip(signals, want):
        curve = D.energy_decay_curve(signal * signal)
        times = D.bin_times(len(signal), 1, 1)
        for fn, (samples, r) in zip((D.rt20, D.rt30, D.edt), rows):
            got_samples, got_r = fn(curve, times)
            print("%s: %r against %r, r %r against %r" % (fn.__name__, float(got_samples), samples, float(got_r), r))
            assert abs(got_samples - samples) <= 1e-12 * abs(samples)
            assert abs(got_r - r) <= 1e-12 * abs(r)
    # the same signals as the nodes of one call: vectorised over the node axes
    n = min(len(s) for s in signals)
    stacked = np.stack([s[-n:] for s in signals], axis=1).reshape(n, 2, 3)
    curve = D.energy_decay_curve(stacked * stacked)
    together, _ = D.rt30(curve, D.bin_times(n, 1, 1))
    for i in range(6):
        alone, _ = D.rt30(D.energy_decay_curve(signals[i][-n:] ** 2), D.bin_times(n, 1, 1))
        assert together.reshape(6)[i] == alone or (np.isnan(alone) and np.isnan(together.reshape(6)[i]))


@pytest.mark.parametrize("length", [1000, 2000, 10000, 20000])
def test_the_references_known_answer_on_binned_noise(length):
    """src/core/tests/schroeder.cpp: uniform noise under an exponential envelope that reaches -60 dB at `length`; rt20, rt30 and edt
    lie within 10 % of `length`.  W = 1 is the reference's algorithm itself; W = 10 and W = length // 50 are what a decay plan gives."""
    rng = np.random.default_rng(length)
    i = np.arange(length)
    noise = rng.uniform(-1.0, 1.0, length) * np.exp(np.log(10.0 ** (-60.0 / 20.0)) * i / length)
    for per_bin in (1, 10, length // 50):
        n_bins = -(-length // per_bin)
        bins = np.zeros(n_bins)
        for j in range(length):
            bins[j // per_bin] = bins[j // per_bin] + noise[j] * noise[j]
        curve = D.energy_decay_curve(bins)
        times = D.bin_times(n_bins, per_bin, 1)
        for fn in (D.rt20, D.rt30, D.edt):
            samples, r = fn(curve, times)
            print("length %d, W = %d, %s: %.1f (r = %.5f)" % (length, per_bin, fn.__name__, samples, r))
            assert abs(samples - length) <= 0.1 * length
            assert -1.0 <= r < -0.95


def test_period_shifts_the_level_and_leaves_the_times():
    """Every third sample of a band-limited decay: the level map falls by 10 log10(3), the decay times stay."""
    rng = np.random.default_rng(5)
    n = 30000
    white = rng.standard_normal(n + 64)
    kernel = np.hanning(65) * np.sinc((np.arange(65) - 32) * 0.2)             # low-pass at 0.1 of the sample rate: below 1 / 6
    signal = np.convolve(white, kernel, mode="valid") * np.exp(np.log(1e-3) * np.arange(n) / n)
    maps = {}
    for period in (1, 3):
        taken = signal[::period]
        per_bin = 300 // period
        bins = (taken[:len(taken) // per_bin * per_bin].reshape(-1, per_bin) ** 2).sum(axis=1)
        maps[period] = D.decay_maps(bins, per_bin, period, 1000.0)
    assert abs((maps[1]["level_db"] - maps[3]["level_db"]) - 10 * np.log10(3.0)) < 0.1
    for name in ("edt_s", "t20_s", "t30_s"):
        assert abs(maps[3][name] / maps[1][name] - 1.0) < 0.01 and abs(maps[1][name] - 30.0) < 3.0


def test_nan_where_the_reference_throws():
    """Silence (0 / 0 levels), a curve that never enters the range, one point in the range: NaN for the time and for r; the other
    nodes of the same call are not disturbed."""
    n = 200
    decay = 10.0 ** (-6.0 * np.arange(n) / n)                                # -60 dB over the run: energy per bin
    bins = np.zeros((n, 4))
    bins[:, 0] = decay
    bins[:, 2] = [1.0] + [0.0] * (n - 1)                                     # everything in the first bin: levels 0, -inf, -inf, ...
    bins[:3, 3] = [1.0, 0.2, 1e-9]                                           # levels 0, -7.8, -97: one point in 0 .. -10
    maps = D.decay_maps(bins, 1, 1, 100.0)
    for name in ("edt", "t20", "t30"):
        assert np.isfinite(maps[name + "_s"][0]) and maps[name + "_r"][0] < -0.95
        assert np.isnan(maps[name + "_s"][1:]).all() and np.isnan(maps[name + "_r"][1:]).all()
    assert maps["level_db"][1] == -np.inf and np.isfinite(maps["level_db"][[0, 2, 3]]).all()
    assert np.isnan(maps["edc_db"][:, 1]).all() and maps["edc_db"][0, 0] == 0.0
    alone = D.decay_maps(bins[:, 0], 1, 1, 100.0)
    assert alone["t30_s"] == maps["t30_s"][0] and alone["t30_s"].shape == ()
    assert abs(maps["t30_s"][0] - 2.0) < 0.2                                  # 200 steps to -60 dB at 100 Hz
    with pytest.raises(ValueError):
        D.decay_time_from_points(np.ones((4, 2)), [0.0, 1.0, 2.0], -5, -25, -60)

"""Waterfall maps from time-binned field spectra (Engine.set_waterfall / fetch_waterfall): the short-time spectrum, the cumulative
spectral decay and the decay time of single modes, per node.  NumPy only.

The bins X[b][k] hold the Fourier sum at frequency k over the captures of time bin b, with the twiddles of the captures' ABSOLUTE steps
(include/wayverb_amd.h, wv_set_waterfall).  So the bins add coherently: the backward running sums Y[b] = X[b] + X[b+1] + ... are the
Fourier transform of the response with everything before capture b * bin_captures cut away -- the cumulative spectral decay (CSD) at the
bin edges, exactly but for the order of summation, because the last bin is open-ended -- and Y[0] is the whole-run spectrum.  |X[b]|^2
is the short-time spectrum under a rectangular window one bin long.  Where one mode dominates a frequency, 10 log10 |Y[b]|^2 falls on a
straight line, and its slope is that mode's decay time (modal_decay_time): what an octave-band decay curve cannot give below the
cutoff, where the modes are further apart than any band filter is narrow.

waterfall_fold is the definition of what the engine folds, in NumPy, to the last bit.
"""
import numpy as np

from . import decay as _decay


def waterfall_fold(snaps, steps, freqs, n_bins, bin_captures, first_capture=0, sums=None):
    """What a waterfall plan folds, from the snapshots float32[n, ...nodes] of the same plan and their steps [n]: freqs float64[K] in
    cycles per step -> complex128[n_bins, K, ...nodes].  Capture j goes to bin b(j) = min(j // bin_captures, n_bins - 1); in capture
    order Re[b][k] = Re[b][k] + p * c, Im[b][k] = Im[b][k] - p * s with (c, s) = engine.spectrum_twiddle(f_k, step) -- every product and
    sum a float64 array operation of its own, from +0.0.  `sums` and `first_capture` continue an earlier call (`sums` is not modified)."""
    from . import engine as E
    freqs = np.asarray(freqs, dtype=np.float64).reshape(-1)
    snaps = np.asarray(snaps)
    steps = [int(n) for n in np.asarray(steps).reshape(-1)]
    if len(steps) != snaps.shape[0]:
        raise ValueError("waterfall_fold: one step per snapshot")
    n_bins, bin_captures = int(n_bins), int(bin_captures)
    shape = (n_bins, freqs.shape[0]) + tuple(snaps.shape[1:])
    if sums is None:
        re, im = np.zeros(shape), np.zeros(shape)
    else:
        sums = np.asarray(sums, dtype=np.complex128).reshape(shape)
        re, im = sums.real.copy(), sums.imag.copy()
    for j, (p, step) in enumerate(zip(snaps, steps)):
        p = p.astype(np.float64)
        b = min((int(first_capture) + j) // bin_captures, n_bins - 1)
        for k, f in enumerate(freqs):
            c, s = E.spectrum_twiddle(f, step)
            re[b, k] = re[b, k] + p * c
            im[b, k] = im[b, k] - p * s
    out = np.empty(shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def cumulative_spectral_decay(bins):
    """The backward running sum of the bins along axis 0: Y[last] = X[last], Y[b] = Y[b+1] + X[b] (complex128, the order
    decay.energy_decay_curve sums the energy bins in): the spectrum of what is still to come at every bin edge."""
    x = np.asarray(bins, dtype=np.complex128)
    y = np.empty_like(x)
    if x.shape[0] == 0:
        return y
    y[-1] = x[-1]
    for b in range(x.shape[0] - 2, -1, -1):
        y[b] = y[b + 1] + x[b]
    return y


def _level_db(power, reference):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(power / reference)


def short_time_level_db(bins, reference=None):
    """10 log10 |X[b][k]|^2 over `reference` (default: each node's and frequency's largest bin, so that the loudest bin is 0 dB): the
    short-time spectrum, [n_bins, K, ...nodes].  -inf where a bin is silent, NaN where a node is silent throughout."""
    power = np.abs(np.asarray(bins, dtype=np.complex128)) ** 2
    if reference is None:
        reference = power.max(axis=0) if power.shape[0] else 1.0
    return _level_db(power, reference)


def csd_level_db(bins):
    """10 log10 (|Y[b][k]|^2 / |Y[0][k]|^2), Y the cumulative spectral decay: the waterfall as it is drawn, 0 dB at the first edge."""
    power = np.abs(cumulative_spectral_decay(bins)) ** 2
    return _level_db(power, power[0] if power.shape[0] else 1.0)


def modal_decay_time(bins, bin_captures, period, sample_rate, lo_db=-5.0, hi_db=-25.0):
    """The decay time of whatever rings at each frequency, in SECONDS PER 60 dB, [K, ...nodes]: the least-squares line through the
    points (edge time, csd_level_db) of the bin edges whose level lies in hi_db <= level <= lo_db, in float64.  NaN where fewer than
    three edges do, or where the line does not fall.  A single mode of damping delta per step gives 3 ln 10 / delta steps."""
    level = csd_level_db(bins)
    times = _decay.bin_times(level.shape[0], bin_captures, period).reshape((-1,) + (1,) * (level.ndim - 1))
    use = (level >= float(hi_db)) & (level <= float(lo_db))         # (a NaN level -- silence -- is in no range)
    x = np.where(use, times, 0.0)
    y = np.where(use, level, 0.0)
    n = use.sum(axis=0).astype(np.float64)
    sx, sy, sxx, sxy = x.sum(axis=0), y.sum(axis=0), (x * x).sum(axis=0), (x * y).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (n * sxy - sx * sy) / (n * sxx - sx * sx)             # dB per step
        steps = -60.0 / slope
    bad = (n < 3) | ~(slope < 0.0) | ~np.isfinite(steps)
    return np.where(bad, np.nan, steps / float(sample_rate))


def waterfall_maps(bins, bin_captures, period, sample_rate, lo_db=-5.0, hi_db=-25.0):
    """Bins complex128[n_bins, K, ...nodes] of a waterfall plan with `bin_captures` captures per bin and a capture every `period`
    steps -> dict(times_s: the bin edges in seconds from the first capture [n_bins]; csd: the cumulative spectral decay, complex;
    csd_db = csd_level_db; short_time_db = short_time_level_db; decay_s = modal_decay_time [K, ...nodes])."""
    bins = np.asarray(bins, dtype=np.complex128)
    return dict(times_s=_decay.bin_times(bins.shape[0], bin_captures, period) / float(sample_rate), csd=cumulative_spectral_decay(bins),
                csd_db=csd_level_db(bins), short_time_db=short_time_level_db(bins),
                decay_s=modal_decay_time(bins, bin_captures, period, sample_rate, lo_db, hi_db))

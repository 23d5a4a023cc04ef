"""Energy decay maps from time-binned field energy (Engine.set_decay / fetch_decay): the energy decay curve, the reverberation times
EDT / T20 / T30 and the level, per node.  NumPy only.

The bins E[b] hold the sum of p^2 over the captures of time bin b (include/wayverb_amd.h, wv_set_decay).  Their backward running sums
S[b] = E[b] + E[b+1] + ... are the Schroeder integral -- the energy still to come -- at the bin edges, exactly but for the order of
summation, because the last bin is open-ended.  decay_time_from_points and rt20 / rt30 / edt restate the reference's algorithm
(src/core/include/core/schroeder.h, linear_regression.h), which takes one receiver trace; here it runs over all nodes at once and on
the curve at the bin edges.  With one capture per bin and a capture every step the two see the same numbers.

Band-limited maps (Engine.set_decay(bands=...), wv_set_decay_bands): octave_band_edges, butterworth_bandpass and bandpass_biquad
supply the sections (the reference's designs, src/core/src/filters_common.cpp, through the library's host functions);
biquad_cascade and banded_bins are the definition of what the engine folds, in NumPy, to the last bit; band_decay_maps is decay_maps
per band.
"""
import ctypes as _C

import numpy as np


def energy_decay_curve(bins):
    """The backward running sum of the bins along axis 0: S[last] = E[last], S[b] = S[b+1] + E[b] (float64, the order the reference's
    squared_integrated sums a reversed trace in)."""
    e = np.asarray(bins, dtype=np.float64)
    s = np.empty_like(e)
    if e.shape[0] == 0:
        return s
    s[-1] = e[-1]
    for b in range(e.shape[0] - 2, -1, -1):
        s[b] = s[b + 1] + e[b]
    return s


def decay_time_from_points(curve, times, begin_db, end_db, min_db):
    """The reference's decay_time_from_points on the decay curve S = `curve` [n, ...nodes] sampled at `times` [n] (in steps): the
    levels 10 log10(S_b / S_0) and the times are held as float32 (the reference's glm::vec2), the points with end_db <= level <
    begin_db are taken latest first, their five sums sx, sy, sxx, sxy, syy run in double over float32 products, and the regression
    line level = m * time + c gives the time at which it reaches min_db.  Returns (time in steps, r), each of the nodes' shape; r is the
    product-moment correlation coefficient (-1 <= r < -0.95 is a decay to trust).  Nodes whose regression is empty or degenerate --
    silence, fewer than two points in the range, a line that does not fall -- get NaN where the reference throws."""
    s = np.asarray(curve, dtype=np.float64)
    t32 = np.asarray(times, dtype=np.float64).astype(np.float32).reshape((-1,) + (1,) * (s.ndim - 1))
    if t32.shape[0] != s.shape[0]:
        raise ValueError("decay_time_from_points: %d times for %d points of the curve" % (t32.shape[0], s.shape[0]))
    begin_db, end_db, min_db = np.float32(begin_db), np.float32(end_db), np.float32(min_db)
    nodes = s.shape[1:]
    n = np.zeros(nodes)
    sx, sy, sxx, sxy, syy = (np.zeros(nodes) for _ in range(5))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(s.shape[0] - 1, -1, -1):                      # latest first, as the reference walks them
            y = (10 * np.log10(s[b] / s[0])).astype(np.float32)
            x = np.broadcast_to(t32[b], nodes)
            use = (y >= end_db) & (y < begin_db)                     # (a NaN level -- silence -- is in no range)
            if not use.any():
                continue
            n = n + use
            sx = sx + np.where(use, x, np.float32(0)).astype(np.float64)
            sy = sy + np.where(use, y, np.float32(0)).astype(np.float64)
            sxx = sxx + np.where(use, x * x, np.float32(0)).astype(np.float64)      # (float32 products, as i.x * i.x is)
            sxy = sxy + np.where(use, x * y, np.float32(0)).astype(np.float64)
            syy = syy + np.where(use, y * y, np.float32(0)).astype(np.float64)
        denominator = n * sxx - sx * sx
        numerator = n * sxy - sx * sy
        m = numerator / denominator
        c = sy / n - m * sx / n
        r = numerator / np.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy))
        samples = (np.float64(min_db) - c) / m
        bad = (n < 2) | (denominator == 0.0) | ~(m < 0.0) | ~np.isfinite(samples)
    return np.where(bad, np.nan, samples), np.where(bad, np.nan, r)


def rt20(curve, times):
    """-5 dB .. -25 dB, extrapolated to -60 dB."""
    return decay_time_from_points(curve, times, -5, -25, -60)


def rt30(curve, times):
    """-5 dB .. -35 dB, extrapolated to -60 dB."""
    return decay_time_from_points(curve, times, -5, -35, -60)


def edt(curve, times):
    """0 dB .. -10 dB, extrapolated to -60 dB."""
    return decay_time_from_points(curve, times, 0, -10, -60)


def bin_times(n_bins, bin_captures, period=1):
    """The step offsets of the bin edges from the first capture: b * bin_captures * period."""
    return np.arange(int(n_bins), dtype=np.float64) * (int(bin_captures) * int(period))


def decay_maps(bins, bin_captures, period, sample_rate):
    """Bins float64[n_bins, ...nodes] of a decay plan with `bin_captures` captures per bin and a capture every `period` steps ->
    dict(edt_s, t20_s, t30_s: the decay times in seconds; edt_r, t20_r, t30_r: their correlation coefficients; level_db = 10 log10 of
    the whole captured energy S_0 (-inf at silent nodes; with period k it lies 10 log10(k) below the every-step level as long as the
    field holds nothing above sample_rate / (2 k)); edc_db = 10 log10(S_b / S_0) [n_bins, ...nodes])."""
    bins = np.asarray(bins, dtype=np.float64)
    curve = energy_decay_curve(bins)
    times = bin_times(bins.shape[0], bin_captures, period)
    out = {}
    for name, fn in (("edt", edt), ("t20", rt20), ("t30", rt30)):
        steps, r = fn(curve, times)
        out[name + "_s"] = steps / float(sample_rate)
        out[name + "_r"] = r
    with np.errstate(divide="ignore", invalid="ignore"):
        out["level_db"] = 10 * np.log10(curve[0]) if bins.shape[0] else np.zeros(bins.shape[1:])
        out["edc_db"] = 10 * np.log10(curve / curve[0]) if bins.shape[0] else curve
    return out


# ---- band-limited decay maps ---------------------------------------------------------------------------------------------------

def octave_band_edges(centres):
    """Octave bands around `centres` (Hz): [(c / sqrt 2, c * sqrt 2), ...]."""
    r2 = np.sqrt(2.0)
    return [(float(c) / r2, float(c) * r2) for c in np.atleast_1d(np.asarray(centres, dtype=np.float64))]


def _design(name, n, lo, hi, sample_rate):
    from . import engine as E
    out = np.zeros((n, 5), dtype=np.float64)
    E._check(getattr(E.load_library(), name)(float(lo), float(hi), float(sample_rate), out.ctypes.data_as(_C.c_void_p)))
    return out


def butterworth_bandpass(lo, hi, sample_rate):
    """wv_butterworth_bandpass: float64[4][5], the reference's compute_hipass_butterworth_coefficients<2>(lo) followed by
    compute_lopass_butterworth_coefficients<2>(hi) -- b0, b1, b2, a1, a2 per section, a 4th-order Butterworth slope on either side.
    `sample_rate` is the rate of the series the filter runs on: a decay plan's is the mesh's sample rate / period."""
    return _design("wv_butterworth_bandpass", 4, lo, hi, sample_rate)


def bandpass_biquad(lo, hi, sample_rate):
    """wv_bandpass_biquad: float64[1][5], the reference's compute_bandpass_biquad_coefficients (one constant-skirt section)."""
    return _design("wv_bandpass_biquad", 1, lo, hi, sample_rate)


def biquad_run(sections, x, state=None):
    """wv_biquad_run: the 1-D float64 series x through the cascade float64[S][5] on the host, in C.  `state` float64[S][2] is
    carried (read, and written back in place); None starts from +0.0.  Returns the outputs."""
    from . import engine as E
    sections = np.ascontiguousarray(sections, dtype=np.float64).reshape(-1, 5)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    out = np.empty_like(x)
    if state is not None and (state.dtype != np.float64 or state.shape != (sections.shape[0], 2) or not state.flags.c_contiguous):
        raise ValueError("biquad_run: state is a C-contiguous float64[S][2]")
    E._check(E.load_library().wv_biquad_run(sections.ctypes.data_as(_C.c_void_p), sections.shape[0], x.ctypes.data_as(_C.c_void_p), x.shape[0],
                                            None if state is None else state.ctypes.data_as(_C.c_void_p), out.ctypes.data_as(_C.c_void_p)))
    return out


def biquad_cascade(sections, x, state=None):
    """The definition of the band filter (include/wayverb_amd.h, wv_set_decay_bands) in NumPy: x float64[n, ...nodes] through the
    sections float64[S][5] in series, transposed direct form II, every product and sum a float64 array operation of its own, a Python
    loop over time.  `state` float64[S][2, ...nodes] to carry on from (not modified); None = +0.0.  Returns (y like x, final state)."""
    sections = np.asarray(sections, dtype=np.float64).reshape(-1, 5)
    x = np.asarray(x, dtype=np.float64)
    nodes = x.shape[1:]
    z = np.zeros((sections.shape[0], 2) + nodes) if state is None else np.array(state, dtype=np.float64).reshape((sections.shape[0], 2) + nodes)
    y = np.empty_like(x)
    for j in range(x.shape[0]):
        v = x[j]
        for s, (b0, b1, b2, a1, a2) in enumerate(sections):
            out = v * b0 + z[s, 0]
            z[s, 0] = (v * b1 - a1 * out) + z[s, 1]
            z[s, 1] = v * b2 - a2 * out
            v = out
        y[j] = v
    return y, z


def banded_bins(snaps, sections, n_bins, bin_captures, state=None, first_capture=0, return_state=False):
    """What a banded decay plan folds, from the snapshots float32[n, ...nodes] of the same plan: sections float64[K][S][5] ->
    bins float64[K, n_bins, ...nodes], E[k][b(j)] = E[k][b(j)] + y * y in capture order with b(j) = min(j // bin_captures,
    n_bins - 1).  `state` float64[K][S][2, ...nodes] and `first_capture` continue an earlier call; return_state adds the final state."""
    sections = np.asarray(sections, dtype=np.float64)
    sections = sections.reshape((-1,) + sections.shape[-2:])
    x = np.asarray(snaps).astype(np.float64)
    bins = np.zeros((sections.shape[0], int(n_bins)) + x.shape[1:])
    states = []
    for k in range(sections.shape[0]):
        y, z = biquad_cascade(sections[k], x, None if state is None else state[k])
        states.append(z)
        for j in range(x.shape[0]):
            b = min((int(first_capture) + j) // int(bin_captures), int(n_bins) - 1)
            bins[k, b] = bins[k, b] + y[j] * y[j]
    return (bins, np.array(states)) if return_state else bins


def band_decay_maps(bins, bin_captures, period, sample_rate):
    """decay_maps for every band of bins float64[K, n_bins, ...nodes]: the same dict, every array with a leading band axis."""
    bins = np.asarray(bins, dtype=np.float64)
    per_band = [decay_maps(bins[k], bin_captures, period, sample_rate) for k in range(bins.shape[0])]
    return {name: np.array([m[name] for m in per_band]) for name in per_band[0]} if per_band else {}

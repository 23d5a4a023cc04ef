"""Interaural maps (Engine.set_interaural / fetch_interaural): the inter-aural cross-correlation function IACF and its maximum IACC
(ISO 3382-1 Annex B; early, late, whole) at every node of a box, and the lag of that maximum.  NumPy only.

For every node taken the engine reads the field at two nodes an ear-distance apart and sums, in bins counted from the node's OWN
onset, the two energies Ea, Eb and the lagged products C[tau], tau = -L .. L captures (include/wayverb_amd.h, "interaural maps").
interaural_fold is the DEFINITION of that fold, operation by operation: fed snapshots of the two ear planes it reproduces onset, pre,
the lag history and all bins to the last bit, in one piece or in several.  The rest turns the bins into acoustics:
IACF(tau) = C[tau] / sqrt(Ea Eb) over a window of bins, IACC = max |IACF|.

The waveguide carries the band below the crossover, where the head is small against the wavelength and the inter-aural difference is a
time difference between two points in space: two mesh nodes 0.15 - 0.2 m apart are the head-less ("spaced omni") form of the
measurement.  It is not a dummy head.  With both ears on the same node the plan is a per-seat autocorrelation (autocorrelation()).

tau = +l means ear a EARLIER, ear b later by l captures.  A product goes to the bin of the LATER of its two samples, which differs
from ISO's "window on the left ear's time" by at most L captures at a bin edge.
"""
import math

import numpy as np

from .arrival import NONE, _check_edges, edges_from_ms   # noqa: F401  (edges_from_ms is re-exported)
from .decay import butterworth_bandpass                   # noqa: F401  (the band both ears run through is designed there)

KEYS = ("onset", "pre", "bins", "history", "filter")
MAX_BINS = 4
MAX_LAG = 16
MAX_EAR = 8


def interaural_fold(ear_a_snaps, ear_b_snaps, threshold, edges, max_lag, sections=None, state=None, first_capture=0, return_state=False):
    """The definition.  ear_a_snaps, ear_b_snaps float32 [T, ...nodes]: what the field holds at every taken node's two ears at captures
    first_capture, first_capture + 1, ...; `threshold` a scalar or a float32 array of the nodes' shape; `edges` the first relative
    capture of every bin (4 at the most); max_lag = L (0 .. 16); `sections` None or float64[S][5], the cascade both ears run through.
    Per node and capture c:

        mag = fmax(|a|, |b|);  if onset is NONE and mag >= threshold: onset = c          float32; a NaN is no onset
        xa, xb = cascade(float64(a)), cascade(float64(b))                                one state per ear
        before the onset: pre[0] = pre[0] + xa * xa;  pre[1] = pre[1] + xb * xb
        from it on: w = bin(c - onset);  Ea[w] += xa * xa;  Eb[w] += xb * xb;  C[w][L] += xa * xb
                    for l = 1 .. L:  C[w][L + l] += ha[l] * xb;  C[w][L - l] += hb[l] * xa
        ha[l] = ha[l - 1] for l = L .. 2, ha[1] = xa, and hb alike                        every capture, before the onset too

    with bin(rel) the largest w with edges[w] <= rel, every product and sum a float64 array operation of its own.  `state`: what an
    earlier call returned (it is not modified); the series may be fed in pieces.  Returns dict(onset uint32 [...nodes], pre float64
    [2, ...nodes], bins float64 [n_bins, 2 L + 3, ...nodes] in the order Ea, Eb, C[-L] .. C[+L], history float64 [2, L, ...nodes] with
    ha[l] at [0, l - 1], filter float64 [2, S, 2, ...nodes]); with return_state also a copy of it to hand to the next call."""
    a_snaps, b_snaps = np.asarray(ear_a_snaps), np.asarray(ear_b_snaps)
    if a_snaps.dtype != np.float32 or b_snaps.dtype != np.float32 or a_snaps.shape != b_snaps.shape:
        raise ValueError("interaural_fold: the two ears' snapshots are float32 arrays of one shape")
    edges = _check_edges(edges)
    if len(edges) > MAX_BINS:
        raise ValueError("interaural_fold: 4 bins at the most")
    L = int(max_lag)
    if not 0 <= L <= MAX_LAG:
        raise ValueError("interaural_fold: max_lag is 0 .. 16")
    sections = np.zeros((0, 5)) if sections is None else np.asarray(sections, dtype=np.float64).reshape(-1, 5)
    S = sections.shape[0]
    nodes = a_snaps.shape[1:]
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), nodes)
    if not (np.isfinite(thr) & (thr >= 0)).all():
        raise ValueError("interaural_fold: thresholds are >= 0 and finite")
    if state is None:
        onset, pre = np.full(nodes, NONE, np.uint32), np.zeros((2,) + nodes)
        bins, history, z = np.zeros((len(edges), 2 * L + 3) + nodes), np.zeros((2, L) + nodes), np.zeros((2, S, 2) + nodes)
    else:
        onset, pre, bins, history, z = (np.array(state[k]) for k in KEYS)
        if bins.shape != (len(edges), 2 * L + 3) + nodes or z.shape != (2, S, 2) + nodes:
            raise ValueError("interaural_fold: the state is of another plan")
    upper = np.array(edges[1:] + [1 << 32], dtype=np.uint64)   # bin w takes edges[w] <= rel < upper[w]; the last bin is open-ended
    with np.errstate(invalid="ignore", over="ignore"):
        for j, (a, b) in enumerate(zip(a_snaps, b_snaps)):
            c = int(first_capture) + j
            if c >= NONE:
                raise ValueError("interaural_fold: captures are numbered 0 .. 2^32 - 2")
            mag = np.fmax(np.abs(a), np.abs(b))                  # (fmaxf: the other operand where one is a NaN)
            onset = np.where((onset == NONE) & (mag >= thr), np.uint32(c), onset)
            x = [a.astype(np.float64), b.astype(np.float64)]
            for ear in range(2):
                v = x[ear]
                for s, (b0, b1, b2, a1, a2) in enumerate(sections):
                    out = v * b0 + z[ear, s, 0]
                    z[ear, s, 0] = (v * b1 - a1 * out) + z[ear, s, 1]
                    z[ear, s, 1] = v * b2 - a2 * out
                    v = out
                x[ear] = v
            xa, xb = x
            heard = onset != NONE
            pre[0] = np.where(heard, pre[0], pre[0] + xa * xa)
            pre[1] = np.where(heard, pre[1], pre[1] + xb * xb)
            rel = np.where(heard, np.uint64(c) - onset.astype(np.uint64), np.uint64(0))
            for w, lo in enumerate(edges):
                mine = heard & (rel >= np.uint64(lo)) & (rel < upper[w])
                if not mine.any():
                    continue
                bins[w, 0] = np.where(mine, bins[w, 0] + xa * xa, bins[w, 0])
                bins[w, 1] = np.where(mine, bins[w, 1] + xb * xb, bins[w, 1])
                bins[w, 2 + L] = np.where(mine, bins[w, 2 + L] + xa * xb, bins[w, 2 + L])
                for l in range(1, L + 1):
                    bins[w, 2 + L + l] = np.where(mine, bins[w, 2 + L + l] + history[0, l - 1] * xb, bins[w, 2 + L + l])
                    bins[w, 2 + L - l] = np.where(mine, bins[w, 2 + L - l] + history[1, l - 1] * xa, bins[w, 2 + L - l])
            if L:
                history[:, 1:] = history[:, :-1].copy()
                history[0, 0], history[1, 0] = xa, xb
    out = dict(onset=onset, pre=pre, bins=bins, history=history, filter=z)
    if return_state:
        return out, {k: v.copy() for k, v in out.items()}
    return out


def ear_offsets(spacing, axis=(0, 1, 0), distance=0.17):
    """The two ears of a seat as offsets in mesh nodes: (ear_a, ear_b, the distance in metres they really are apart).  The vector
    `distance` metres long along `axis` is rounded to nodes component by component, and split so that ear_a = -(d // 2) and
    ear_b = ear_a + d: an odd number of nodes puts the seat's own node half a node towards ear a."""
    axis = np.asarray(axis, dtype=np.float64).reshape(3)
    norm = float(np.sqrt((axis * axis).sum()))
    if not (norm > 0.0 and math.isfinite(norm) and float(spacing) > 0.0 and float(distance) >= 0.0 and math.isfinite(float(distance))):
        raise ValueError("ear_offsets: a non-zero finite axis, a positive spacing and a distance >= 0")
    d = [int(round(float(distance) * float(u) / norm / float(spacing))) for u in axis]
    a = tuple(-(v // 2) for v in d)
    b = tuple(p + v for p, v in zip(a, d))
    return a, b, float(spacing) * math.sqrt(sum(v * v for v in d))


def max_lag(sample_rate, every=1, ms=1.0):
    """Captures that cover lags up to `ms` milliseconds in a series captured every `every` steps of a mesh sampled at `sample_rate`:
    ceil(ms rate / (1000 every)) (ISO 3382-1 takes +-1 ms).  The engine holds 16 at the most: the caller clips, or captures less often."""
    return int(math.ceil(float(ms) * 1e-3 * float(sample_rate) / int(every) - 1e-9))


def _window(bins, window):
    bins = np.asarray(bins, dtype=np.float64)
    if bins.ndim < 2 or bins.shape[1] < 3 or bins.shape[1] % 2 == 0:
        raise ValueError("bins are float64 [n_bins, 2 L + 3, ...nodes]")
    if window is None:
        picked = list(range(bins.shape[0]))
    else:
        picked = [int(window)] if np.isscalar(window) else [int(w) for w in window]
    if not picked or any(not 0 <= w < bins.shape[0] for w in picked):
        raise ValueError("window: bins of the plan, 0 .. %d" % (bins.shape[0] - 1))
    total = bins[picked[0]].copy()
    for w in picked[1:]:
        total = total + bins[w]
    return total


def iacf(bins, window=None):
    """IACF over a window of bins (one bin, a list of them, or None for all: IACC_A): C[tau] / sqrt(Ea Eb) with every sum taken over the
    window first, float64 [2 L + 1, ...nodes], tau = -L .. L along axis 0.  NaN where either energy is 0."""
    total = _window(bins, window)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.sqrt(total[0] * total[1])
        return np.where(norm > 0.0, total[2:] / norm, np.nan)


def _peak(bins, window, interpolate):
    f = np.abs(iacf(bins, window))
    L = (f.shape[0] - 1) // 2
    empty = np.isnan(f).any(axis=0)
    k = np.argmax(np.where(np.isnan(f), -1.0, f), axis=0)              # (the first of equal maxima)
    top = np.take_along_axis(f, k[None], axis=0)[0]
    lag = k.astype(np.float64) - L
    if interpolate and L >= 1:
        inner = (k >= 1) & (k <= 2 * L - 1)                                # (both neighbours are lags of the plan)
        lo = np.take_along_axis(f, np.clip(k - 1, 0, 2 * L)[None], axis=0)[0]
        hi = np.take_along_axis(f, np.clip(k + 1, 0, 2 * L)[None], axis=0)[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            curve = lo - 2.0 * top + hi
            shift = np.where(inner & (curve < 0.0), 0.5 * (lo - hi) / curve, 0.0)
            shift = np.where(np.isfinite(shift), np.clip(shift, -0.5, 0.5), 0.0)
            top = np.where(shift != 0.0, top - 0.25 * (lo - hi) * shift, top)
        lag = lag + shift
    return np.where(empty, np.nan, top), np.where(empty, np.nan, lag)


def iacc(bins, window=None, interpolate=True):
    """IACC over a window of bins: the maximum of |IACF| over the lags, [...nodes].  `interpolate`: the vertex of the parabola through
    the largest sample and its two neighbours, where it has both and they lie below it.  NaN where either energy is 0."""
    return _peak(bins, window, interpolate)[0]


def iacc_lag(bins, window=None, interpolate=True, period=None, sample_rate=None):
    """The lag of that maximum, in captures -- or, given the plan's `period` and the mesh's `sample_rate`, in milliseconds.  Positive:
    ear a earlier."""
    lag = _peak(bins, window, interpolate)[1]
    return lag if period is None or sample_rate is None else lag * (1e3 * int(period) / float(sample_rate))


def autocorrelation(bins, window=None):
    """The ear_a == ear_b form: the normalised autocorrelation of each node's signal at lags 0 .. L, float64 [L + 1, ...nodes], 1 at lag
    0 (periodicity, echo and flutter detection).  NaN where the node is silent."""
    f = iacf(bins, window)
    return f[(f.shape[0] - 1) // 2:]


def interaural_maps(out, edges, period, sample_rate, early_ms=80.0):
    """Everything at once from fetch_interaural's dict: dict(iacc_a, lag_a_ms over all bins; iacc_e, lag_e_ms over the bins ahead of
    the edge at early_ms and iacc_l, lag_l_ms from it on, where early_ms is an edge of the plan)."""
    bins = out["bins"]
    maps = dict(iacc_a=iacc(bins), lag_a_ms=iacc_lag(bins, None, True, period, sample_rate))
    edges = _check_edges(edges)
    edge = int(round(float(early_ms) * 1e-3 * float(sample_rate) / int(period)))
    if edge in edges[1:]:
        k = edges.index(edge)
        early, late = list(range(k)), list(range(k, len(edges)))
        maps.update(iacc_e=iacc(bins, early), lag_e_ms=iacc_lag(bins, early, True, period, sample_rate),
                    iacc_l=iacc(bins, late), lag_l_ms=iacc_lag(bins, late, True, period, sample_rate))
    return maps

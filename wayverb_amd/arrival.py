"""Arrival-aligned energy maps (Engine.set_arrival / fetch_arrival): when the direct sound reaches every node of a box, how loud the
strongest arrival is, and the ISO 3382 measures that count time from that arrival -- clarity C50 / C80, definition D50, centre time
Ts -- per node.  NumPy only.

arrival_fold is the DEFINITION of what the engine folds on the device (include/wayverb_amd.h, wv_set_arrival), operation by
operation: fed the snapshots of the same box and cadence it reproduces onset, peak, peak_capture, pre, moment and bins to the last
bit, in one piece or in several.  The rest turns those six arrays into acoustics.
"""
import numpy as np

NONE = 0xFFFFFFFF   # onset / peak_capture of a node that has none yet
KEYS = ("onset", "peak", "peak_capture", "pre", "moment", "bins")


def _check_edges(edges):
    edges = [int(v) for v in edges]
    if not 1 <= len(edges) <= 16 or edges[0] != 0 or any(b <= a for a, b in zip(edges, edges[1:])) or edges[-1] > NONE:
        raise ValueError("edges: 1 .. 16 integers, edges[0] == 0, strictly increasing")
    return edges


def arrival_fold(snaps, threshold, edges, state=None, first_capture=0, return_state=False):
    """The definition.  `snaps` float32 [T, ...nodes]: captures first_capture, first_capture + 1, ... of every node; `threshold` a
    scalar or a float32 array of the nodes' shape; `edges` the first relative capture of every bin.  Per node and capture c:

        a = |p|;  if a > peak: peak, peak_capture = a, c;  if onset is NONE and a >= threshold: onset = c
        sq = float64(p) * float64(p)
        before the onset: pre = pre + sq;  from it on: rel = c - onset, E[bin(rel)] = E[bin(rel)] + sq, M = M + float64(rel) * sq

    with bin(rel) the largest k with edges[k] <= rel.  `state`: what an earlier call returned (it is not modified); the series may be
    fed in pieces.  Returns dict(onset uint32, peak float32, peak_capture uint32, pre, moment float64 [...nodes], bins float64
    [n_bins, ...nodes]); with return_state also a copy of it to hand to the next call."""
    snaps = np.asarray(snaps)
    if snaps.dtype != np.float32:
        raise ValueError("arrival_fold: snapshots are float32")
    edges = _check_edges(edges)
    nodes = snaps.shape[1:]
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), nodes)
    if not (np.isfinite(thr) & (thr >= 0)).all():
        raise ValueError("arrival_fold: thresholds are >= 0 and finite")
    if state is None:
        onset, peak_capture = np.full(nodes, NONE, np.uint32), np.full(nodes, NONE, np.uint32)
        peak, pre, moment = np.zeros(nodes, np.float32), np.zeros(nodes, np.float64), np.zeros(nodes, np.float64)
        bins = np.zeros((len(edges),) + nodes, np.float64)
    else:
        onset, peak, peak_capture, pre, moment, bins = (np.array(state[k]) for k in KEYS)
        if bins.shape != (len(edges),) + nodes:
            raise ValueError("arrival_fold: the state is of another plan")
    upper = np.array(edges[1:] + [1 << 32], dtype=np.uint64)   # bin k takes edges[k] <= rel < upper[k]; the last bin is open-ended
    with np.errstate(invalid="ignore", over="ignore"):
        for j, p in enumerate(snaps):
            c = int(first_capture) + j
            if c >= NONE:
                raise ValueError("arrival_fold: captures are numbered 0 .. 2^32 - 2")
            a = np.abs(p)
            higher = a > peak                                   # strict: the first occurrence; False for a NaN
            peak = np.where(higher, a, peak)
            peak_capture = np.where(higher, np.uint32(c), peak_capture)
            onset = np.where((onset == NONE) & (a >= thr), np.uint32(c), onset)
            p = p.astype(np.float64)
            sq = p * p
            heard = onset != NONE
            pre = np.where(heard, pre, pre + sq)
            rel = np.where(heard, np.uint64(c) - onset.astype(np.uint64), np.uint64(0))
            for k, lo in enumerate(edges):
                mine = heard & (rel >= np.uint64(lo)) & (rel < upper[k])
                if mine.any():
                    bins[k] = np.where(mine, bins[k] + sq, bins[k])
            moment = np.where(heard, moment + rel.astype(np.float64) * sq, moment)
    out = dict(onset=onset, peak=peak, peak_capture=peak_capture, pre=pre, moment=moment, bins=bins)
    if return_state:
        return out, {k: v.copy() for k, v in out.items()}
    return out


def edges_from_ms(ms, period, sample_rate):
    """Bin edges in captures for bins that begin at 0 and at each of `ms` milliseconds behind a node's onset, with a capture every
    `period` steps of a mesh sampled at `sample_rate`: [0, round(ms_1 rate / (1000 period)), ...].  Two times that fall on the same
    capture, or one that falls on capture 0, cannot both be edges: ValueError."""
    ms = [ms] if np.isscalar(ms) else list(ms)
    return _check_edges([0] + [int(round(float(m) * 1e-3 * float(sample_rate) / int(period))) for m in ms])


def arrival_time(onset, first_step, period, sample_rate):
    """Seconds from step 0 to the step of each node's onset capture, (first_step + onset * period) / sample_rate; NaN where the node
    has no onset.  (For a plan run by one wv_run after another from the step it was set at: captures are then first_step, first_step
    + period, ...)"""
    onset = np.asarray(onset)
    steps = float(first_step) + onset.astype(np.float64) * float(period)
    return np.where(onset == NONE, np.nan, steps / float(sample_rate))


def _split(bins, edges, ms, period, sample_rate):
    edges = _check_edges(edges)
    bins = np.asarray(bins, dtype=np.float64)
    if bins.shape[0] != len(edges):
        raise ValueError("%d bins for %d edges" % (bins.shape[0], len(edges)))
    at = edges_from_ms([ms], period, sample_rate)[1]
    if at not in edges:
        raise ValueError("%g ms is capture %d behind the onset, which is no bin edge of this plan (%r)" % (ms, at, edges))
    k = edges.index(at)
    return bins[:k].sum(axis=0), bins[k:].sum(axis=0)


def clarity(bins, edges, ms, period=1, sample_rate=1000.0):
    """C_ms in dB per node: 10 log10(energy in [onset, onset + ms) / energy from onset + ms on); C50 for speech, C80 for music (ISO
    3382-1).  `ms` must be an edge of the plan (edges_from_ms with the same period and sample_rate; the defaults make a capture a
    millisecond).  NaN where a node has no energy at all, +inf where none is late."""
    early, late = _split(bins, edges, ms, period, sample_rate)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(early / late)


def definition(bins, edges, ms=50.0, period=1, sample_rate=1000.0):
    """D_ms per node: energy in [onset, onset + ms) / all energy from the onset on (D50; ISO 3382-1).  NaN where there is none."""
    early, late = _split(bins, edges, ms, period, sample_rate)
    with np.errstate(divide="ignore", invalid="ignore"):
        return early / (early + late)


def centre_time(moment, bins, period, sample_rate):
    """Ts in seconds per node: the first moment of the squared pressure in time counted from the node's onset, sum(t p^2) / sum(p^2),
    with t = rel * period / sample_rate (ISO 3382-1).  NaN where a node has no energy behind an onset."""
    total = np.asarray(bins, dtype=np.float64).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(moment, dtype=np.float64) / total * (float(period) / float(sample_rate))


def direct_level_db(peak):
    """20 log10(peak) per node, -inf where nothing arrived: the level of the strongest arrival, re a pressure of 1."""
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.asarray(peak, dtype=np.float64))


def arrival_maps(out, edges, first_step, period, sample_rate, early_ms=(50.0, 80.0)):
    """Everything at once from fetch_arrival's dict: dict(arrival_s, direct_db, ts_s, pre_fraction, c<ms>_db and d<ms> for every one
    of early_ms that is an edge of the plan)."""
    maps = dict(arrival_s=arrival_time(out["onset"], first_step, period, sample_rate), direct_db=direct_level_db(out["peak"]),
                ts_s=centre_time(out["moment"], out["bins"], period, sample_rate))
    total = np.asarray(out["bins"]).sum(axis=0) + out["pre"]
    with np.errstate(divide="ignore", invalid="ignore"):
        maps["pre_fraction"] = out["pre"] / total
    for ms in early_ms:
        if edges_from_ms([ms], period, sample_rate)[1] in list(edges):
            maps["c%g_db" % ms] = clarity(out["bins"], edges, ms, period, sample_rate)
            maps["d%g" % ms] = definition(out["bins"], edges, ms, period, sample_rate)
    return maps


# ---- band-limited arrival maps (Engine.set_arrival_bands / fetch_arrival_bands) ------------------------------------------------

BAND_KEYS = KEYS + ("z",)   # what banded_arrival_fold carries from call to call: the six outputs and the filter states


def _check_tail(edges, tail):
    if tail is None:
        return 0, 0, 1
    n_tail, tail_first, tail_captures = (int(v) for v in tail)
    if not 0 <= n_tail <= 4096 - len(edges) or (n_tail and (not edges[-1] < tail_first <= NONE or not 1 <= tail_captures <= NONE)):
        raise ValueError("tail: (n_tail <= 4096 - n_edges, tail_first > edges[-1], tail_captures >= 1)")
    return (n_tail, tail_first, tail_captures) if n_tail else (0, 0, 1)


def bin_first_rels(edges, tail=None):
    """The first relative capture of every bin of a banded arrival plan, n_edges + n_tail integers: the explicit edges, then
    tail_first + m * tail_captures."""
    edges = _check_edges(edges)
    n_tail, tail_first, tail_captures = _check_tail(edges, tail)
    return edges + [tail_first + m * tail_captures for m in range(n_tail)]


def banded_bin(rel, edges, tail=None):
    """bin(rel) of include/wayverb_amd.h (wv_set_arrival_bands) for an integer array rel: behind tail_first the uniform tail, its last
    bin open-ended; ahead of it the largest j with edges[j] <= rel."""
    edges = _check_edges(edges)
    n_tail, tail_first, tail_captures = _check_tail(edges, tail)
    rel = np.asarray(rel, dtype=np.uint64)
    explicit = np.searchsorted(np.array(edges, dtype=np.uint64), rel, side="right").astype(np.int64) - 1
    if not n_tail:
        return explicit
    behind = np.where(rel >= np.uint64(tail_first), rel - np.uint64(tail_first), np.uint64(0))
    return np.where(rel >= np.uint64(tail_first), len(edges) + np.minimum(behind // np.uint64(tail_captures), np.uint64(n_tail - 1)).astype(np.int64), explicit)


def banded_arrival_fold(snaps, threshold, edges, sections, tail=None, lag=0, state=None, first_capture=0, return_state=False):
    """The definition of what a banded arrival plan folds (include/wayverb_amd.h, wv_set_arrival_bands), operation by operation.
    `snaps` float32 [T, ...nodes]: captures first_capture, first_capture + 1, ...; `threshold` a scalar or a float32 array of the
    nodes' shape; `edges` the first relative capture of every explicit bin; `sections` float64[K][S][5]; `tail` None or (n_tail,
    tail_first, tail_captures); `lag` one integer or K of them.  Per node and capture c, onset and peak as arrival_fold has them (on
    float32), then per band k, on float64: x = p through the S sections in series (decay.biquad_cascade's three lines), sq = y * y,

        before the onset: pre[k] = pre[k] + sq
        from it on: d = c - onset, rel = d - lag[k] if d > lag[k] else 0, E[k][bin(rel)] += sq, M[k] = M[k] + float64(rel) * sq

    `state`: what an earlier call returned with return_state (it is not modified); the series may be fed in pieces.  Returns
    dict(onset uint32, peak float32, peak_capture uint32 [...nodes]; pre, moment float64 [K, ...nodes]; bins float64 [K, n_bins,
    ...nodes]); with return_state also the state to hand to the next call: a copy of it plus z float64 [K, S, 2, ...nodes], the
    filter memories -- which the engine's are, bit for bit."""
    snaps = np.asarray(snaps)
    if snaps.dtype != np.float32:
        raise ValueError("banded_arrival_fold: snapshots are float32")
    edges = _check_edges(edges)
    n_tail, tail_first, tail_captures = _check_tail(edges, tail)
    sections = np.asarray(sections, dtype=np.float64)
    if sections.ndim != 3 or sections.shape[2] != 5 or not 1 <= sections.shape[0] <= 8 or not 1 <= sections.shape[1] <= 4:
        raise ValueError("banded_arrival_fold: sections is float64[K <= 8][S <= 4][5]")
    K, S = sections.shape[:2]
    lags = [int(lag)] * K if np.isscalar(lag) else [int(v) for v in lag]
    if len(lags) != K or min(lags) < 0 or max(lags) > NONE:
        raise ValueError("banded_arrival_fold: one lag, or one per band, each 0 .. 2^32 - 1")
    nodes = snaps.shape[1:]
    n_bins = len(edges) + n_tail
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), nodes)
    if not (np.isfinite(thr) & (thr >= 0)).all():
        raise ValueError("banded_arrival_fold: thresholds are >= 0 and finite")
    if state is None:
        onset, peak_capture = np.full(nodes, NONE, np.uint32), np.full(nodes, NONE, np.uint32)
        peak = np.zeros(nodes, np.float32)
        pre, moment = np.zeros((K,) + nodes, np.float64), np.zeros((K,) + nodes, np.float64)
        bins = np.zeros((K, n_bins) + nodes, np.float64)
        z = np.zeros((K, S, 2) + nodes, np.float64)
    else:
        onset, peak, peak_capture, pre, moment, bins, z = (np.array(state[k]) for k in BAND_KEYS)
        if bins.shape != (K, n_bins) + nodes or z.shape != (K, S, 2) + nodes:
            raise ValueError("banded_arrival_fold: the state is of another plan")
    with np.errstate(invalid="ignore", over="ignore"):
        for j, p in enumerate(snaps):
            c = int(first_capture) + j
            if c >= NONE:
                raise ValueError("banded_arrival_fold: captures are numbered 0 .. 2^32 - 2")
            a = np.abs(p)
            higher = a > peak                                   # strict: the first occurrence; False for a NaN
            peak = np.where(higher, a, peak)
            peak_capture = np.where(higher, np.uint32(c), peak_capture)
            onset = np.where((onset == NONE) & (a >= thr), np.uint32(c), onset)
            heard = onset != NONE
            d = np.where(heard, np.uint64(c) - onset.astype(np.uint64), np.uint64(0))
            x = p.astype(np.float64)
            for k in range(K):
                v = x
                for s, (b0, b1, b2, a1, a2) in enumerate(sections[k]):
                    out = v * b0 + z[k, s, 0]
                    z[k, s, 0] = (v * b1 - a1 * out) + z[k, s, 1]
                    z[k, s, 1] = v * b2 - a2 * out
                    v = out
                sq = v * v
                pre[k] = np.where(heard, pre[k], pre[k] + sq)
                rel = np.where(d > np.uint64(lags[k]), d - np.uint64(lags[k]), np.uint64(0))
                b = banded_bin(rel, edges, tail)
                for m in np.unique(b[heard]):
                    mine = heard & (b == m)
                    bins[k, m] = np.where(mine, bins[k, m] + sq, bins[k, m])
                moment[k] = np.where(heard, moment[k] + rel.astype(np.float64) * sq, moment[k])
    out = dict(onset=onset, peak=peak, peak_capture=peak_capture, pre=pre, moment=moment, bins=bins)
    if return_state:
        carried = {k: v.copy() for k, v in out.items()}
        carried["z"] = z
        return out, carried
    return out


def band_edges(early_ms, tail_ms, tail_bin_ms, period, sample_rate):
    """(edges, tail) for Engine.set_arrival_bands: explicit bins that begin at a node's onset and at each of `early_ms` milliseconds
    behind it (edges_from_ms), then uniform bins of `tail_bin_ms` out to `tail_ms` behind the onset.  The tail begins one tail bin behind
    the last early edge, so that from that edge on the bins are all W = round(tail_bin_ms rate / (1000 period)) >= 1 captures long; the
    last bin is open-ended.  tail_ms None or not beyond the early edges: no tail, (edges, None)."""
    edges = edges_from_ms(early_ms, period, sample_rate)
    if tail_ms is None:
        return edges, None
    per_ms = 1e-3 * float(sample_rate) / int(period)
    w = max(1, int(round(float(tail_bin_ms) * per_ms)))
    tail_first = edges[-1] + w
    n_tail = min(-(-(int(round(float(tail_ms) * per_ms)) - tail_first) // w), 4096 - len(edges))
    return (edges, (n_tail, tail_first, w)) if n_tail >= 1 else (edges, None)


def group_delay(sections, hz, rate):
    """The group delay, in samples, of the cascade float64[S][5] at `hz` on a series sampled at `rate`: per section
    Re(sum k b_k e^(-ikw) / sum b_k e^(-ikw)) - the same of (1, a1, a2), summed (the derivative of the phase, exactly)."""
    w = 2.0 * np.pi * float(hz) / float(rate)
    e = np.exp(-1j * w * np.arange(3))
    total = 0.0
    for b0, b1, b2, a1, a2 in np.asarray(sections, dtype=np.float64).reshape(-1, 5):
        for poly, sign in (((b0, b1, b2), 1.0), ((1.0, a1, a2), -1.0)):
            poly = np.array(poly)
            total += sign * float(np.real((np.arange(3) * poly * e).sum() / (poly * e).sum()))
    return total


def lag_captures(sections, centre_hz, rate):
    """A band's `lag`: the cascade's group delay at the band's centre, rounded to captures (never negative).  `rate` is the rate of the
    CAPTURED series, which is what the sections were designed for."""
    return max(0, int(round(group_delay(sections, centre_hz, rate))))


def _band_split(bins, edges, ms, period, sample_rate):
    edges = _check_edges(edges)
    bins = np.asarray(bins, dtype=np.float64)
    if bins.ndim < 2 or bins.shape[1] < len(edges):
        raise ValueError("bins is float64[K, n_bins, ...nodes] with n_bins >= %d" % len(edges))
    at = edges_from_ms([ms], period, sample_rate)[1]
    if at not in edges:
        raise ValueError("%g ms is capture %d behind the onset, which is no explicit edge of this plan (%r)" % (ms, at, edges))
    k = edges.index(at)
    return bins[:, :k].sum(axis=1), bins[:, k:].sum(axis=1)


def band_clarity(bins, edges, ms, period=1, sample_rate=1000.0):
    """C_ms in dB per band and node from bins float64[K, n_bins, ...nodes] (explicit and tail bins alike): 10 log10(energy ahead of
    the edge at `ms` / energy from it on).  With a lag the window is [onset, onset + lag + ms) of the band's own output."""
    early, late = _band_split(bins, edges, ms, period, sample_rate)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(early / late)


def band_definition(bins, edges, ms=50.0, period=1, sample_rate=1000.0):
    """D_ms per band and node: energy ahead of the edge at `ms` / all energy from the onset on."""
    early, late = _band_split(bins, edges, ms, period, sample_rate)
    with np.errstate(divide="ignore", invalid="ignore"):
        return early / (early + late)


def band_centre_time(moment, bins, period, sample_rate):
    """Ts in seconds per band and node: moment[K, ...] / the band's energy from the onset on, times period / sample_rate."""
    total = np.asarray(bins, dtype=np.float64).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(moment, dtype=np.float64) / total * (float(period) / float(sample_rate))


def band_decay_maps(bins, edges, tail, period, sample_rate):
    """EDT / T20 / T30 per band and node from bins float64[K, n_bins, ...nodes]: the backward sums of explicit and tail bins are the
    Schroeder integral at the bins' first captures (the last bin is open-ended), and decay.py's regression -- the reference's -- runs on
    it with the time axis of the real edges, bin_first_rels * period steps behind the node's onset.  dict(edt_s, t20_s, t30_s, edt_r,
    t20_r, t30_r [K, ...nodes], edc_db [K, n_bins, ...nodes])."""
    from . import decay as D
    bins = np.asarray(bins, dtype=np.float64)
    times = np.array(bin_first_rels(edges, tail), dtype=np.float64) * int(period)
    if bins.ndim < 2 or bins.shape[1] != times.shape[0]:
        raise ValueError("bins is float64[K, %d, ...nodes] for these edges and this tail" % times.shape[0])
    out = {name: [] for name in ("edt_s", "t20_s", "t30_s", "edt_r", "t20_r", "t30_r", "edc_db")}
    for band in bins:
        curve = D.energy_decay_curve(band)
        for name, fn in (("edt", D.edt), ("t20", D.rt20), ("t30", D.rt30)):
            steps, r = fn(curve, times)
            out[name + "_s"].append(steps / float(sample_rate))
            out[name + "_r"].append(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["edc_db"].append(10 * np.log10(curve / curve[0]))
    return {name: np.array(v) for name, v in out.items()}

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

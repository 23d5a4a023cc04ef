"""Lateral maps (Engine.set_lateral / fetch_lateral): the early lateral energy fraction LF (J_LF, ISO 3382-1) at every node of a
box, the direction the direct sound reached it from, and a diffuseness that measures both halves of the energy density.  NumPy only.

The engine runs the reference's directional_receiver integrator (src/waveguide/src/postprocessor/directional_receiver.cpp:29-69)
at every node of a box and sums, in bins counted from the node's OWN onset, the squared pressure E, the intensity I = p v and the
symmetric second-moment tensor Q = v v^T (include/wayverb_amd.h, "lateral maps").  lateral_fold is the DEFINITION of that fold,
operation by operation: fed snapshots of the box's hull (intensity.hull_box) it reproduces onset, pre, velocity and all ten bin
planes to the last bit, in one piece or in several.  The rest turns them into acoustics: a figure-of-eight microphone along the
unit vector d hears rho c (d . v), so its energy in a bin is (rho c)^2 d^T Q d -- d is chosen AFTER the run, per seat.
"""
import numpy as np

from .arrival import NONE, _check_edges, edges_from_ms   # noqa: F401  (edges_from_ms is re-exported)
from .intensity import _shift, hull_box                   # noqa: F401  (hull_box likewise)

KEYS = ("onset", "pre", "velocity", "bins")
PLANES = ("E", "Ix", "Iy", "Iz", "Qxx", "Qyy", "Qzz", "Qxy", "Qxz", "Qyz")
MAX_BINS = 8
_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # planes 4 .. 9


def staged_planes(hull_snap, box_in_hull, spacing):
    """What a capture stages for every node taken, from one float32 hull snapshot [hz][hy][hx]: (pressure float32 [nz][ny][nx],
    g float32 [3][nz][ny][nx]) -- the intensity plan's float lines (intensity.intensity_bins), the same casts, the same association."""
    sz, sy, sx = box_in_hull
    ports = [(sz, sy, _shift(sx, -1)), (sz, sy, _shift(sx, 1)), (sz, _shift(sy, -1), sx), (sz, _shift(sy, 1), sx),
             (_shift(sz, -1), sy, sx), (_shift(sz, 1), sy, sx)]            # nx, px, ny, py, nz, pz
    pressure = hull_snap[sz, sy, sx]
    surrounding = [((hull_snap[q] - pressure).astype(np.float64) / np.float64(spacing)).astype(np.float32) for q in ports]
    return pressure, np.stack([surrounding[2 * i + 1] - surrounding[2 * i] for i in range(3)])


def lateral_fold(hull_snaps, box_in_hull, threshold, edges, spacing, sample_rate, ambient_density, state=None, first_capture=0,
                 return_state=False):
    """The definition.  hull_snaps float32 [T][hz][hy][hx]: snapshots of the hull, captures first_capture, first_capture + 1, ...;
    box_in_hull: three slices (z, y, x) with start >= 1 that pick the nodes taken (intensity.hull_box makes both); `threshold` a
    scalar or a float32 array of the box's shape; `edges` the first relative capture of every bin (8 at the most).  Per node and
    capture c:

        pressure, g = the intensity plan's float lines;  a = |pressure|;  if onset is NONE and a >= threshold: onset = c
        v[i] = v[i] - (float64(g[i]) * 0.5) / (ambient_density * sample_rate)            every capture, before the onset too
        p = float64(pressure)
        before the onset: pre = pre + p * p
        from it on: b = bin(c - onset);  E[b] += p * p;  Ii[b] += v[i] * p;  Qij[b] += v[i] * v[j]   (ij = xx, yy, zz, xy, xz, yz)

    with bin(rel) the largest b with edges[b] <= rel.  `state`: what an earlier call returned (it is not modified); the series may
    be fed in pieces.  Returns dict(onset uint32 [nz][ny][nx], pre float64 [nz][ny][nx], velocity float64 [3][nz][ny][nx], bins
    float64 [10][n_bins][nz][ny][nx] in the order of PLANES); with return_state also a copy of it to hand to the next call."""
    snaps = np.asarray(hull_snaps)
    if snaps.dtype != np.float32 or snaps.ndim != 4:
        raise ValueError("lateral_fold: hull snapshots are float32 [T][hz][hy][hx]")
    edges = _check_edges(edges)
    if len(edges) > MAX_BINS:
        raise ValueError("lateral_fold: 8 bins at the most")
    sz, sy, sx = box_in_hull
    nodes = np.empty(snaps.shape[1:], np.bool_)[sz, sy, sx].shape
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), nodes)
    if not (np.isfinite(thr) & (thr >= 0)).all():
        raise ValueError("lateral_fold: thresholds are >= 0 and finite")
    if state is None:
        onset, pre = np.full(nodes, NONE, np.uint32), np.zeros(nodes, np.float64)
        v, bins = np.zeros((3,) + nodes, np.float64), np.zeros((len(PLANES), len(edges)) + nodes, np.float64)
    else:
        onset, pre, v, bins = (np.array(state[k]) for k in KEYS)
        if bins.shape != (len(PLANES), len(edges)) + nodes or v.shape != (3,) + nodes:
            raise ValueError("lateral_fold: the state is of another plan")
    k = np.float64(ambient_density) * np.float64(sample_rate)
    upper = np.array(edges[1:] + [1 << 32], dtype=np.uint64)   # bin b takes edges[b] <= rel < upper[b]; the last bin is open-ended
    with np.errstate(invalid="ignore", over="ignore"):
        for j, snap in enumerate(snaps):
            c = int(first_capture) + j
            if c >= NONE:
                raise ValueError("lateral_fold: captures are numbered 0 .. 2^32 - 2")
            pressure, g = staged_planes(snap, box_in_hull, spacing)                  # float32
            a = np.abs(pressure)
            onset = np.where((onset == NONE) & (a >= thr), np.uint32(c), onset)
            for i in range(3):
                m = g[i].astype(np.float64) * 0.5
                v[i] = v[i] - m / k
            p = pressure.astype(np.float64)
            sq = p * p
            heard = onset != NONE
            pre = np.where(heard, pre, pre + sq)
            rel = np.where(heard, np.uint64(c) - onset.astype(np.uint64), np.uint64(0))
            terms = [sq] + [v[i] * p for i in range(3)] + [v[i] * v[jj] for i, jj in _PAIRS]
            for b, lo in enumerate(edges):
                mine = heard & (rel >= np.uint64(lo)) & (rel < upper[b])
                if mine.any():
                    # (masked assignment only: adding +0.0 elsewhere would turn a -0.0 sum into +0.0)
                    for plane, term in enumerate(terms):
                        bins[plane, b] = np.where(mine, bins[plane, b] + term, bins[plane, b])
    out = dict(onset=onset, pre=pre, velocity=v, bins=bins)
    if return_state:
        return out, {key: val.copy() for key, val in out.items()}
    return out


def _bins(out):
    bins = np.asarray(out["bins"] if isinstance(out, dict) else out, dtype=np.float64)
    if bins.shape[0] != len(PLANES):
        raise ValueError("bins are [10][n_bins][...nodes]")
    return bins


def _pick(n_bins, which):
    which = range(n_bins) if which is None else ([which] if np.isscalar(which) else list(which))
    which = [int(b) for b in which]
    if any(b < 0 or b >= n_bins for b in which):
        raise ValueError("bins are 0 .. %d" % (n_bins - 1))
    return which


def direct_direction(out):
    """The unit vector the direct sound ARRIVED FROM at every node, float64 [3][...nodes] (x, y, z): -I / |I| of bin 0, the bin that
    begins with the node's onset.  The source's position is not needed.  NaN where bin 0 holds no intensity."""
    vec = _bins(out)[1:4, 0]
    mag = np.sqrt((vec * vec).sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mag > 0, -vec / mag, np.nan)


def lateral_axis(direction, up=(0, 0, 1)):
    """The axis of a figure-of-eight microphone whose null points along `direction` ([3] or [3][...nodes]) and which lies in the
    plane perpendicular to `up`: up x direction, normalised -- a listener facing the source hears left / right along it.  NaN
    where the direction is NaN or parallel to `up`."""
    d = np.asarray(direction, dtype=np.float64)
    u = np.asarray(up, dtype=np.float64).reshape((3,) + (1,) * (d.ndim - 1))
    axis = np.stack([u[1] * d[2] - u[2] * d[1], u[2] * d[0] - u[0] * d[2], u[0] * d[1] - u[1] * d[0]])
    mag = np.sqrt((axis * axis).sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mag > 0, axis / mag, np.nan)


def _quadratic_form(q, axis):
    """d^T Q d per bin: q [6][n_bins][...nodes] = Qxx, Qyy, Qzz, Qxy, Qxz, Qyz; axis [3] or [3][...nodes] -> [n_bins][...nodes]."""
    d = np.asarray(axis, dtype=np.float64)
    if d.shape[0] != 3:
        raise ValueError("an axis is [3] or [3][...nodes]")
    if d.ndim == 1:
        d = d.reshape((3,) + (1,) * (q.ndim - 2))
    elif d.shape[1:] != q.shape[2:]:
        raise ValueError("the axis map is of another box")
    total = 0.0
    for i in range(3):
        total = total + d[i] * d[i] * q[i]
    for plane, (i, jj) in enumerate(_PAIRS[3:], start=3):
        total = total + 2.0 * (d[i] * d[jj] * q[plane])
    return total


def figure_of_eight_energy(out, axis, ambient_density, speed_of_sound):
    """Per bin and node the energy a figure-of-eight microphone along the unit vector `axis` hears, in the units of E (pressure
    squared): (rho c)^2 d^T Q d, float64 [n_bins][...nodes].  The axis is one vector [3] or a map [3][...nodes]."""
    rc = float(ambient_density) * float(speed_of_sound)
    return rc * rc * _quadratic_form(_bins(out)[4:], axis)


def lateral_fraction(out, axis, early_bins, reference_bins, ambient_density, speed_of_sound):
    """LF per node: the figure-of-eight energy along `axis` summed over `early_bins` over the omnidirectional energy E summed over
    `reference_bins` (bin numbers or lists of them).  With edges_from_ms((5, 80), ...) J_LF of ISO 3382-1 is early_bins = 1,
    reference_bins = (0, 1).  NaN where the reference holds no energy."""
    bins = _bins(out)
    n_bins = bins.shape[1]
    eight = figure_of_eight_energy(bins, axis, ambient_density, speed_of_sound)
    early = sum(eight[b] for b in _pick(n_bins, early_bins))
    reference = sum(bins[0, b] for b in _pick(n_bins, reference_bins))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(reference > 0, early / reference, np.nan)


def energy_density(out, ambient_density, speed_of_sound, which=None):
    """The summed energy density of bins `which` (None: all) per node: E / (2 rho c^2) + rho tr(Q) / 2, the potential and the
    kinetic half, both measured."""
    bins = _bins(out)
    which = _pick(bins.shape[1], which)
    rho, c = float(ambient_density), float(speed_of_sound)
    potential = sum(bins[0, b] for b in which) / (2.0 * rho * c * c)
    kinetic = rho * sum(bins[4, b] + bins[5, b] + bins[6, b] for b in which) / 2.0
    return potential + kinetic


def diffuseness(out, ambient_density, speed_of_sound, which=None):
    """1 - |sum I| / (c w) over bins `which` (None: all), per node, with w = energy_density: 0 for a plane wave, towards 1 for a
    diffuse field.  Unlike intensity.diffuseness the kinetic half of w is measured, not assumed.  NaN where w is 0."""
    bins = _bins(out)
    picked = _pick(bins.shape[1], which)
    total = sum(bins[1:4, b] for b in picked)
    mag = np.sqrt((total * total).sum(axis=0))
    w = energy_density(bins, ambient_density, speed_of_sound, picked)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(w > 0, 1.0 - mag / (float(speed_of_sound) * w), np.nan)


def fold_traffic(onset, edges, fold_captures, first_capture=0, with_map=False):
    """Bytes the engine's folds move for a run whose FINAL onsets are `onset` (uint32, NONE where a node heard none), one entry per
    fold: `fold_captures` lists how many staged captures each fold took, in order (16 each but for the last, as the engine folds
    when its stage of 16 is full and on a fetch).  Per node and fold of t captures c0 .. c1:
      - every node: 16 t of stage, the onset read (4), the three velocities read and written (48), the threshold where a map gives it (4)
      - a node with no onset up to c1: `pre` read and written (16), no bin:                       16 t + 68
      - a node whose onset lies in c0 .. c1: `pre` (16), the onset written (4), r bins (160 r):    16 t + 72 + 160 r
      - a node with its onset behind it: r bins:                                                  16 t + 52 + 160 r
    with r the number of bins the node passes through in the fold.  A model of what the kernel asks of the memory, not a measurement."""
    onset = np.asarray(onset).ravel()
    edges = np.array(_check_edges(edges), dtype=np.int64)
    heard_at = np.where(onset == NONE, np.int64(1) << 40, onset.astype(np.int64))

    def bin_of(rel):
        return np.searchsorted(edges, rel, side="right") - 1

    out, c0 = [], int(first_capture)
    for t in fold_captures:
        c1 = c0 + int(t) - 1
        behind, inside = heard_at < c0, (heard_at >= c0) & (heard_at <= c1)
        live = behind | inside
        rel_last = np.where(live, c1 - heard_at, 0)
        rel_first = np.where(behind, c0 - heard_at, 0)
        r = np.where(live, bin_of(rel_last) - bin_of(rel_first) + 1, 0)
        per_node = 16 * int(t) + 52 + (4 if with_map else 0) + 160 * r + np.where(behind, 0, 16) + np.where(inside, 4, 0)
        out.append(int(per_node.sum()))
        c0 = c1 + 1
    return out

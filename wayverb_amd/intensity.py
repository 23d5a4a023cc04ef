"""Intensity maps: the definition of wv_set_intensity's bins in NumPy, and what one reads off them.

The engine runs the reference's directional_receiver integrator (src/waveguide/src/postprocessor/directional_receiver.cpp:29-69) at
every node of a box and sums the sound intensity I = p v and the squared pressure p^2 into time bins on the device
(include/wayverb_amd.h, "intensity maps").  `intensity_bins` evaluates the same lines, operation for operation, over snapshots of
the box's HULL (the box and one node around it): the float lines on float32 arrays, the rest on float64, so bins and velocities
come out bit for bit.  `net_intensity`, `arrival_direction` and `diffuseness` turn bins into maps.
"""
import numpy as np


def hull_box(box, stride=1):
    """The hull of a plan's box at stride 1: ((x0 - 1, y0 - 1, z0 - 1), ((nx - 1) sx + 3, ...)) for box = ((x0, y0, z0), (nx, ny, nz))
    in nodes TAKEN, and the slices `box_in_hull` that pick the taken nodes out of a hull snapshot [z][y][x]."""
    origin, taken = box
    stride = (stride,) * 3 if np.isscalar(stride) else tuple(stride)
    hull = (tuple(int(o) - 1 for o in origin), tuple((int(n) - 1) * int(s) + 3 for n, s in zip(taken, stride)))
    box_in_hull = tuple(slice(1, 1 + (int(n) - 1) * int(s) + 1, int(s)) for n, s in zip(taken[::-1], stride[::-1]))   # (z, y, x)
    return hull, box_in_hull


def _shift(sl, by):
    return slice(sl.start + by, sl.stop + by, sl.step)


def intensity_bins(hull_snaps, box_in_hull, spacing, sample_rate, ambient_density, n_bins, bin_captures, velocity=None, first_capture=0,
                   return_velocity=False):
    """The definition.  hull_snaps float32[T][hz][hy][hx]: snapshots of the hull, in capture order; box_in_hull: three slices (z, y, x)
    with start >= 1 that pick the nodes taken (hull_box makes both).  Capture j (counted from first_capture) goes to bin
    min(j // bin_captures, n_bins - 1).  `velocity` float64[3][nz][ny][nx] carries the integrator's state from an earlier piece of the
    series (None: +0.0).  Returns bins float64[4][n_bins][nz][ny][nx] = Ix, Iy, Iz, E -- and the velocities with return_velocity."""
    snaps = np.asarray(hull_snaps)
    assert snaps.dtype == np.float32 and snaps.ndim == 4
    sz, sy, sx = box_in_hull
    ports = [(sz, sy, _shift(sx, -1)), (sz, sy, _shift(sx, 1)), (sz, _shift(sy, -1), sx), (sz, _shift(sy, 1), sx),
             (_shift(sz, -1), sy, sx), (_shift(sz, 1), sy, sx)]            # nx, px, ny, py, nz, pz
    shape = snaps[0][sz, sy, sx].shape
    v = np.zeros((3,) + shape) if velocity is None else np.array(velocity, dtype=np.float64)
    assert v.shape == (3,) + shape
    bins = np.zeros((4, int(n_bins)) + shape)
    k = np.float64(ambient_density) * np.float64(sample_rate)
    spacing = np.float64(spacing)
    for j, snap in enumerate(snaps):
        b = min((int(first_capture) + j) // int(bin_captures), int(n_bins) - 1)
        pressure = snap[sz, sy, sx]                                              # float32
        surrounding = [((snap[p] - pressure).astype(np.float64) / spacing).astype(np.float32) for p in ports]
        p64 = pressure.astype(np.float64)
        for a in range(3):
            g = surrounding[2 * a + 1] - surrounding[2 * a]                      # float32
            m = g.astype(np.float64) * 0.5
            v[a] = v[a] - m / k
            bins[a, b] = bins[a, b] + v[a] * p64
        bins[3, b] = bins[3, b] + p64 * p64
    return (bins, v) if return_velocity else bins


def net_intensity(bins):
    """Sum over the bins: (I float64[3][nz][ny][nx], magnitude [nz][ny][nx], unit direction [3][nz][ny][nx], NaN where |I| is 0)."""
    total = np.asarray(bins)[:3].sum(axis=1)
    mag = np.sqrt((total * total).sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        direction = np.where(mag > 0, total / mag, np.nan)
    return total, mag, direction


def arrival_direction(bins):
    """Per bin and node the unit vector the energy ARRIVES FROM (-I / |I|), float64[3][n_bins][nz][ny][nx]; NaN where |I| is 0."""
    vec = np.asarray(bins)[:3]
    mag = np.sqrt((vec * vec).sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mag > 0, -vec / mag, np.nan)


def diffuseness(bins, speed_of_sound, ambient_density, first_bin=0, last_bin=None):
    """1 - rho c |sum I| / sum E over bins [first_bin, last_bin), per node.  The far-field estimate: the energy density is taken as
    p^2 / (rho c^2) (its kinetic half assumed equal to its potential half), so a plane wave gives 0 and a diffuse field tends to 1;
    close to a source, and in the near field of a wall, it is only indicative.  NaN where sum E is 0."""
    part = np.asarray(bins)[:, first_bin:last_bin]
    total = part[:3].sum(axis=1)
    mag = np.sqrt((total * total).sum(axis=0))
    energy = part[3].sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(energy > 0, 1.0 - float(ambient_density) * float(speed_of_sound) * mag / energy, np.nan)

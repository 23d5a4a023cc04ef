"""Intensity maps, the definition on the CPU: wayverb_amd.intensity.intensity_bins against the library's host twin of the reference's
directional_receiver integrator (postprocess.directional_accumulate, already pinned to the reference), against the decay plan's
formula for E, and against itself when a series is fed in pieces.  Everything is BYTEWISE, on seeded random series."""
import numpy as np
import pytest

from helpers import numpy_bins as decay_bins
from test_receiver_arrays_host import canonical_parameters
from wayverb_amd import intensity as I
from wayverb_amd import postprocess as P

STEPS = 200


def series(valued, seed, nodes=3):
    """Per node a 7-column series (centre, then ports nx, px, ny, py, nz, pz) as neighbouring nodes of a field have them: a common
    part plus small differences, over several orders of magnitude; float32-valued, as a snapshot holds them."""
    rng = np.random.default_rng(seed)
    common = rng.uniform(-1.0, 1.0, (nodes, STEPS, 1)) * 10.0 ** rng.uniform(-6, 0, (nodes, STEPS, 1))
    p7 = common + rng.uniform(-1.0, 1.0, (nodes, STEPS, 7)) * 10.0 ** rng.uniform(-9, -1, (nodes, STEPS, 7))
    p7[:, 4, 1:] = p7[:, 4, :1]                    # no gradient
    return p7.astype(valued).astype(np.float32)


def hull_of(p7):
    """Three nodes at z = 1, 4, 7 of a hull [T][9][3][3] (a box of 1 x 1 x 3 nodes at stride 3 along z, so that no two nodes share a
    neighbour), the seven columns at the centre and at its six neighbours."""
    nodes, steps, _ = p7.shape
    hull = np.zeros((steps, 3 * nodes, 3, 3), dtype=np.float32)
    for n in range(nodes):
        z = 1 + 3 * n
        hull[:, z, 1, 1] = p7[n, :, 0]
        hull[:, z, 1, 0], hull[:, z, 1, 2] = p7[n, :, 1], p7[n, :, 2]
        hull[:, z, 0, 1], hull[:, z, 2, 1] = p7[n, :, 3], p7[n, :, 4]
        hull[:, z - 1, 1, 1], hull[:, z + 1, 1, 1] = p7[n, :, 5], p7[n, :, 6]
    _, box_in_hull = I.hull_box(((1, 1, 1), (1, 1, nodes)), (1, 1, 3))
    assert hull[0][box_in_hull].shape == (nodes, 1, 1)
    return hull, box_in_hull


@pytest.mark.parametrize("valued", [np.float32, np.float64], ids=["fp32-valued", "fp64-valued"])
@pytest.mark.parametrize("seed", [1, 2])
def test_the_definition_is_the_pinned_integrator(built_library, valued, seed):
    """Step by step, carrying the velocity: the float records (float)(v * p) recomputed from NumPy's velocities equal the library's
    records bytewise, and so do the final velocities."""
    spacing, rate, density = canonical_parameters()
    p7 = series(valued, seed)
    hull, box_in_hull = hull_of(p7)
    v = None
    records = np.zeros((3, STEPS), dtype=P.directional_output_dtype)
    for j in range(STEPS):
        bins, v = I.intensity_bins(hull[j:j + 1], box_in_hull, spacing, rate, density, 1, 1, velocity=v, first_capture=j, return_velocity=True)
        p64 = hull[j][box_in_hull].astype(np.float64)
        records["intensity"][:, j, :] = (v * p64).astype(np.float32)[:, :, 0, 0].T
        records["pressure"][:, j] = hull[j][box_in_hull][:, 0, 0]
        assert bins[:3].tobytes() == (0.0 + v * p64).tobytes()
    for n in range(3):
        velocity = np.zeros(3)
        want = P.directional_accumulate(p7[n].astype(np.float64), spacing, rate, density, velocity)
        assert records[n].tobytes() == want.tobytes()
        assert v[:, n, 0, 0].tobytes() == velocity.tobytes()
        assert np.abs(want["intensity"]).max() > 0 and np.abs(velocity).min() > 0
    # ... and the whole series at once is the same series
    bins, v_once = I.intensity_bins(hull, box_in_hull, spacing, rate, density, 1, 1, return_velocity=True)
    assert v_once.tobytes() == v.tobytes()


def random_hull(seed, shape=(37, 6, 7, 8)):
    rng = np.random.default_rng(seed)
    smooth = rng.standard_normal(shape[:1] + (1, 1, 1)) * 10.0 ** rng.integers(-20, 3, shape[:1] + (1, 1, 1))
    return (smooth * (1.0 + 1e-3 * rng.standard_normal(shape))).astype(np.float32)


@pytest.mark.parametrize("n_bins,w", [(37, 1), (7, 5), (2, 40), (1, 1), (4, 3)])
def test_the_energy_plane_is_the_decay_plans(n_bins, w):
    hull = random_hull(5)
    for stride in ((1, 1, 1), (2, 1, 3)):
        taken = tuple((e - 3) // s + 1 for e, s in zip((8, 7, 6), stride))
        _, box_in_hull = I.hull_box(((1, 1, 1), taken), stride)
        bins = I.intensity_bins(hull, box_in_hull, 0.05, 12000.0, 1.225, n_bins, w)
        snaps = hull[(slice(None),) + box_in_hull]
        assert bins.shape == (4, n_bins) + snaps.shape[1:] == (4, n_bins) + taken[::-1]
        assert bins[3].tobytes() == decay_bins(snaps, n_bins, w).tobytes() and bins[3].max() > 0
        assert all(np.abs(bins[a]).max() > 0 for a in range(3))


@pytest.mark.parametrize("cut", [1, 16, 17])
def test_a_series_fed_in_two_pieces_that_carry_the_velocity(cut):
    """Every capture a bin of its own: the two pieces' bins, side by side, are the unsplit bins bytewise, and the velocities agree.
    With five captures per bin every bin that lies in one piece is that piece's, and the other piece left it at +0.0."""
    hull = random_hull(7)
    _, box_in_hull = I.hull_box(((1, 1, 1), (6, 5, 4)))
    for n_bins, w in ((37, 1), (7, 5)):
        args = (box_in_hull, 0.05, 12000.0, 1.225, n_bins, w)
        whole, v_whole = I.intensity_bins(hull, *args, return_velocity=True)
        first, v = I.intensity_bins(hull[:cut], *args, return_velocity=True)
        second, v = I.intensity_bins(hull[cut:], *args, velocity=v, first_capture=cut, return_velocity=True)
        assert v.tobytes() == v_whole.tobytes() and np.abs(v).min() > 0
        lo, hi = (cut - 1) // w, cut // w          # the last bin the first piece reaches, the first bin the second piece reaches
        assert whole[:, :lo].tobytes() == first[:, :lo].tobytes() and whole[:, hi + 1:].tobytes() == second[:, hi + 1:].tobytes()
        assert (first[:, lo + 1:] == 0).all() and (second[:, :hi] == 0).all()
        if w == 1:
            assert np.concatenate([first[:, :cut], second[:, cut:]], axis=1).tobytes() == whole.tobytes()
        assert all(np.abs(whole[a]).max() > 0 for a in range(4))
        # (without the carried velocity the second piece is another series)
        assert I.intensity_bins(hull[cut:], *args, first_capture=cut)[:3].tobytes() != second[:3].tobytes()


def test_maps_read_off_the_bins():
    """A plane wave along +x in the far-field normalisation (I = E / (rho c)) has diffuseness 0 and arrives from -x; opposed waves of
    equal energy cancel in I and give 1; where nothing arrived the maps say NaN, not a direction."""
    rho, c = 1.225, 340.0
    bins = np.zeros((4, 3, 1, 2, 2))
    bins[3, :, 0, 0, :] = [[2.0, 2.0], [1.0, 1.0], [0.5, 0.5]]
    bins[0, :, 0, 0, 0] = bins[3, :, 0, 0, 0] / (rho * c)                 # node (0, 0): one plane wave
    bins[0, :, 0, 0, 1] = [2.0 / (rho * c), -1.0 / (rho * c), -1.0 / (rho * c)]   # node (0, 1): opposed, net 0
    total, mag, direction = I.net_intensity(bins)
    assert total.shape == (3, 1, 2, 2) and mag.shape == (1, 2, 2) and direction.shape == (3, 1, 2, 2)
    assert direction[:, 0, 0, 0].tolist() == [1.0, 0.0, 0.0] and np.isnan(direction[:, 0, 1, 0]).all()
    arrival = I.arrival_direction(bins)
    assert arrival.shape == (3, 3, 1, 2, 2) and arrival[:, 1, 0, 0, 0].tolist() == [-1.0, 0.0, 0.0]
    assert arrival[0, :, 0, 0, 1].tolist() == [-1.0, 1.0, 1.0] and np.isnan(arrival[:, :, 0, 1, :]).all()
    d = I.diffuseness(bins, c, rho)
    assert d.shape == (1, 2, 2) and abs(d[0, 0, 0]) < 1e-15 and abs(d[0, 0, 1] - 1.0) < 1e-15 and np.isnan(d[0, 1]).all()
    assert abs(I.diffuseness(bins, c, rho, first_bin=1)[0, 0, 1] - (1.0 - 2.0 / 1.5)) < 1e-15   # a bin range of its own

"""wayverb_amd/interaural.py on the CPU, against closed forms: an integer delay gives its lag and IACC = 1; a fractional delay of a
Gaussian pulse is recovered by the parabola through the peak; independent noise stays under a 1 / sqrt N bound; equal ears give a
symmetric correlation, bitwise; the definition fed in pieces is the definition fed at once."""
import numpy as np
import pytest

from wayverb_amd import interaural as IA

L = 8


def fold(a, b, edges=(0,), lag=L, threshold=0.0, **more):
    a, b = np.asarray(a, np.float32).reshape(len(a), -1), np.asarray(b, np.float32).reshape(len(b), -1)
    return IA.interaural_fold(a, b, threshold, list(edges), lag, **more)


@pytest.mark.parametrize("m", range(0, L + 1))
def test_an_integer_delay_is_the_peak_lag_and_iacc_is_one(m):
    """b is a copy of a, m <= L captures late, the pulse (and its copy) wholly inside one bin: the peak is at lag exactly +m -- a
    earlier -- and IACC = 1 to 1e-12; with the ears exchanged the lag is -m."""
    rng = np.random.default_rng(m)
    pulse = rng.standard_normal(20)
    a, b = np.zeros(64), np.zeros(64)
    a[10:30], b[10 + m:30 + m] = pulse, pulse
    a[0] = b[0] = 1e-3                                   # (the onset of the seat: capture 0)
    for x, y, sign in ((a, b, 1), (b, a, -1)):
        out = fold(x, y, edges=(0, 5, 50))               # bin 1 holds captures 5 .. 49: all of both pulses
        for interpolate in (False, True):
            assert abs(IA.iacc(out["bins"], 1, interpolate)[0] - 1.0) <= 1e-12
            assert IA.iacc_lag(out["bins"], 1, interpolate)[0] == sign * m
        assert IA.iacc_lag(out["bins"], 1, False, period=2, sample_rate=8000.0)[0] == sign * m * 0.25     # in milliseconds
        f = IA.iacf(out["bins"], 1)
        assert f.shape == (2 * L + 1, 1) and np.nanmax(np.abs(f)) <= 1.0 + 1e-12
    silent = fold(np.zeros(8), np.zeros(8))
    assert np.isnan(IA.iacc(silent["bins"])[0]) and np.isnan(IA.iacc_lag(silent["bins"])[0]) and np.isnan(IA.iacf(silent["bins"])).all()


FRACTIONAL_BOUND = 0.0054   # captures: twice the 0.0027 measured on the CPU at the worst of the delays below (d = 1.3; sigma = 3 captures)


def test_a_fractional_delay_of_a_gaussian_pulse_is_recovered_by_the_parabola():
    """a(t) = exp(-(t - 30)^2 / 2 sigma^2), b(t) = a(t - d) evaluated analytically, sigma = 3 captures: the correlation of two Gaussians
    is a Gaussian of width sigma sqrt 2 about d, and the parabola through the three samples about its peak finds d to within
    FRACTIONAL_BOUND captures (the parabola's own error on a Gaussian that wide; float32 samples add 1e-7)."""
    t = np.arange(80, dtype=np.float64)
    worst = 0.0
    for d in (0.0, 0.25, 0.5, 1.3, 2.5, 3.75, -0.4, -2.2, 5.49, -6.5):
        a = np.exp(-0.5 * ((t - 30.0) / 3.0) ** 2)
        b = np.exp(-0.5 * ((t - 30.0 - d) / 3.0) ** 2)
        out = fold(a, b)
        got = IA.iacc_lag(out["bins"], None, True)[0]
        worst = max(worst, abs(got - d))
        assert abs(got - d) <= FRACTIONAL_BOUND, (d, got)
        assert abs(IA.iacc_lag(out["bins"], None, False)[0] - d) <= 0.5 + 1e-9
        assert 0.99 <= IA.iacc(out["bins"], None, True)[0] <= 1.0 + 1e-3
    print("worst error of the interpolated lag: %.4f captures" % worst)
    assert worst >= FRACTIONAL_BOUND / 8        # (the bound is of the error's order, not a blank cheque)


NOISE_N, NOISE_SEED = 4096, 5


def test_independent_noise_stays_under_the_one_over_root_n_bound():
    """Two independent series of N = 4096 unit normal samples: every IACF(tau) is near N(0, 1 / N), so the largest of the 2 L + 1 = 17
    lags stays under 4 / sqrt N = 0.0625 with a probability above 0.998; this seed's twin gives
    0.027 (seeds 0 .. 7: 0.026 .. 0.039).  (The seed was chosen so; the bound was not.)"""
    rng = np.random.default_rng(NOISE_SEED)
    a, b = rng.standard_normal(NOISE_N), rng.standard_normal(NOISE_N)
    out = fold(a, b)
    for interpolate in (False, True):
        got = IA.iacc(out["bins"], None, interpolate)[0]
        print("IACC of independent noise: %.4f" % got)
        assert 0.0 < got < 4.0 / np.sqrt(NOISE_N)
    assert abs(IA.iacc(fold(a, a)["bins"], None, False)[0] - 1.0) <= 1e-12 and IA.iacc_lag(fold(a, a)["bins"])[0] == 0


def test_equal_ears_give_a_symmetric_correlation_bitwise():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((50, 7)).astype(np.float32)
    sections = np.array([[0.2, 0.1, -0.3, -0.5, 0.25], [1.0, -2.0, 1.0, -1.2, 0.5]])
    out = IA.interaural_fold(a, a, np.float32(0.5), [0, 4, 9], L, sections)
    bins = out["bins"]
    assert bins[:, 0].tobytes() == bins[:, 1].tobytes() == bins[:, 2 + L].tobytes() and np.abs(bins).max() > 0
    for l in range(1, L + 1):
        assert bins[:, 2 + L + l].tobytes() == bins[:, 2 + L - l].tobytes()
    auto = IA.autocorrelation(bins)
    assert auto.shape == (L + 1, 7) and (np.abs(auto[0] - 1.0) <= 1e-12).all()
    assert out["pre"][0].tobytes() == out["pre"][1].tobytes()


def test_the_definition_in_pieces_is_the_definition_at_once():
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((45, 3, 5)).astype(np.float32), rng.standard_normal((45, 3, 5)).astype(np.float32)
    thr = np.abs(a[rng.integers(0, 45, (3, 5)), np.arange(3)[:, None], np.arange(5)[None]])
    sections = np.array([[0.2, 0.1, -0.3, -0.5, 0.25]])
    whole = IA.interaural_fold(a, b, thr, [0, 2, 7, 30], 5, sections)
    state, at = None, 0
    for n in (1, 16, 3, 25):
        piece, state = IA.interaural_fold(a[at:at + n], b[at:at + n], thr, [0, 2, 7, 30], 5, sections, state=state, first_capture=at, return_state=True)
        at += n
    for key in IA.KEYS:
        assert piece[key].tobytes() == whole[key].tobytes(), key
    assert whole["history"][0, 0].tobytes() != whole["history"][0, 1].tobytes() and len(set(whole["onset"].reshape(-1).tolist())) >= 3
    with pytest.raises(ValueError, match="4 bins at the most"):
        IA.interaural_fold(a, b, 0.0, [0, 1, 2, 3, 4], 5)
    with pytest.raises(ValueError, match="max_lag is 0 .. 16"):
        IA.interaural_fold(a, b, 0.0, [0], 17)


def test_ear_offsets_and_max_lag():
    assert IA.ear_offsets(0.05, (0, 1, 0), 0.17) == ((0, -1, 0), (0, 2, 0), pytest.approx(0.15))          # 3.4 nodes -> 3
    assert IA.ear_offsets(0.0425, (0, 1, 0), 0.17) == ((0, -2, 0), (0, 2, 0), pytest.approx(0.17))
    assert IA.ear_offsets(0.05, (1, 0, 0), 0.2) == ((-2, 0, 0), (2, 0, 0), pytest.approx(0.2))
    assert IA.ear_offsets(0.05, (0, 0, -3), 0.1) == ((0, 0, 1), (0, 0, -1), pytest.approx(0.1))
    assert IA.ear_offsets(0.05, (1, 1, 0), 0.2)[:2] == ((-1, -1, 0), (2, 2, 0))                            # 2.83 nodes each -> 3
    assert IA.ear_offsets(0.05, (0, 1, 0), 0.0) == ((0, 0, 0), (0, 0, 0), 0.0)                             # the autocorrelation form
    with pytest.raises(ValueError):
        IA.ear_offsets(0.05, (0, 0, 0), 0.17)
    assert IA.max_lag(8000.0, 1, 1.0) == 8 and IA.max_lag(8000.0, 2, 1.0) == 4 and IA.max_lag(8000.0, 3, 1.0) == 3 and IA.max_lag(44100.0, 1, 1.0) == 45
    assert IA.max_lag(8000.0, 1, 0.0) == 0

"""Band-limited arrival maps, host side (no GPU): arrival_bands_fold_kernel's text (wayverb_amd/csrc/arrival_bands_kernels.hip.h) compiled
for the host and run lane by lane, band after band, fold after fold, against the NumPy definition arrival.banded_arrival_fold, bytewise
on all six outputs and the filter states; the same program once under AddressSanitizer and UndefinedBehaviorSanitizer (its own main,
nothing loaded into python); the two identities of the definition (identity sections -> arrival_fold, threshold 0 -> banded_bins);
lag_captures against a measured phase slope; band_decay_maps on an exponential decay."""
import os
import struct
import subprocess

import numpy as np
import pytest

from plan_cases import random_sections
from test_arrival_host import NAN_CAPTURE, T, THRESHOLD, series
from wayverb_amd import arrival as A
from wayverb_amd import decay as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "arrival_bands_kernel_host.cpp")
COMPILE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", CSRC, SOURCE]
IDENTITY = np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]]])


def run_host(exe, tmp_path, snaps, edges, sections, tail, lags, threshold, threshold_map, first_fold):
    nodes, (K, S) = snaps.shape[1], sections.shape[:2]
    n_tail, tail_first, tail_captures = tail if tail else (0, 0, 1)
    n_bins = len(edges) + n_tail
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6Q28If", nodes, K, S, snaps.shape[0], first_fold, int(threshold_map is not None),
                            *(list(edges) + [0xDEADBEEF] * (16 - len(edges)) + [len(edges), n_tail, tail_first, tail_captures] +
                              list(lags) + [0xDEADBEEF] * (8 - len(lags))), threshold))   # (entries behind n_edges / K are not looked at)
        f.write(np.ascontiguousarray(sections, np.float64).tobytes())
        if threshold_map is not None:
            f.write(np.asarray(threshold_map, np.float32).tobytes())
        f.write(snaps.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=300)
    raw = open(fout, "rb").read()
    assert len(raw) == nodes * (8 * K * (2 + n_bins) + 4 * K + 8 + 16 * K * S)
    d = nodes * 8 * K
    o = d * (2 + n_bins)
    q = o + nodes * 4 * K
    return dict(pre=np.frombuffer(raw[:d]).reshape(K, nodes), moment=np.frombuffer(raw[d:2 * d]).reshape(K, nodes),
                bins=np.frombuffer(raw[2 * d:o]).reshape(K, n_bins, nodes), onset=np.frombuffer(raw[o:o + nodes * 4], np.uint32),
                peak=np.frombuffer(raw[q:q + nodes * 4], np.float32), peak_capture=np.frombuffer(raw[q + nodes * 4:q + nodes * 8], np.uint32),
                z=np.frombuffer(raw[q + nodes * 8:]).reshape(K, S, 2, nodes))


@pytest.fixture(scope="module")
def kernel_host():
    exe = os.path.join(ROOT, "tests", "cpp", "arrival_bands_kernel_host")
    subprocess.check_call(COMPILE + ["-O2", "-o", exe])
    return exe


EDGES = {"five": (0, 1, 5, 16, 17), "one": (0,), "sixteen": tuple(range(0, 32, 2)), "clarity": (0, 6, 10)}
TAILS = {"none": None, "w3": (4, 19, 3), "w1": (20, 18, 1), "inside": (3, 20, 7), "decay": (8, 3, 3), "long": (2, 40, 100)}
# (B, shift of the kinds, first fold, edges, tail, lags, K, S, a per-node map?): test_arrival_host.series puts onsets on capture 0, on the
# last slot of a fold (15), the first of the next (16), on 12 / 13 around a short first fold, on 31, nowhere, and a NaN at capture 20.
# "w3" from onset 0 fills tail bins 19 .. 27, 28 .. and goes open-ended at 28 with 17 captures to come; "w1" moves on at every capture;
# "inside" begins inside a fold for every built onset; "long" is never left; "decay" is the threshold-0 shape; lags 2 and 20 hold rel
# at 0 across a fold boundary
CASES = [(1, s, 16, "five", "w3", (0,), 1, 1 + s % 4, False) for s in range(8)] + \
        [(1, 1, 13, "five", "none", (2,), 1, 2, True), (1, 6, 16, "one", "w1", (0, 20), 2, 3, False),
         (63, 0, 16, "five", "w3", (0, 2, 20), 3, 4, False), (255, 0, 16, "five", "inside", (1,) * 8, 8, 1, False),
         (256, 1, 13, "five", "w3", (20, 2), 2, 2, False), (257, 2, 16, "five", "w1", (0, 2, 20), 3, 3, True),
         (257, 3, 13, "sixteen", "none", (3,), 1, 4, False), (256, 4, 16, "one", "decay", (0, 0), 2, 4, True),
         (255, 5, 13, "clarity", "long", (2, 0), 2, 1, True), (630, 6, 1, "five", "w3", (0, 1, 2, 3, 5, 8, 13, 21), 8, 2, False),
         (300, 7, 16, "clarity", "w3", (20, 0), 2, 3, False)]


def case_id(c):
    return "B%d-shift%d-first%d-%s-%s-K%dS%d%s" % (c[:5] + c[6:8] + ("-map" if c[8] else "",))


@pytest.mark.parametrize("nodes,shift,first_fold,edges,tail,lags,K,S,with_map", CASES, ids=[case_id(c) for c in CASES])
def test_the_kernels_text_on_the_host_reproduces_the_definition_bytewise(kernel_host, tmp_path, nodes, shift, first_fold, edges, tail, lags, K, S, with_map):
    snaps, wanted = series(nodes, shift, 100 * nodes + shift)
    sections = random_sections(K, S, nodes + 31 * shift)
    threshold_map = None
    if with_map:
        rng = np.random.default_rng(nodes + 7)
        threshold_map = np.where([w is None for w in wanted], 10.0 ** rng.uniform(-6, 6, nodes), THRESHOLD).astype(np.float32)
    got = run_host(kernel_host, tmp_path, snaps, EDGES[edges], sections, TAILS[tail], lags, 123.0 if with_map else THRESHOLD, threshold_map, first_fold)
    want, state = A.banded_arrival_fold(snaps, threshold_map if with_map else THRESHOLD, EDGES[edges], sections, tail=TAILS[tail], lag=lags,
                                        return_state=True)
    for i, at in enumerate(wanted):
        if at is not None:
            assert want["onset"][i] == (A.NONE if at == T else at), (i, at)
    for key in A.BAND_KEYS:
        assert got[key].dtype == state[key].dtype and got[key].tobytes() == state[key].tobytes(), key
    if nodes >= 255:
        onset = want["onset"]
        assert (onset == A.NONE).any() and (onset == 0).any() and (onset == 15).any() and (onset == 16).any() and (onset == 31).any()
        assert np.isnan(want["bins"]).any() or np.isnan(want["pre"]).any()                 # the NaN capture went somewhere ...
        assert np.isnan(state["z"]).any() and snaps[NAN_CAPTURE:].shape[0] > 0             # ... and stays in that node's filters
        quiet = onset == A.NONE
        assert (want["moment"][:, quiet] == 0).all() and (want["bins"][:, :, quiet] == 0).all() and (want["pre"][:, ~quiet & (onset == 0)] == 0).all()
        if TAILS[tail] and tail != "long":
            filled = (np.nan_to_num(want["bins"], nan=1.0) > 0).any(axis=2)
            assert filled.any(axis=0).all(), filled                                           # every explicit and every tail bin took something in the band that lags least


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (-fno-sanitize-recover: a report is a failure): B = 257
    with a map, a short first fold, three bands of four sections, lags and a tail that goes open-ended; B = 1 without a tail.  Both
    blocks, the table of the bins' first rels and every fold's stage are allocated at exactly their sizes."""
    exe = os.path.join(ROOT, "tests", "cpp", "arrival_bands_kernel_host_san")
    subprocess.check_call(COMPILE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    for nodes, shift, first_fold, with_map, tail, lags, K, S in ((257, 2, 13, True, "w3", (0, 2, 20), 3, 4), (1, 3, 16, False, "none", (0,), 1, 1)):
        snaps, wanted = series(nodes, shift, 9)
        sections = random_sections(K, S, 5)
        threshold_map = np.full(nodes, THRESHOLD, np.float32) if with_map else None
        got = run_host(exe, tmp_path, snaps, EDGES["five"], sections, TAILS[tail], lags, THRESHOLD, threshold_map, first_fold)
        want, state = A.banded_arrival_fold(snaps, THRESHOLD, EDGES["five"], sections, tail=TAILS[tail], lag=lags, return_state=True)
        for key in A.BAND_KEYS:
            assert got[key].tobytes() == state[key].tobytes(), key


def random_snaps(seed, shape=(41, 3, 5)):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-12, 9, shape)).astype(np.float32)


def test_identity_sections_reproduce_the_arrival_plan():
    """One band, lag 0, no tail, the section b0 = 1, b1 = b2 = a1 = a2 = 0: y == x (x * 1 + 0 is x; the memories stay +0.0 or -0.0,
    and adding either to x * 1 gives x), so all six outputs are arrival_fold's, bytewise."""
    snaps = random_snaps(1)
    thr = np.float32(10.0) ** np.random.default_rng(2).integers(-3, 12, snaps.shape[1:]).astype(np.float32)
    for edges in ((0, 1, 5, 16, 17), (0,), (0, 6, 10)):
        want = A.arrival_fold(snaps, thr, edges)
        got = A.banded_arrival_fold(snaps, thr, edges, IDENTITY)
        for key in ("onset", "peak", "peak_capture"):
            assert got[key].tobytes() == want[key].tobytes(), key
        for key in ("pre", "moment", "bins"):
            assert got[key][0].tobytes() == want[key].tobytes(), key
    assert (want["onset"] == A.NONE).any() and (want["onset"] != A.NONE).any()


@pytest.mark.parametrize("n_bins,w", [(16, 1), (7, 5), (2, 40), (1, 1), (4, 3)])
def test_threshold_zero_reproduces_the_banded_decay_plan(n_bins, w):
    """Threshold 0, n_edges = 1, tail_first = tail_captures = W, n_tail = n - 1: every onset is capture 0 and the bins and the filter
    states are decay.banded_bins' with bin_captures = W, n_bins = n, bytewise."""
    snaps = random_snaps(5)
    sections = random_sections(3, 2, 11)
    got, state = A.banded_arrival_fold(snaps, 0.0, (0,), sections, tail=(n_bins - 1, w, w) if n_bins > 1 else None, return_state=True)
    want, z = D.banded_bins(snaps, sections, n_bins, w, return_state=True)
    assert got["bins"].tobytes() == want.tobytes() and want.max() > 0 and state["z"].tobytes() == z.tobytes()
    assert (got["onset"] == 0).all() and not got["pre"].any() and not np.signbit(got["pre"]).any()


def test_a_series_fed_in_pieces_equals_the_series_fed_at_once():
    snaps = random_snaps(3)
    thr = np.float32(10.0) ** np.random.default_rng(4).integers(-3, 12, snaps.shape[1:]).astype(np.float32)
    sections = random_sections(2, 3, 6)
    args = dict(tail=(4, 19, 3), lag=(2, 20))
    whole, whole_state = A.banded_arrival_fold(snaps, thr, (0, 1, 5, 16, 17), sections, return_state=True, **args)
    for cuts in ((13,), (1, 2, 40), (16, 32), tuple(range(1, 41))):
        state, first = None, 0
        for end in cuts + (41,):
            out, state = A.banded_arrival_fold(snaps[first:end], thr, (0, 1, 5, 16, 17), sections, state=state, first_capture=first, return_state=True, **args)
            first = end
        for key in A.BAND_KEYS:
            assert state[key].tobytes() == whole_state[key].tobytes(), (cuts, key)
    before = {k: v.copy() for k, v in state.items()}
    A.banded_arrival_fold(snaps[:3], thr, (0, 1, 5, 16, 17), sections, state=state, first_capture=41, **args)
    assert all(state[k].tobytes() == before[k].tobytes() for k in A.BAND_KEYS)        # the state handed in is not modified


def test_the_lag_keeps_the_direct_sound_in_bin_zero():
    """One node, onset at capture 3, identity section: with lag 4 the captures 3 .. 7 have rel 0 (d = 0 .. 4), capture 8 has rel 1; the
    moment counts from there.  A lag larger than every d keeps everything in bin 0 and the moment at +0.0."""
    snaps = np.zeros((12, 1), np.float32)
    snaps[3:] = 2.0
    out = A.banded_arrival_fold(snaps, 1.0, (0, 1, 3), np.repeat(IDENTITY, 3, axis=0), lag=(0, 4, 100))
    assert out["onset"][0] == 3 and list(out["bins"][0, :, 0]) == [4.0, 8.0, 24.0] and list(out["bins"][1, :, 0]) == [20.0, 8.0, 8.0]
    assert list(out["bins"][2, :, 0]) == [36.0, 0.0, 0.0] and list(out["moment"][:, 0]) == [4.0 * 36, 4.0 * 10, 0.0]
    assert A.banded_bin([0, 18, 19, 21, 22, 27, 28, 1000, 2 ** 32 - 2], (0, 1, 5, 16, 17), (4, 19, 3)).tolist() == [0, 4, 5, 5, 6, 7, 8, 8, 8]


def test_lag_captures_is_the_measured_phase_slope_of_the_butterworth_bandpass(built_library):
    """The reference-pinned Butterworth band-pass of the 500 Hz octave at 8 kHz (decay.butterworth_bandpass): wv_biquad_run's response
    to an impulse, 16384 samples long (the poles' radius is below 0.9: what is cut off is far below one ulp), its FFT, and the
    central difference of the unwrapped phase across the two bins around the centre frequency.  The difference quotient is off from
    the derivative by (dw^2 / 6) |tau''| with dw = 2 pi / 16384 = 3.8e-4 rad; tau is about 15 samples over a band 0.28 rad wide, so
    tau'' is of the order tau / 0.28^2 = 200 and the error of the order 5e-6 samples; the bound is 1e-4.  lag_captures rounds it."""
    lo, hi = D.octave_band_edges([500.0])[0]
    sections = D.butterworth_bandpass(lo, hi, 8000.0)
    n = 16384
    impulse = np.zeros(n)
    impulse[0] = 1.0
    h = D.biquad_run(sections, impulse)
    assert abs(h[-64:]).max() < 1e-16 * abs(h).max()
    phase = np.unwrap(np.angle(np.fft.rfft(h)))
    k = int(round(500.0 / 8000.0 * n))
    measured = -(phase[k + 1] - phase[k - 1]) / (2 * 2 * np.pi / n)
    tau = A.group_delay(sections, k * 8000.0 / n, 8000.0)
    assert abs(tau - measured) < 1e-4, (tau, measured)
    assert 5 < tau < 40 and A.lag_captures(sections, k * 8000.0 / n, 8000.0) == int(round(measured))
    assert A.lag_captures(IDENTITY[0], 500.0, 8000.0) == 0


def test_band_decay_maps_recovers_the_decay_constant_of_an_exponential():
    """p_j = r^j from the onset at capture 0 with r = 10^(-60 / (20 T60)), T60 = 4000 captures, 8000 captures long (120 dB), identity
    section, edges (0, 50, 80) and a tail of 20-capture bins: the Schroeder curve at the bins' first captures is r^(2 t) (1 - r^(2 (8000
    - t))) / (1 - r^2).  What is cut off at capture 8000 lowers the curve at -35 dB (t = 2333) by the factor 1 - 10^(-8.5): 1.4e-8 dB.
    The regression takes levels and times as float32 (relative 6e-8: 2e-6 dB at -35 dB, times exact below 2^24) and p is float32
    (relative 6e-8 per square, 5e-7 dB).  A line through points that are off by less than 3e-6 dB over a span of 30 dB has a slope
    within 2 * 3e-6 / 30 = 2e-7 relative: T30 within 1e-6 relative of 4000 captures, T20 and EDT likewise over their 20 and 10 dB
    (3e-7, 6e-7); the bound for all three is 2e-6."""
    t60 = 4000.0
    r = 10.0 ** (-60.0 / (20.0 * t60))
    snaps = (r ** np.arange(8000, dtype=np.float64)).astype(np.float32).reshape(-1, 1)
    edges, tail = A.band_edges((50, 80), 7000, 20, 1, 1000.0)
    assert edges == [0, 50, 80] and tail == (345, 100, 20)
    out = A.banded_arrival_fold(snaps, 0.5, edges, IDENTITY, tail=tail)
    assert out["onset"][0] == 0 and out["bins"].shape == (1, 348, 1)
    maps = A.band_decay_maps(out["bins"], edges, tail, 1, 1000.0)
    for name in ("edt_s", "t20_s", "t30_s"):
        assert abs(maps[name][0, 0] * 1000.0 / t60 - 1.0) < 2e-6, (name, maps[name])
        assert maps[name.replace("_s", "_r")][0, 0] < -0.999999
    # C50 of the same decay: 10 log10((1 - r^100) / r^100) but for the 8000-capture cut (a factor 1 - 10^-11.85)
    want = 10 * np.log10((1 - r ** 100) / r ** 100)
    assert abs(A.band_clarity(out["bins"], edges, 50)[0, 0] - want) < 1e-5
    assert abs(A.band_definition(out["bins"], edges, 50)[0, 0] - (1 - r ** 100)) < 1e-6
    # Ts = sum t r^2t / sum r^2t = r^2 / (1 - r^2) captures, in seconds at a capture per millisecond
    assert abs(A.band_centre_time(out["moment"], out["bins"], 1, 1000.0)[0, 0] / (r * r / (1 - r * r) * 1e-3) - 1) < 1e-5

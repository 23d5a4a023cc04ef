"""Arrival-aligned energy maps, host side (no GPU): arrival_fold_kernel's text (wayverb_amd/csrc/arrival_kernels.hip.h) compiled for
the host and run lane by lane, fold after fold, against the NumPy definition arrival.arrival_fold, bytewise on all six outputs; the
same program once under AddressSanitizer and UndefinedBehaviorSanitizer (its own main, nothing loaded into python); and identities
of the definition itself."""
import os
import struct
import subprocess

import numpy as np
import pytest

from wayverb_amd import arrival as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "arrival_kernel_host.cpp")
COMPILE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", CSRC, SOURCE]

T = 45                  # captures: 16 + 16 + 13, or 13 + 16 + 16 with a short first fold
THRESHOLD = 1.0
NAN_CAPTURE = 20


def series(nodes, shift, seed):
    """float32 [T, nodes] spanning 20 orders of magnitude (1e-12 .. 1e8), and the onset each node was built to have against a threshold
    of 1 (None: whatever the random series gives).  Node i is of kind (i + shift) % 8:
      0  never reaches the threshold           4  onset 12 / 13: last slot of a short first fold of 13, first slot of the next
      1  onset at capture 0                    5  as the random numbers fall
      2  onset 15: the last slot of a fold     6  as they fall, and a NaN at capture 20
      3  onset 16: the first slot of a fold    7  onset 31; with edges (0, 1, 5, 16, 17) kind 2's edges 16 and 17 fall into captures 31
                                                  and 32: an onset and a bin edge in different folds, and two edges across a fold's end"""
    rng = np.random.default_rng(seed)
    snaps = (rng.standard_normal((T, nodes)) * 10.0 ** rng.integers(-12, 9, (T, nodes))).astype(np.float32)
    wanted = []
    for i in range(nodes):
        kind = (i + shift) % 8
        at = {0: T, 1: 0, 2: 15, 3: 16, 4: 12 + (i // 8) % 2, 7: 31}.get(kind)
        if at is not None:
            quiet = snaps[:at, i]
            loud = np.abs(quiet) >= THRESHOLD
            quiet[loud] = quiet[loud] / np.abs(quiet[loud]) * np.float32(0.999)     # (still 20 orders below: the small ones stay)
            if at < T:
                snaps[at, i] = np.float32(1.0) if i % 3 == 0 else np.float32(-37.5)  # exactly the threshold counts (>=)
        if kind == 6:
            snaps[NAN_CAPTURE, i] = np.nan
        wanted.append(at)
    return snaps, wanted


def run_host(exe, tmp_path, snaps, edges, threshold, threshold_map, first_fold):
    nodes, n_bins = snaps.shape[1], len(edges)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<5Q16If", nodes, n_bins, snaps.shape[0], first_fold, int(threshold_map is not None),
                            *(list(edges) + [0xDEADBEEF] * (16 - n_bins)), threshold))   # (the entries behind n_bins are not looked at)
        if threshold_map is not None:
            f.write(np.asarray(threshold_map, np.float32).tobytes())
        f.write(snaps.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=300)
    raw = open(fout, "rb").read()
    assert len(raw) == nodes * (28 + 8 * n_bins)
    d, o = nodes * 8, nodes * 8 * (2 + n_bins)
    return dict(pre=np.frombuffer(raw[:d]), moment=np.frombuffer(raw[d:2 * d]), bins=np.frombuffer(raw[2 * d:o]).reshape(n_bins, nodes),
                onset=np.frombuffer(raw[o:o + nodes * 4], np.uint32), peak=np.frombuffer(raw[o + nodes * 4:o + nodes * 8], np.float32),
                peak_capture=np.frombuffer(raw[o + nodes * 8:], np.uint32))


@pytest.fixture(scope="module")
def kernel_host():
    exe = os.path.join(ROOT, "tests", "cpp", "arrival_kernel_host")
    subprocess.check_call(COMPILE + ["-O2", "-o", exe])
    return exe


EDGES = {"five": (0, 1, 5, 16, 17), "one": (0,), "sixteen": tuple(range(0, 32, 2)), "clarity": (0, 6, 10)}
# (B, shift of the kinds, first fold, edges, a per-node map?)
CASES = [(1, s, 16, "five", False) for s in range(8)] + [(1, 2, 13, "five", True), (1, 6, 16, "one", False)] + \
        [(255, 0, 16, "five", False), (256, 1, 13, "five", False), (257, 2, 16, "five", True), (257, 3, 13, "sixteen", False),
         (256, 4, 16, "one", True), (255, 5, 13, "clarity", True), (630, 6, 1, "five", False)]


@pytest.mark.parametrize("nodes,shift,first_fold,edges,with_map", CASES, ids=["B%d-shift%d-first%d-%s%s" % (c[:4] + ("-map" if c[4] else "",)) for c in CASES])
def test_the_kernels_text_on_the_host_reproduces_the_definition_bytewise(kernel_host, tmp_path, nodes, shift, first_fold, edges, with_map):
    snaps, wanted = series(nodes, shift, 100 * nodes + shift)
    threshold_map = None
    if with_map:
        # per node 1 (the built onsets hold) or, for the kinds left to chance, anything in 1e-6 .. 1e6
        rng = np.random.default_rng(nodes + 7)
        threshold_map = np.where([w is None for w in wanted], 10.0 ** rng.uniform(-6, 6, nodes), THRESHOLD).astype(np.float32)
    got = run_host(kernel_host, tmp_path, snaps, EDGES[edges], 123.0 if with_map else THRESHOLD, threshold_map, first_fold)
    want = A.arrival_fold(snaps, threshold_map if with_map else THRESHOLD, EDGES[edges])
    # the inputs are what the docstring of series() says: the built onsets are the definition's
    for i, at in enumerate(wanted):
        if at is not None:
            assert want["onset"][i] == (A.NONE if at == T else at), (i, at)
    for key in A.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    if nodes >= 255:
        onset = want["onset"]
        assert (onset == A.NONE).any() and (onset == 0).any() and (onset == 15).any() and (onset == 16).any() and (onset == 31).any()
        assert (onset == 12).any() and (onset == 13).any()
        assert np.isnan(want["bins"]).any() or np.isnan(want["pre"]).any()                 # the NaN capture went somewhere
        assert (want["peak_capture"][onset == A.NONE] != A.NONE).all()                      # quiet nodes still have a peak
        assert np.isfinite(want["peak"]).all() and (want["pre"][onset == 0] == 0).all() and not np.signbit(want["pre"][onset == 0]).any()
        if len(EDGES[edges]) > 1:
            filled = (np.nan_to_num(want["bins"], nan=1.0) > 0).any(axis=1)
            assert filled.all(), filled                                                       # every bin took something
        quiet = onset == A.NONE
        assert (want["moment"][quiet] == 0).all() and (want["bins"][:, quiet] == 0).all()


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (-fno-sanitize-recover: a report is a failure): B = 257
    with a map and a short first fold, and B = 1.  The state block and every fold's stage are allocated at exactly their sizes."""
    exe = os.path.join(ROOT, "tests", "cpp", "arrival_kernel_host_san")
    subprocess.check_call(COMPILE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    for nodes, shift, first_fold, with_map in ((257, 2, 13, True), (1, 3, 16, False)):
        snaps, wanted = series(nodes, shift, 9)
        threshold_map = np.full(nodes, THRESHOLD, np.float32) if with_map else None
        got = run_host(exe, tmp_path, snaps, EDGES["five"], THRESHOLD, threshold_map, first_fold)
        want = A.arrival_fold(snaps, THRESHOLD, EDGES["five"])
        for key in A.KEYS:
            assert got[key].tobytes() == want[key].tobytes(), key


def random_snaps(seed, shape=(41, 3, 5)):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-12, 9, shape)).astype(np.float32)


def test_a_series_fed_in_pieces_equals_the_series_fed_at_once():
    snaps = random_snaps(1)
    thr = np.float32(10.0) ** np.random.default_rng(2).integers(-3, 12, snaps.shape[1:]).astype(np.float32)
    whole = A.arrival_fold(snaps, thr, (0, 1, 5, 16, 17))
    assert (whole["onset"] == A.NONE).any() and (whole["onset"] != A.NONE).any() and len(set(whole["onset"].ravel())) > 4
    for cuts in ((13,), (1, 2, 40), (16, 32), tuple(range(1, 41))):
        state, first = None, 0
        for end in cuts + (41,):
            out, state = A.arrival_fold(snaps[first:end], thr, (0, 1, 5, 16, 17), state=state, first_capture=first, return_state=True)
            first = end
        for key in A.KEYS:
            assert out[key].tobytes() == whole[key].tobytes(), (cuts, key)
    # the state handed in is not modified
    out, state = A.arrival_fold(snaps[:7], thr, (0, 3), return_state=True)
    before = {k: v.copy() for k, v in state.items()}
    A.arrival_fold(snaps[7:], thr, (0, 3), state=state, first_capture=7)
    assert all(state[k].tobytes() == before[k].tobytes() for k in A.KEYS)


@pytest.mark.parametrize("n_bins,w", [(16, 1), (7, 5), (2, 40), (1, 1), (4, 3)])
def test_threshold_zero_and_even_edges_are_the_decay_plans_bins(n_bins, w):
    """Every onset is capture 0, the plan degenerates to a global clock: E[min(j // W, n - 1)] += p^2, bytewise, and pre is +0.0."""
    snaps = random_snaps(5)
    out = A.arrival_fold(snaps, 0.0, [k * w for k in range(n_bins)])
    plain = np.zeros((n_bins,) + snaps.shape[1:])
    for j, p in enumerate(snaps):
        p = p.astype(np.float64)
        b = min(j // w, n_bins - 1)
        plain[b] = plain[b] + p * p
    assert out["bins"].tobytes() == plain.tobytes() and plain.max() > 0
    assert (out["onset"] == 0).all() and out["pre"].tobytes() == np.zeros(snaps.shape[1:]).tobytes()
    moment = np.zeros(snaps.shape[1:])
    for j, p in enumerate(snaps):
        moment = moment + float(j) * (p.astype(np.float64) * p.astype(np.float64))
    assert out["moment"].tobytes() == moment.tobytes()


def test_pre_and_the_bins_hold_all_the_energy():
    """pre + sum E against the plain ordered sum of p^2: 41 non-negative terms summed in another grouping, each partial sum within
    2^-53 of exact relative to the total, so |difference| <= 2 * 41 * 2^-53 of the total."""
    snaps = random_snaps(8)
    thr = np.where(np.arange(15).reshape(3, 5) % 4 == 0, 1e12, 1.0).astype(np.float32)   # every fourth node never hears an onset
    out = A.arrival_fold(snaps, thr, (0, 1, 5, 16, 17))
    total = (snaps.astype(np.float64) ** 2).sum(axis=0)
    got = out["pre"] + out["bins"].sum(axis=0)
    assert (np.abs(got - total) <= 82 * 2.0 ** -53 * total).all() and total.min() > 0
    assert (out["onset"] == A.NONE).any() and (out["pre"][out["onset"] == A.NONE] > 0).all()


def test_acoustic_measures_on_a_hand_made_decay():
    """One node: onset at capture 3, p^2 = 4 in the onset capture, then 1 per capture for 9 captures; a capture per millisecond."""
    snaps = np.zeros((13, 1), np.float32)
    snaps[1] = 0.25                       # ahead of the onset: below the threshold
    snaps[3] = -2.0
    snaps[4:] = 1.0
    edges = A.edges_from_ms((5, 8), 1, 1000.0)
    assert edges == [0, 5, 8]
    out = A.arrival_fold(snaps, 0.5, edges)
    assert out["onset"][0] == 3 and out["peak"][0] == 2.0 and out["peak_capture"][0] == 3 and out["pre"][0] == 0.0625
    assert list(out["bins"][:, 0]) == [8.0, 3.0, 2.0] and out["moment"][0] == sum(range(1, 10))
    assert A.clarity(out["bins"], edges, 5)[0] == 10 * np.log10(8.0 / 5.0)
    assert A.clarity(out["bins"], edges, 8)[0] == 10 * np.log10(11.0 / 2.0)
    assert A.definition(out["bins"], edges, 5)[0] == 8.0 / 13.0
    assert A.centre_time(out["moment"], out["bins"], 1, 1000.0)[0] == 45.0 / 13.0 * 1e-3
    assert A.arrival_time(out["onset"], 2, 3, 1000.0)[0] == 11e-3
    assert A.direct_level_db(out["peak"])[0] == 20 * np.log10(2.0)
    with pytest.raises(ValueError):
        A.clarity(out["bins"], edges, 6)          # no edge of the plan
    with pytest.raises(ValueError):
        A.edges_from_ms((5, 5.2), 1, 1000.0)       # the same capture twice
    silent = A.arrival_fold(np.zeros((4, 2), np.float32), 1e-30, edges)
    assert np.isnan(A.arrival_time(silent["onset"], 0, 1, 1000.0)).all() and np.isneginf(A.direct_level_db(silent["peak"])).all()
    assert (silent["peak_capture"] == A.NONE).all() and np.isnan(A.centre_time(silent["moment"], silent["bins"], 1, 1000.0)).all()
    maps = A.arrival_maps(out, edges, 0, 1, 1000.0, early_ms=(5, 8, 50))
    assert sorted(maps) == ["arrival_s", "c5_db", "c8_db", "d5", "d8", "direct_db", "pre_fraction", "ts_s"]

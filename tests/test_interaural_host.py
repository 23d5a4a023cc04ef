"""Interaural maps, host side (no GPU): the planning header against hand-derived cases (tests/cpp/interaural_plan_test.cpp: every
refusal and their order, sizes, places), and the text of interaural_fold_kernel and ear_gather_kernel compiled for the host against
the NumPy definition interaural.interaural_fold, byte for byte (tests/cpp/interaural_kernel_host.cpp) -- every lag class, with and
without the cascade -- and once more under the address and undefined-behaviour sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from wayverb_amd import interaural as IA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wayverb_amd", "csrc")
COMPILE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-Wno-unused-variable", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "interaural_kernel_host.cpp")]


def test_planning_header_against_hand_derived_cases():
    src = os.path.join(ROOT, "tests", "cpp", "interaural_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "interaural_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "INTERAURAL PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    header = open(os.path.join(CSRC, "interaural_plan.h")).read()
    assert "hip" not in header.split("#pragma once")[1].lower()
    assert sorted(re.findall(r"#include [<\"]([^>\"]+)[>\"]", header)) == ["../../include/wayverb_amd.h", "arrival_plan.h", "cstdint", "snapshot_plan.h"]


def series(rng, t, nodes):
    """float32 captures over 30 orders of magnitude, subnormal floats among them."""
    return (rng.standard_normal((t, nodes)) * 10.0 ** rng.integers(-44, -14, (t, nodes))).astype(np.float32)


SECTIONS = np.array([[0.2, 0.1, -0.3, -0.5, 0.25], [1.0, -2.0, 1.0, -1.2, 0.5], [0.7, 0.0, -0.7, 0.3, -0.1], [0.5, 0.5, 0.0, 0.0, 0.9]])


def run_host(exe, tmp_path, a, b, L, edges, S, threshold=0.0, first_fold=16, first_capture=0, threshold_map=None):
    t, nodes = a.shape
    e = list(edges) + [0] * (4 - len(edges))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8Q4If", nodes, L, len(edges), S, t, first_fold, first_capture, int(threshold_map is not None), *e, threshold))
        if threshold_map is not None:
            f.write(np.asarray(threshold_map, np.float32).tobytes())
        f.write(SECTIONS[:S].tobytes() + a.tobytes() + b.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=300)
    raw = open(fout, "rb").read()
    planes = 2 * L + 3
    assert len(raw) == nodes * (16 + 8 * len(edges) * planes + 4)
    pre = np.frombuffer(raw, np.float64, 2 * nodes).reshape(2, nodes)
    bins = np.frombuffer(raw, np.float64, len(edges) * planes * nodes, 16 * nodes).reshape(len(edges), planes, nodes)
    onset = np.frombuffer(raw, np.uint32, nodes, 16 * nodes + bins.nbytes)
    return dict(onset=onset, pre=pre, bins=bins)


def same(got, want, case):
    for key in ("onset", "pre", "bins"):
        assert got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), (case, key)


# (B, L, edges, S, captures, first fold, first capture): B of 1 / 255 / 256 / 257 / 630; L of 0 and at and on either side of every lag
# class and chunk; one to four bins with edges inside and between folds; 0, 1 and 4 sections; one capture, a full stage, 17 and 33
# captures (the history carried across folds, shorter and longer than a fold), a short first fold, a plan that did not start at capture 0
KERNEL_SHAPES = [(1, 0, [0], 0, 1, 16, 0), (255, 1, [0, 3], 0, 16, 16, 0), (256, 4, [0, 2, 5, 30], 0, 33, 16, 0), (257, 5, [0, 16], 1, 17, 16, 0),
                 (630, 8, [0, 1, 2, 3], 4, 33, 15, 0), (257, 9, [0, 20], 0, 33, 3, 7), (256, 16, [0, 4, 17], 4, 33, 16, 0), (255, 16, [0], 0, 15, 16, 0),
                 (2, 13, [0, 5, 6, 40], 1, 40, 1, 100), (257, 0, [0, 8], 4, 20, 16, 0), (300, 3, [0, 7], 0, 50, 2, 5), (255, 7, [0, 2], 0, 18, 16, 0), (256, 2, [0, 1, 9], 2, 19, 16, 0)]


@pytest.fixture(scope="module")
def host_exe():
    exe = os.path.join(ROOT, "tests", "cpp", "interaural_kernel_host")
    subprocess.check_call(COMPILE + ["-O2", "-o", exe])
    return exe


def test_the_kernels_text_on_the_host_reproduces_the_definition_bytewise(host_exe, tmp_path):
    """Onset, pre and every bin bytewise, both blocks allocated at exactly the plan's byte counts; thresholds that put the onsets of
    different nodes at different captures (a map), so that the held bin differs from lane to lane, and some never reached."""
    rng = np.random.default_rng(23)
    classes = set()
    for case in KERNEL_SHAPES:
        nodes, L, edges, S, t, first_fold, first = case
        a, b = series(rng, t, nodes), series(rng, t, nodes)
        level = np.sort(np.maximum(np.abs(a), np.abs(b)), axis=0)
        thr_map = level[rng.integers(0, t, nodes), np.arange(nodes)].astype(np.float32)    # each node's onset at a capture of its own
        thr_map[::7] = np.float32(3e38)                                                     # ... and every seventh node: never
        for threshold, tmap in ((0.0, None), (float(np.median(level)), None), (0.0, thr_map)):
            want = IA.interaural_fold(a, b, threshold if tmap is None else tmap, edges, L, SECTIONS[:S] if S else None, first_capture=first)
            got = run_host(host_exe, tmp_path, a, b, L, edges, S, threshold, first_fold, first, tmap)
            same(got, want, (case, threshold, tmap is not None))
            if tmap is not None and nodes > 8:
                assert (want["onset"] == IA.NONE).any() and len(set(want["onset"].tolist())) > 3, case
        classes.add((S > 0, 0 if L == 0 else 4 if L <= 4 else 8 if L <= 8 else 16))
    assert len(classes) == 8                                                                # every instance of the kernel ran


def test_equal_ears_give_a_symmetric_correlation(host_exe, tmp_path):
    rng = np.random.default_rng(24)
    a = series(rng, 40, 257)
    got = run_host(host_exe, tmp_path, a, a, 6, [0, 9], 1)
    bins = got["bins"]
    assert bins[:, 0].tobytes() == bins[:, 1].tobytes() == bins[:, 2 + 6].tobytes()
    for l in range(1, 7):
        assert bins[:, 2 + 6 + l].tobytes() == bins[:, 2 + 6 - l].tobytes()


def test_a_nan_is_no_onset_and_poisons_its_node_only(host_exe, tmp_path):
    rng = np.random.default_rng(25)
    a, b = series(rng, 20, 257), series(rng, 20, 257)
    a[3, 100] = np.nan
    want = IA.interaural_fold(a, b, 0.0, [0, 5], 2)
    got = run_host(host_exe, tmp_path, a, b, 2, [0, 5], 0)
    same(got, want, "nan")
    # (ear a's energy and every product with the sample; ear b's energy is ear b's alone)
    assert got["onset"][100] == 0 and np.isnan(got["bins"][0, [0, 2, 3, 4, 5], 100]).all() and not np.isnan(got["bins"][:, 1, 100]).any()
    assert not np.isnan(np.delete(got["bins"], 100, axis=2)).any()
    a[:, 5], b[:, 5] = np.nan, np.nan                       # a node that is NaN throughout never has an onset
    got = run_host(host_exe, tmp_path, a, b, 2, [0, 5], 0)
    assert got["onset"][5] == IA.NONE and np.isnan(got["pre"][:, 5]).all() and not got["bins"][:, :, 5].any()
    same(got, IA.interaural_fold(a, b, 0.0, [0, 5], 2), "nan node")


def test_the_capture_kernels_text_on_the_host(host_exe, tmp_path):
    """ear_gather_kernel over a row-padded field: strides, negative ears, ears at +-8, a grid smaller than the box."""
    rng = np.random.default_rng(26)
    nx, ny, nz, pitch = 40, 30, 19, 64
    field = rng.standard_normal((nz, ny, pitch)).astype(np.float32)
    for (x0, y0, z0), (bx, by, bz), (sx, sy, sz), ear_a, ear_b in (((8, 8, 8), (24, 14, 3), (1, 1, 1), (-8, -8, -8), (8, 8, 8)),
                                                                  ((3, 2, 1), (9, 7, 6), (4, 3, 3), (-3, 0, 2), (1, -2, -1)),
                                                                  ((5, 5, 5), (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0)),
                                                                  ((0, 9, 0), (40, 1, 19), (1, 1, 1), (0, -4, 0), (0, 4, 0))):
        fin, fout = str(tmp_path / "gin.bin"), str(tmp_path / "gout.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<19i", nx, ny, nz, pitch, x0, y0, z0, bx, by, bz, sx, sy, sz, *ear_a, *ear_b) + field.tobytes())
        subprocess.run([host_exe, "gather", fin, fout], check=True, timeout=300)
        got = np.fromfile(fout, np.float32).reshape(2, bz, by, bx)
        for k, ear in enumerate((ear_a, ear_b)):
            want = field[z0 + ear[2]:z0 + ear[2] + bz * sz:sz, y0 + ear[1]:y0 + ear[1] + by * sy:sy, x0 + ear[0]:x0 + ear[0] + bx * sx:sx]
            assert got[k].tobytes() == np.ascontiguousarray(want).tobytes(), (x0, y0, z0, ear)


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (-fno-sanitize-recover: a report is a failure): both blocks,
    every fold's stage, the map and the coefficients are allocated at exactly their sizes."""
    exe = os.path.join(ROOT, "tests", "cpp", "interaural_kernel_host_san")
    subprocess.check_call(COMPILE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    rng = np.random.default_rng(27)
    for nodes, L, edges, S, t, first_fold, first in ((257, 16, [0, 3, 20], 4, 33, 13, 0), (257, 0, [0], 0, 1, 16, 0), (256, 7, [0, 1, 2, 3], 0, 17, 16, 3),
                                                     (3, 1, [0, 2], 1, 35, 16, 0)):
        a, b = series(rng, t, nodes), series(rng, t, nodes)
        tmap = np.abs(a[rng.integers(0, t, nodes), np.arange(nodes)])
        got = run_host(exe, tmp_path, a, b, L, edges, S, 0.0, first_fold, first, tmap)
        same(got, IA.interaural_fold(a, b, tmap, edges, L, SECTIONS[:S] if S else None, first_capture=first), (nodes, L, S))

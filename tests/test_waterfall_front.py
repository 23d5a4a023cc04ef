"""The Python front of the waterfall plan, without a GPU: simulation.waterfall_plan_arguments (valid dicts, every fault alone and every
ordered pair of two), what canonical hands on to the engine (a recording stand-in, as tests/python_front_cases.py builds one), the
refusal of slabs, and tools/waterfall_map.py's refusals as a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import python_front_cases as cases
from wayverb_amd import simulation as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH, Z, BOX = cases.MESH, cases.Z, cases.BOX      # dims (8, 9, 10), spacing 0.05, min corner z = 0.3; plane 4; a box
RATE = 8000.0
KEYS = ("freqs_hz", "every", "bin_ms", "n_bins", "bin_captures", "stride", "first_step")
BASE = dict(freqs_hz=[50.0, 100.0, 200.0], plane=Z, bin_ms=2.0)


def without_bin_ms(**keys):
    return lambda d: (d.pop("bin_ms", None), d.update(keys))


FAULTS = dict(cases.PLANE_FAULTS, **{
    "no-freqs_hz": cases.drop("freqs_hz"), "no-freqs": cases.put(freqs_hz=[]), "65-freqs": cases.put(freqs_hz=list(range(65))),
    "nan-freq": cases.put(freqs_hz=[50.0, float("nan")]), "negative-freq": cases.put(freqs_hz=[-1.0]), "above-nyquist": cases.put(freqs_hz=[50.0, 4100.0]),
    "above-the-series-nyquist": cases.put(freqs_hz=[1400.0], every=3),
    "bin_ms-and-bin_captures": cases.put(bin_captures=3, n_bins=4), "no-bin-length": cases.drop("bin_ms"), "bin_captures-without-n_bins": without_bin_ms(bin_captures=3),
    "bin_ms-0": cases.put(bin_ms=0.0), "bin_ms-nan": cases.put(bin_ms=float("nan")), "bin_captures-0": without_bin_ms(bin_captures=0, n_bins=4),
    "n_bins-0": cases.put(n_bins=0), "n_bins-over-the-cap": cases.put(n_bins=1366)})


def expected(plan, rate=RATE):
    """The sentence a dict is refused with, by the order the function's docstring and DESIGN.md 4.15 give: keys and cadence first, the
    plan's own checks (frequencies, then how long a bin is, then how many) in the middle, the plane last; None for a valid dict."""
    if set(plan) - {"plane", "box"} - set(KEYS) or ("plane" in plan) == ("box" in plan) or "freqs_hz" not in plan:
        return "waterfall=dict(plane=<z in metres> or box=..., freqs_hz=, every=, bin_ms=, n_bins=, bin_captures=, stride=, first_step=)"
    every = int(plan.get("every", 1))
    if every < 1:
        return "waterfall: every must be >= 1"
    freqs = list(np.atleast_1d(np.asarray(plan["freqs_hz"], dtype=np.float64)))
    if not 1 <= len(freqs) <= 64:
        return "waterfall: freqs_hz holds 1 .. 64 frequencies"
    for f in freqs:
        if not 0.0 <= f <= rate / 2.0 / every:
            return "waterfall: %.6g Hz is outside 0 .. %.6g Hz (half the sample rate %.6g Hz divided by every=%d)" % (f, rate / 2.0 / every, rate, every)
    by_ms, by_captures = plan.get("bin_ms") is not None, plan.get("bin_captures") is not None
    if by_ms == by_captures or (by_captures and plan.get("n_bins") is None):
        return "waterfall: a bin is bin_ms= long, or bin_captures= captures long with n_bins= of them"
    if by_ms and not plan["bin_ms"] > 0:
        return "waterfall: bin_ms must be > 0"
    if by_captures and plan["bin_captures"] < 1:
        return "waterfall: bin_captures must be >= 1"
    most = 4096 // len(freqs)
    if plan.get("n_bins") is not None and not 1 <= plan["n_bins"] <= most:
        return "waterfall: n_bins must be 1 .. %d with %d frequencies (4096 sums per node at the most)" % (most, len(freqs))
    if "plane" in plan and not 0 <= int(round((plan["plane"] - MESH.min_corner[2]) / MESH.spacing)) <= MESH.dims[2] - 1:
        return "waterfall: plane z=%g m is outside the mesh" % plan["plane"]
    return None


def says(plan, rate=RATE):
    got = cases.answer(lambda: W.waterfall_plan_arguments(dict(plan), MESH, rate))
    return got.get("says") if got.get("raises") == "ValueError" else got


def test_valid_dicts_become_the_arguments_of_set_waterfall():
    got = W.waterfall_plan_arguments(dict(BASE), MESH, RATE)
    assert sorted(got) == ["bin_captures", "box", "first_step", "freqs", "n_bins", "period", "stride"]
    assert got["freqs"].tolist() == [50.0 / RATE, 100.0 / RATE, 200.0 / RATE]                   # Hz to cycles per STEP, whatever `every`
    assert (got["bin_captures"], got["n_bins"], got["period"], got["stride"], got["first_step"]) == (16, 64, 1, 1, 0)     # 2 ms at 8 kHz
    assert got["box"] == ((0, 0, 4), (None, None, 1))
    # bin_ms to bin_captures: at the rate of the CAPTURED series, rounded, one at the least
    for rate, every, ms, want in ((8000.0, 1, 2.0, 16), (8000.0, 3, 2.0, 5), (12000.0, 3, 2.0, 8), (8000.0, 4, 0.3, 1), (8000.0, 1, 0.01, 1), (12000.0, 1, 10.0, 120)):
        got = W.waterfall_plan_arguments(dict(BASE, every=every, bin_ms=ms), MESH, rate)
        assert (got["bin_captures"], got["period"]) == (want, every), (rate, every, ms)
        assert got["freqs"].tolist() == [50.0 / rate, 100.0 / rate, 200.0 / rate]
    # the default number of bins: 64, or what 4096 sums per node allow
    assert W.waterfall_plan_arguments(dict(BASE, freqs_hz=list(range(1, 65))), MESH, RATE)["n_bins"] == 64
    assert W.waterfall_plan_arguments(dict(BASE, freqs_hz=list(range(1, 101))[:64], n_bins=64), MESH, RATE)["n_bins"] == 64
    assert W.waterfall_plan_arguments(dict(BASE, freqs_hz=100.0, n_bins=4096), MESH, RATE)["n_bins"] == 4096
    assert W.waterfall_plan_arguments(dict(BASE, n_bins=1365), MESH, RATE)["n_bins"] == 1365
    got = W.waterfall_plan_arguments(dict(freqs_hz=[4000.0], box=BOX, n_bins=7, bin_captures=3, stride=(1, 2, 1), first_step=7, every=1), MESH, RATE)
    assert (got["n_bins"], got["bin_captures"], got["box"], got["stride"], got["first_step"]) == (7, 3, BOX, (1, 2, 1), 7) and got["freqs"].tolist() == [0.5]
    assert all(expected(p) is None for p in (BASE, dict(BASE, every=3), dict(freqs_hz=[4000.0], box=BOX, n_bins=7, bin_captures=3)))


def test_every_fault_alone_and_every_ordered_pair_of_faults():
    names = list(FAULTS)
    seen = set()
    for first in names:
        for second in names:
            plan = dict(BASE)
            for name in ([first] if first == second else [first, second]):
                FAULTS[name](plan)
            want = expected(plan)
            got = says(plan)
            if want is None:      # (two faults that undo each other)
                assert isinstance(got, dict) and "returns" in got, (first, second, got)
            else:
                assert got == want, (first, second, got, want)
                seen.add("a frequency" if "Hz is outside" in want else "the plane" if "plane z=" in want else want)
    assert len(names) == 21 and expected(BASE) is None
    for name in names:      # each fault alone IS refused
        plan = dict(BASE)
        FAULTS[name](plan)
        assert expected(plan) is not None, name
    assert len(seen) == 9      # keys, every, the count of frequencies, a frequency, how long a bin is, bin_ms, bin_captures, n_bins, the plane


def test_plan_call_and_canonical_hand_the_arguments_on():
    vm, source, receiver = cases.box_scene(W)
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)
    plan = dict(freqs_hz=[0.0, rate / 16.0], plane=5 * vm.mesh.spacing, every=2, n_bins=3, bin_captures=2)
    name, positional, keywords = W.plan_call("waterfall", plan, vm.mesh, rate, env, 0.01)
    assert (name, positional) == ("waterfall", ()) and keywords["freqs"].tolist() == [0.0, 1.0 / 16.0]
    assert {k: v for k, v in keywords.items() if k != "freqs"} == dict(n_bins=3, bin_captures=2, box=((0, 0, 5), (None, None, 1)), stride=1, first_step=0, period=2)
    assert [k for k, _ in W.PLANS][:7] == list(cases.PLAN_KEYWORDS) and [k for k, _ in W.PLANS][7:] == ["waterfall"]
    log = []

    def run_fast(eng, kind, index, signal, receivers, keep_going=None):
        log.append(["run_fast"])
        return signal.shape[0], np.zeros((signal.shape[0], 7))

    with cases.stand_ins(W.E, Engine=lambda *a, **k: cases.RecordingEngine(log, *a, **k), run_fast=run_fast):
        bands, taken = W.canonical(vm, source, receiver, env, 100.0, 0.6, 9.5 / rate, precision="f32", waterfall=plan)
    assert taken == "what fetch_waterfall returned" and len(bands) == 1
    calls = [c[0] for c in log]
    assert calls == ["Engine", "set_waterfall", "run_fast", "fetch_waterfall", "close"]
    assert log[1] == ["set_waterfall", [], cases.canon(keywords)]
    # impulse_response() hands the dict to canonical under its keyword
    seen = {}

    def canonical(vm_, source_, receiver_, environment, cutoff, usable_portion, simulation_time, precision, device, **given):
        seen.update(given)
        return ["bands"], "what was taken"

    with cases.stand_ins(W, compute_voxels_and_mesh=lambda *a, **k: vm, canonical=canonical), cases.stand_ins(W.P, postprocess=lambda *a, **k: "audio"):
        got = W.impulse_response(None, None, None, source, receiver, waterfall=plan)
    assert seen == dict(waterfall=plan) and len(got) == 4 and got[3] == "what was taken"


def test_slabs_are_refused_and_every_earlier_keyword_answers_first():
    def slabbed(**plans):
        return cases.answer(lambda: W.canonical(None, None, None, None, 100.0, 0.6, 0.01, slabs=2, **plans))
    assert slabbed(waterfall={}) == {"raises": "ValueError", "says": "waterfall sums are accumulated on one domain only (slabs=1)"}
    for keyword in cases.PLAN_KEYWORDS:
        assert slabbed(**{keyword: {}, "waterfall": {}}) == slabbed(**{keyword: {}}) != slabbed(waterfall={})
    assert list(W.SLABS_REFUSALS)[-1] == "waterfall" and len(W.SLABS_REFUSALS) == 8


TOOL_REFUSALS = {
    "--freqs by name": (["--freqs", "low,high"], "--freqs takes 1 .. 64 frequencies in Hz, e.g. 31.5,40,50"),
    "--freqs negative": (["--freqs", "40,-80"], "--freqs takes 1 .. 64 frequencies in Hz, e.g. 31.5,40,50"),
    "--freqs 65": (["--freqs", ",".join(str(k) for k in range(65))], "--freqs takes 1 .. 64 frequencies in Hz, e.g. 31.5,40,50"),
    "--plane without z=": (["--freqs", "40", "--plane", "1.5"], "--plane takes z=<metres>"),
    "--plane z=abc": (["--freqs", "40", "--plane", "z=abc"], "--plane takes z=<metres>"),
    "--every 0": (["--freqs", "40", "--every", "0"], "--every must be >= 1 and --bin-ms positive"),
    "--bin-ms 0": (["--freqs", "40", "--bin-ms", "0"], "--every must be >= 1 and --bin-ms positive"),
    "--bin-ms nan": (["--freqs", "40", "--bin-ms", "nan"], "--every must be >= 1 and --bin-ms positive"),
    "--room 4": (["--freqs", "40", "--room", "4"], "--room takes 8 or more nodes per axis, and no --obj beside it"),
    "--freqs before --plane": (["--freqs", "x", "--plane", "1.5"], "--freqs takes 1 .. 64 frequencies in Hz, e.g. 31.5,40,50"),
    "--plane before --every": (["--freqs", "40", "--plane", "1.5", "--every", "0"], "--plane takes z=<metres>"),
    "no --freqs": ([], "the following arguments are required: --freqs"),
}


@pytest.mark.parametrize("case", sorted(TOOL_REFUSALS))
def test_the_tool_refuses_with_exit_2_and_the_sentence(case):
    arguments, sentence = TOOL_REFUSALS[case]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "waterfall_map.py")] + arguments, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and p.stderr.strip().splitlines()[-1] == "waterfall_map.py: error: " + sentence, p.stderr[-2000:]

"""The march planners (wayverb_amd/csrc/march_plan.h: windows of a long row, chunks along z, a sparse room's work list) on the CPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_march_plans_equal_the_recorded_ones_and_hold_together():
    """tests/cpp/march_plan_test.cpp: inputs from fixed formulas through split_row / triple_windows, choose_chunks and plan_units with the
    two-step and the three-step march's parameters.  The program checks what must hold by construction (every live unit listed once and no
    dead one, the eight runs, their order, spans that cover their masks) and prints what the planners made; that equals
    tests/golden/march_plan_cases.json, recorded from the planners as they stood inside the engine before they moved to the header.
    No GPU."""
    src = os.path.join(ROOT, "tests", "cpp", "march_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "march_plan_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "wayverb_amd", "csrc"), src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "MARCH PLAN OK" in p.stdout, p.stdout[-4000:] + p.stderr
    got = json.loads(p.stdout[:p.stdout.index("MARCH PLAN OK")])
    with open(os.path.join(ROOT, "tests", "golden", "march_plan_cases.json")) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, "\n".join("%s: got %s, recorded %s" % (k, got[k], want[k]) for k in differ[:8])

"""The Python front of the capture plans -- simulation.py's *_plan_arguments, canonical and impulse_response(), the Engine's plan
wrappers, tools/impulse_response.py's refusals -- says and does what tests/golden/python_front.json holds, recorded from the commit
before their copies were folded (tests/python_front_cases.py; profiles/r21/README.md).  No GPU: stand-ins take the engine's place."""
import json

import numpy as np
import pytest

import python_front_cases as cases


@pytest.fixture(scope="module")
def golden():
    with open(cases.GOLDEN) as f:
        return cases.unpack(json.load(f))


@pytest.fixture(scope="module")
def tree():
    return cases.record()


def test_the_tree_answers_every_case_as_the_fixture_has_it(golden, tree):
    want, got = dict(cases.cases_of(golden)), dict(cases.cases_of(tree))
    assert sorted(got) == sorted(want), "the cases are not the fixture's: %r" % sorted(set(got) ^ set(want))[:8]
    assert len(want) > 900
    differ = [name for name in want if got[name] != want[name]]
    with open(cases.GOLDEN) as f:
        recorded_under = json.load(f)["numpy"]
    assert not differ, ("%d cases differ, the first: %s\n  fixture: %s\n  tree:    %s\n(where only a sha256 differs: it is of an array, and the arrays "
                        "of filter sections are designed by libwayverb_amd.so -- wv_butterworth_bandpass -- so they follow its compiler and libm, "
                        "not the Python front; the fixture was recorded under NumPy %s, this is NumPy %s)") % (
        len(differ), differ[0], json.dumps(want[differ[0]], sort_keys=True), json.dumps(got[differ[0]], sort_keys=True), recorded_under, np.__version__)


def test_the_fixture_repacks_to_itself(golden):
    with open(cases.GOLDEN) as f:
        fixture = json.load(f)
    assert cases.pack(golden)["answers"] == fixture["answers"] and cases.pack(golden)["cases"] == fixture["cases"]


def test_every_sentence_of_the_front_is_in_some_case(golden):
    said = [got.get("says", "") + " ".join(got.get("warnings", [])) for _, got in cases.cases_of(golden)]
    missing = [lead for lead in cases.SENTENCES if not any(lead in s for s in said)]
    assert not missing, "no case of the fixture says: %r" % missing
    assert len(cases.SENTENCES) == len(set(cases.SENTENCES)) == 56


def test_no_injected_fault_went_unanswered(golden):
    unanswered = [name for name, got in cases.cases_of(golden)
                  if ("/faults/" in name or "/slabs/" in name or "/refusals/" in name) and "raises" not in got
                  or name.startswith(("tool/pairs/", "tool/receivers/", "tool/malformed/", "tool/multiband/")) and got["exit"] != 2]
    assert not unanswered, unanswered
    faults = [name for name, _ in cases.cases_of(golden) if "/faults/" in name]
    assert len(faults) == sum(len(spec["faults"]) ** 2 for spec in cases.ARGUMENTS.values())

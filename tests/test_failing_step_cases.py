"""Every failing-step case proves itself against the oracle alone before it meets the engine (tests/failing_step_cases.py): run from the
case's fields, the oracle fails at step k exactly, with exactly ERR_INF where the value is made by overflow (the word the table
records where it is written), and the target is among the non-finite nodes of the failing step -- the only one where it overflowed."""
import numpy as np
import pytest

import failing_step_cases as F
from wayverb_amd import mesh as M

NEEDS = {"inf": M.ERR_INF, "inf-inf": M.ERR_INF | M.ERR_NAN, "nan": M.ERR_NAN}


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_the_oracle_fails_at_the_chosen_step_at_the_chosen_node(case):
    mesh = F.mesh_of(case.mesh)
    target = mesh.compute_index(*case.target)
    prev, cur, bd = F.poisoned_fields(case)
    # level by level: nothing before the k-th step, then the word, and who went non-finite
    s, flag, bad = F.first_flag(case, prev, cur, bd)
    assert s == case.k - 1 and flag != 0
    assert target in bad
    if case.how == "overflow":
        assert flag == M.ERR_INF
        assert np.all(np.isfinite([v for _, v in F.placements(case)]))
        assert bad.tolist() == [target]
    else:
        assert case.k == 1 and flag & NEEDS[case.how] == NEEDS[case.how]
    # the run loop says the same: the step, the word, and rows up to the failing step only
    done, word, rows = F.expected(case)
    assert (done, word) == (case.k - 1, flag)
    assert rows.shape == (F.PREFIX + done, 3) and np.all(np.isfinite(rows))


def test_the_table_omits_nothing():
    """Every class at every level in both precisions, but for the three pairs no shell can single out; nothing skipped."""
    ids = {c.id for c in F.CASES}
    assert F.OMITTED == {("edge-crook", 3), ("corner-crook", 2), ("corner-crook", 3)}
    for name, _ in F.BOX_CLASSES:
        for tag in ("f32", "f64"):
            for k in (1, 2, 3):
                assert ("%s-%s-k%d" % (name, tag, k) in ids) == ((name, k) not in F.OMITTED)
    for name in ("face-lo", "next-to-face-lo", "march-lo", "face-hi", "next-to-face-hi", "march-hi"):
        for k in (1, 2, 3):
            assert "slab-%s-f64-k%d" % (name, k) in ids

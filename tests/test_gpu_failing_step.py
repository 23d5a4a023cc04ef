"""The step a run stops at, and the word it stops with, in every stepping form of the engine: the cases of tests/failing_step_cases.py
(each proven on the CPU against the oracle alone, tests/test_failing_step_cases.py) put a non-finite value on a chosen node at a chosen
level of a pass.  Whichever launch owns that node's flag at that level -- the march and the exact-flags check behind it, the fix-up
lists, the boundary launches, the x-facing walls' routine, a slab's face steps -- the engine has to name the oracle's step and the
oracle's word, and the receiver rows up to there have to be the oracle's bytes.  A twin engine that takes the same calls without the
poison shows which passes the nine steps are taken in, so that step k of the run is level k of a pass."""
import numpy as np
import pytest

import failing_step_cases as F
from helpers import set_tuning
from wayverb_amd import engine as E
from wayverb_amd.slab import SlabLayout, slab_mesh

pytestmark = pytest.mark.gpu

TRIPLE = dict(pair=1, triple=1, tile_lists=0)


def _triple_forms():
    out = []
    for extra_name, extra in (("", {}), ("-unfused", dict(fuse_pre_post=0)), ("-inner0", dict(pair_inner_fix=0))):
        for xwall in (1, 2, 0):
            out.append(("triple-xwall%d%s" % (xwall, extra_name), dict(TRIPLE, boundary_xwall=xwall, **extra), "triple"))
    return out


# (name, tuning, how the twin has to take nine steps from a pass boundary: "triple" = three three-step passes, "pair" = four two-step
# passes and a single step, "single" = nine single steps)
FORMS = {
    "f64": [("default", {}, "single"), ("pair0", dict(pair=0), "single"), ("pair0-whole0", dict(pair=0, whole_step=0), "single"),
            ("pair1", dict(pair=1), "pair"), ("pair1-inner0", dict(pair=1, pair_inner_fix=0), "pair")] + _triple_forms(),
    "f32": [("default", {}, "single"), ("pair1", dict(pair=1), "pair"), ("triple", dict(TRIPLE), "triple")],
}
SLAB_FORMS = [("single-steps", {}, "single"), ("two-step-passes", dict(pair=1, slab_early=1), "pair"),
              ("three-step-passes", dict(pair=1, triple=1, slab_early=1, tile_lists=0), "triple")]
TAKEN = {"triple": (3, 0), "pair": (0, 4), "single": (0, 0)}


def forms_of(case):
    if case.slabs:
        return SLAB_FORMS
    if case.seam:  # the three-step march with the tuning that puts the seam where the table says, and the two-step march beside it
        seam = dict(case.seam)
        return [("triple-seam", dict(TRIPLE, **seam), "triple"), ("triple-seam-xwall0", dict(TRIPLE, boundary_xwall=0, **seam), "triple"),
                ("pair1", dict(pair=1), "pair")][:3 if case.tag == "f64" else 1]
    return FORMS[case.tag]


@pytest.fixture(autouse=True)
def _library_defaults(built_library):
    set_tuning()
    yield
    set_tuning()


class Single:
    """One engine over the whole mesh."""

    def __init__(self, case, tuning):
        self.mesh = F.mesh_of(case.mesh)
        self.eng = E.Engine(self.mesh, precision=case.tag, tuning=tuning, **F.engine_kw(case))
        prev, cur = F.quiet_fields(case.mesh, case.tag)
        self.eng.write_field(prev, E.BUF_PREVIOUS)
        self.eng.write_field(cur, E.BUF_CURRENT)
        self.eng.set_receivers(F.receivers(case))

    def run_steps(self, n):
        return self.eng.run_steps(n)

    def write_value(self, node, value):
        self.eng.write_value(node, value)

    def passes(self):
        return [(self.eng.query(E.Engine.QUERY_TRIPLE_PASSES), self.eng.query(E.Engine.QUERY_PASSES))]

    def step_counts(self):
        return [self.eng.step_count()]

    def rows(self, n):
        return self.eng.fetch_receivers(0, n)

    def close(self):
        self.eng.close()


class Chain:
    """The mesh cut into z-slabs of this process (LocalSlabGroup): a value goes to every slab that holds the node, ghost copies included;
    a receiver is recorded by the slab that owns it."""

    def __init__(self, case, tuning):
        gmesh = F.mesh_of(case.mesh)
        prev, cur = F.quiet_fields(case.mesh, case.tag)
        recv = F.receivers(case)
        self.layouts, self.engines, self.columns = [], [], []
        for r in range(case.slabs):
            L = SlabLayout(gmesh.dims, r, case.slabs)
            e = E.Engine(slab_mesh(gmesh, L), precision=case.tag, ghost_lo=L.ghost_lo, ghost_hi=L.ghost_hi, tuning=tuning)
            e.write_field(prev[L.zl0 * L.plane:L.zl1 * L.plane], E.BUF_PREVIOUS)
            e.write_field(cur[L.zl0 * L.plane:L.zl1 * L.plane], E.BUF_CURRENT)
            mine = [(pos, L.to_local(node)) for pos, node in enumerate(recv) if L.owns_z(node // L.plane)]
            e.set_receivers([idx for _, idx in mine])
            self.layouts.append(L)
            self.engines.append(e)
            self.columns.append([pos for pos, _ in mine])
        self.n_recv = len(recv)
        self.group = E.LocalSlabGroup(self.engines)

    def run_steps(self, n):
        return self.group.run_steps(n)

    def write_value(self, node, value):
        holders = [(e, L.to_local(node)) for e, L in zip(self.engines, self.layouts) if L.to_local(node) is not None]
        assert holders
        for e, local in holders:
            e.write_value(local, value)

    def passes(self):
        return [(e.query(E.Engine.QUERY_TRIPLE_PASSES), e.query(E.Engine.QUERY_PASSES)) for e in self.engines]

    def step_counts(self):
        return [e.step_count() for e in self.engines]

    def rows(self, n):
        out = np.full((n, self.n_recv), np.nan)
        for e, cols in zip(self.engines, self.columns):
            got = e.fetch_receivers(0, n)
            for col, pos in enumerate(cols):
                out[:, pos] = got[:, col]
        return out

    def close(self):
        self.group.close()


def run_form(case, tuning, poisoned):
    """The call sequence of one form: quiet fields, the healthy prefix, the case's values (or not: the twin), nine steps."""
    domain = (Chain if case.slabs else Single)(case, tuning)
    try:
        assert domain.run_steps(F.PREFIX) == (F.PREFIX, 0)
        before = domain.passes()
        if poisoned:
            for node, value in F.placements(case):
                domain.write_value(node, value)
        done, flag = domain.run_steps(F.RUN)
        taken = [(t1 - t0, p1 - p0) for (t0, p0), (t1, p1) in zip(before, domain.passes())]
        return dict(done=done, flag=flag, taken=taken, step_counts=domain.step_counts(), rows=domain.rows(F.PREFIX + done))
    finally:
        domain.close()


_twins = {}


def twin_of(case, name, tuning):
    """The twin's run: the same calls without the case's values.  Cases that share mesh, precision, receivers and form share the call
    sequence, hence the twin."""
    key = (case.mesh, case.tag, case.slabs, name, tuple(sorted(tuning.items())), tuple(F.receivers(case)))
    if key not in _twins:
        _twins[key] = run_form(case, tuning, poisoned=False)
    return _twins[key]


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_every_form_stops_at_the_oracles_step_with_the_oracles_word(case):
    want_done, want_flag, want_rows = F.expected(case)
    assert want_done == case.k - 1 and want_flag != 0     # (tests/test_failing_step_cases.py: why)
    dtype = F.DTYPE[case.tag]
    failures = []
    for name, tuning, kind in forms_of(case):
        twin = twin_of(case, name, tuning)
        assert (twin["done"], twin["flag"]) == (F.RUN, 0), name
        assert all(t == TAKEN[kind] for t in twin["taken"]), (name, twin["taken"])   # step k of the run is level k of a pass
        got = run_form(case, tuning, poisoned=True)
        print("%s %s: engine (%d, %d), oracle (%d, %d)" % (case.id, name, got["done"], got["flag"], want_done, want_flag))
        if (got["done"], got["flag"]) != (want_done, want_flag):
            failures.append("%s: stopped at (%d, %d), the oracle at (%d, %d)" % (name, got["done"], got["flag"], want_done, want_flag))
            continue
        if any(c != F.PREFIX + want_done for c in got["step_counts"]):
            failures.append("%s: step_count %r" % (name, got["step_counts"]))
        if got["rows"].astype(dtype).tobytes() != want_rows.tobytes():
            failures.append("%s: receiver rows up to the failing step differ from the oracle's" % name)
    assert not failures, "\n".join(failures)

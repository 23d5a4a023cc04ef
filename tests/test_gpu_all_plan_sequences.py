"""The family `all-plans` of tests/test_gpu_plan_sequences.py -- all eight kinds of capture plan in ONE random sequence of API calls, with
a plan replaced by one of its own kind, refused setters, refused rollbacks and plans stopped mid-way -- under the names its cases have
had since they were written.  Nothing of the fuzz lives here: the scripts, the replay and the comparisons are tests/plan_twin.py's, the
modes, the engine and the tally are that module's run_case."""
import pytest

import plan_twin as P
import test_gpu_plan_sequences as S

pytestmark = pytest.mark.gpu

_default_tuning_afterwards = S._default_tuning_afterwards


@pytest.mark.parametrize("mode", S.FAMILY_MODES["all-plans"])
@pytest.mark.parametrize("seed", range(P.FAMILIES["all-plans"].seeds))
def test_random_sequence_of_all_plans(oracle, built_library, seed, mode):
    S.run_case(oracle, "all-plans", seed, mode)


def test_every_mode_met_its_form():
    """Each forced mode took the form it is named after in a quarter of the seeds at the least (a plan of period 1 or 2 leaves no
    room for a three-step pass, one of period 1 none for any).  Of `graph-and-passes` only the passes can be seen: the engine has no
    query that counts replayed graphs (it replays one for an even batch of 16 steps or more on a mesh with clean outside nodes,
    engine_batch.hip.h), so that a graph was replayed is NOT shown."""
    S.met_in_a_quarter_of_the_seeds("all-plans", [
        ("three-step-passes", "three-step passes", lambda t: t[1] > 0),
        ("graph-and-passes", "two-step passes", lambda t: t[0] > 0),
        ("single-steps", "one-launch steps", lambda t: t[2] > 0),
        ("single-steps", "no pass", lambda t: t[0] == 0 and t[1] == 0),
        ("default", "one-launch steps", lambda t: t[2] > 0)])

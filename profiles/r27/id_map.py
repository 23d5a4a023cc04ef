"""id_map.py PARENT_IDS THIS_IDS: the test ids of `pytest --collect-only -q -m gpu tests` at the parent and at this tree, every id the
parent has and this tree has not mapped to the id that covers it, the ids only this tree has, and the totals.  Exits 1 if a deleted
id has no cover, a cover does not exist, or the total fell."""
import re
import sys

KIND = {"spectrum": "spectrum", "decay": "decay", "decay_bands": "banded", "intensity": "intensity", "arrival": "arrival", "lateral": "lateral",
        "modulation": "modulation", "arrival_bands": "arrival_bands", "waterfall": "waterfall", "interaural": "interaural"}
NEW = "tests/test_gpu_plan_life_cycle.py::"


def ids(path):
    return [line.strip() for line in open(path) if "::" in line and line.startswith("tests/")]


def cover(old):
    m = re.fullmatch(r"tests/test_gpu_(\w+)\.py::(\w+?)(?:\[(.*)\])?", old)
    if not m or m.group(1) not in KIND:
        return None
    kind, name, param = KIND[m.group(1)], m.group(2), m.group(3)
    if name == "test_fetching_mid_run_and_at_the_end":
        return NEW + "test_fetching_mid_run_and_at_the_end[%s]" % kind
    if name == "test_calls_of_1_7_and_30_steps_give_the_same_bytes":                            # spectrum: f32, every second step
        return NEW + "test_calls_of_1_7_and_30_steps_give_the_same_bytes[%s-%s-f32-every2]" % (kind, param)
    if name == "test_calls_of_one_seven_and_thirty_steps_give_the_same_bytes":                  # waterfall: f64, pair
        return NEW + "test_calls_of_1_7_and_30_steps_give_the_same_bytes[%s-pair-f64-every1]" % kind
    if name == "test_calls_of_one_seven_and_thirty_steps_and_a_fetch_mid_run_give_the_same_bytes":      # interaural: f32, pair, a map
        return NEW + "test_calls_of_1_7_and_30_steps_give_the_same_bytes[%s-pair-f32-every1]" % kind
    if name.startswith("test_a_run_that_stops_on_a_flag_"):
        return NEW + "test_a_run_that_stops_on_a_flag_folds_no_capture_of_a_later_step[%s-%s]" % (kind, param if "-" in param else param + "-triple")
    if name.startswith("test_checkpoint_run_rollback_rerun_gives_the_same_"):
        return NEW + "test_checkpoint_run_rollback_rerun_gives_the_same_outputs_twice[%s-%s]" % (kind, param)
    if name.startswith("test_generic_steps_in_between_"):
        return NEW + "test_generic_steps_in_between_capture_nothing[%s]" % kind
    if name.startswith("test_kernel_timing_accounts_for_") or name.startswith("test_queries_count_folds_and_captures_and_kernel_timing"):
        return NEW + "test_kernel_timing_accounts_for_the_fold_and_the_gather_kernels[%s]" % kind
    return None


parent, this = ids(sys.argv[1]), ids(sys.argv[2])
gone, new = [i for i in parent if i not in set(this)], [i for i in this if i not in set(parent)]
bad, covers = 0, set()
print("# deleted at this tree -> covered by (%d ids)" % len(gone))
for old in gone:
    to = cover(old)
    ok = to is not None and to in set(this)
    bad += not ok
    covers.add(to)
    print("%s -> %s%s" % (old, to, "" if ok else "   !!! NO COVER"))
print()
only = [i for i in new if i not in covers]
print("# only at this tree: the union's additions, and what stayed behind of a deleted test (%d ids)" % len(only))
for i in only:
    print(i)
print()
print("# collected with -m gpu: parent %d, this tree %d (%+d); deleted %d, covering ids %d, new-only %d" % (len(parent), len(this), len(this) - len(parent), len(gone), len(covers), len(only)))
sys.exit(1 if bad or len(this) < len(parent) else 0)

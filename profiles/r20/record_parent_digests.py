"""tests/golden/plan_sequence_digests.json from the generators of the commit BEFORE the four sequence fuzzes became one: this tree's
plan_twin.digest over the 90 scripts of that commit's four build_script functions.

    git worktree add ../parent <the parent commit>
    python profiles/r20/record_parent_digests.py ../parent > tests/golden/plan_sequence_digests.json

The library and the oracle are this tree's, built (that commit's are the same sources); only tests/ and tests/golden/ come from the
parent's checkout."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT = os.path.abspath(sys.argv[1])

sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
digest = importlib.import_module("plan_twin").digest
for name in ("plan_twin", "helpers"):      # (the parent's modules of these names come next)
    del sys.modules[name]
sys.path[1:2] = [os.path.join(PARENT, "tests"), os.path.join(PARENT, "tests", "golden")]

import all_plans_twin  # noqa: E402
import plan_twin  # noqa: E402
import test_gpu_arrival_bands_sequences  # noqa: E402
import test_gpu_modulation_sequences  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

assert plan_twin.__file__.startswith(PARENT) and not hasattr(plan_twin, "digest")
oracle = Oracle()
families = {"plans": (plan_twin.build_script, plan_twin.SEEDS), "all-plans": (all_plans_twin.build_script, all_plans_twin.SEEDS),
            "modulation": (test_gpu_modulation_sequences.build_script, test_gpu_modulation_sequences.SEEDS),
            "arrival-bands": (test_gpu_arrival_bands_sequences.build_script, test_gpu_arrival_bands_sequences.SEEDS)}
out = {"numpy": np.__version__, "digests": {family: [digest(build(oracle, seed)) for seed in range(seeds)] for family, (build, seeds) in families.items()}}
json.dump(out, sys.stdout, indent=1)
print()

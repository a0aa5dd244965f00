"""Child process of test_memory_contract_gpu.py::test_interpreted_plans_on_poisoned_pools: one cycle plan (argv: cycle
file, fused | unfused, output .npy) run for two windows under the environment the parent set (MG_POOL_POISON,
MG_CYCLE_BATCH=0: both are read once).  The two windows must agree bit for bit; the last U goes to the .npy file."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_poisson_solver_amd as mg

mg.init(0)
path, mode, out = sys.argv[1:4]
plan = mg.CyclePlan(path, fused=mode == "fused")
a = plan.execute(fetch_U=True)
b = plan.execute(fetch_U=True)
plan.close()
assert a["status"] == 0 and b["status"] == 0, (a["status"], b["status"])
assert np.array_equal(a["U"].view(np.uint64), b["U"].view(np.uint64)), "two windows of one plan differ"
np.save(out, b["U"])
print("POISON_PLAN OK " + json.dumps({"mg_error": b["mg_error"], "schedule_launches": b["schedule_launches"]}), flush=True)
mg.finalize()

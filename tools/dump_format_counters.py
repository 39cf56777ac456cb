#!/usr/bin/env python3
"""Write tests/golden/format_runs_counters.json: the GN-evaluation counters of the recurring-width case of
tests/test_gpu_format_runs.py as the library in ONGYM_HIP_LIB computes them (needs a GPU).

    ONGYM_HIP_LIB=/path/to/parent/libongym_hip.so python tools/dump_format_counters.py [--out FILE]

The fixture pins the counters of the run-table rule to the rule it replaced, so it is written once with the library of the
commit BEFORE the run table and never with the tree under test; the script refuses to run without ONGYM_HIP_LIB."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "format_runs_counters.json"))
a = ap.parse_args()
if not os.environ.get("ONGYM_HIP_LIB"):
    sys.exit("set ONGYM_HIP_LIB to the parent commit's library: the fixture never comes from the tree under test")

from common import golden_tables                                                            # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv                             # noqa: E402
from test_gpu_format_runs import COUNTERS, recurring_width_case                             # noqa: E402

kw, B, seed, warm, steps = recurring_width_case()
env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
env.seed(seed); env.reset()
assert env.occupancy()["lean_kernel"]
env.step_policy(warm, record=False)
env.step_policy(steps)
st = env.stats()
doc = {"library": "parent commit (first fit groups derived per evaluation)",
       "recurring_width": {c: st[c].tolist() for c in COUNTERS}}
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", a.out, {c: int(st[c].sum()) for c in COUNTERS})

#!/usr/bin/env python3
"""max |dlogp| of the bf16 kernels against the bf16 arithmetic model (oracle/bf16_model.py) per case group of
tests/test_gpu_bf16_model.py: per group the largest max-abs gap of a case and the largest mean-abs gap; the bounds in
oracle/bf16_model.py are 2x these.  Test-side tool (it imports
the CPU model and the test's case list).  --json PATH also writes every case's gap."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tests import test_gpu_bf16_model as t  # noqa: E402

out = {}
worst = 0.0
for group, calls in t.GROUPS.items():
    t0 = time.time()
    res = []
    for fn, args in calls:
        res += fn(torch, *args)
    g = max(r[1] for r in res)
    gm = max(r[2] for r in res)
    worst = max(worst, gm)
    out[group] = {r[0]: r[1:] for r in res}
    top = max(res, key=lambda r: r[1])
    print(f"{group:18s} max {g:.3e} ({top[0]})  mean {gm:.3e}  {len(res)} cases, {time.time() - t0:.1f} s", flush=True)
print(f"worst mean gap {worst:.3e}")
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f, indent=1)

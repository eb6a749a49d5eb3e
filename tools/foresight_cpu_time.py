"""Solver time of the perfect-foresight recursion on the CPU oracle, the figure the GPU sweep's time stands next to.

Times the NumPy-on-oracle twin of the backward sweep (tests/foresight_twin.py: one oracle env per (node, action) through
oracle/libshems_oracle.so, float64 interpolation in NumPy) over 24 hours of ONE problem -- the Charger98 test series from row 1 -- at
the default grid (65 x 33 nodes, 17 x 17 actions), and scales it linearly to the series' horizon: every hour costs the same
nodes x actions evaluations.  It reads oracle/ and therefore stays separate from tools/foresight_demo.py, which must not.

    python tools/foresight_cpu_time.py [out.json]     (default profiles/r10_foresight_cpu.json; run beside the GPU run, needs no GPU)
"""
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import foresight_twin as FT
import util as U
from util import oracle_c

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_foresight_cpu.json")
HOURS = 24
tab = U.tables_mod().profile_table(98, "test")
prof = oracle_c.profile(98)
grid = dict(nb=65, ne=33, nab=17, nae=17)
FT.twin_solve(tab, prof, 1, 2, **grid)                       # warm-up: builds / loads the oracle
t0 = time.perf_counter()
V, _ = FT.twin_solve(tab, prof, 1, HOURS, **grid)
dt = time.perf_counter() - t0
horizon = tab.shape[0] - 1
evals = grid["nb"] * grid["ne"] * grid["nab"] * grid["nae"]
doc = {"what": "NumPy-on-oracle backward sweep, one problem (Charger98 test series from row 1), default grid", "grid": grid,
       "hours_timed": HOURS, "seconds": dt, "evaluations_per_hour": evals, "evaluations_per_s": evals * HOURS / dt,
       "horizon_hours": horizon, "seconds_scaled_to_horizon": dt / HOURS * horizon,
       "timing_method": "time.perf_counter around one call after a 2-hour warm-up call; one thread drives the oracle (orc_batch_step "
                        "is a serial loop); scaled linearly: every hour is the same nodes x actions evaluations",
       "cpu": platform.processor() or platform.machine(), "V0_checksum": float(V[0].sum())}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps(doc))

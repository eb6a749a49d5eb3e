"""The perfect-foresight controller next to the rule-based one, on every series this project holds (not a benchmark, not a test).

For the 15 real exogenous series of data/mpc_series.npz and the synthetic Charger98 splits, from the reset!(rng = -1) start over the
whole series (T = rows - 1: a pass of n steps reads row n + 1):
    the rule-based return (harness.inference, track < 0);
    the foresight return with its profit / discomfort / penalty sums (foresight.solve + foresight.track);
    V_0 at the start state and its gap to the achieved return -- the discretisation error made visible;
    the same at state grids 33 x 17 and 129 x 65, so a reader sees whether the default 65 x 33 has converged;
    the wall time of solve and of track by HIP events, after a warm-up call.
Beside each real series stands the profit the reference's MPC benchmark reached on it (tests/golden/mpc_profit_sums.json).  The MPC
maximises p_sell * PV_GR - p_buy * (GR_DE + GR_EV) - costfactor * p_buy * EX_EV under LINEAR SoC dynamics, with kWh set-points as
decisions; the foresight controller maximises the reward of step! as written (SoC-target actions, penalty term, Float32 stores) on a
discretised state.  The two are neighbours, not equals: the figures are reported, never asserted.

    python tools/foresight_demo.py [out.json]        (default profiles/r10_foresight.json; needs the GPU, does not read oracle/)
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
F = importlib.import_module(PKG + ".foresight")
H = importlib.import_module(PKG + ".harness")

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_foresight.json")
GRIDS = {"33x17": F.Grid(33, 17), "65x33": F.Grid(), "129x65": F.Grid(129, 65)}
mpc = json.load(open(os.path.join(ROOT, "tests", "golden", "mpc_profit_sums.json")))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def one_series(name, cid, tab):
    T = tab.shape[0] - 1
    cfg = S.make_config(cid, 0, tab.shape[0])
    env = S.ShemsBatch(1, T, [tab], [cfg]).use_torch_stream()
    rule_total, rule_res = H.inference(env, track=-1)
    doc = {"charger": cid, "rows": int(tab.shape[0]), "hours": T, "rule_based_return": float(rule_total[0]),
           "rule_based_profit": float(rule_res[:, 6].sum()), "grids": {}}
    for gname, grid in GRIDS.items():
        env.reset_(-1)
        start = env.state[0]
        F.solve(env, [cfg], 1, min(T, 24), grid, want_argmax=False)                      # warm-up (module load, LDS opt-in)
        val, solve_ms = timed(lambda: F.solve(env, [cfg], 1, T, grid, want_argmax=False))
        (tot, res, _), track_ms = timed(lambda: F.track(env, val, which=0))
        v0 = val.at(0, 0, start[0], start[1])
        doc["grids"][gname] = {"foresight_return": float(tot[0]), "profit": float(res[0][:, 6].sum()), "discomfort": float(res[0][:, 7].sum()),
                               "penalty": float(res[0][:, 8].sum()), "V0_at_start": v0, "V0_minus_return": v0 - float(tot[0]),
                               "solve_ms": solve_ms, "track_ms": track_ms, "evaluations": T * grid.nodes * grid.actions}
        del val
    if name in mpc:
        doc["mpc_profit_total"] = mpc[name]["profit_total"]
        doc["mpc_ext_ev_sum"] = mpc[name]["ext_ev_sum"]
    env.close()
    return doc


def warm_up():
    """The first launch of each kernel (module load) stays out of every timed call."""
    tab = S.tables.synthetic_table("eval", 98)
    cfg = S.make_config(98, 0, tab.shape[0])
    env = S.ShemsBatch(1, 24, [tab], [cfg]).use_torch_stream()
    env.reset_(-1)
    F.track(env, F.solve(env, [cfg], 1, 24, F.Grid(), want_argmax=False), which=0)
    env.close()


warm_up()
series = {}
for key in S.tables.real_series_keys():
    cid, split = int(key[7:9]), key.split("_")[1]
    series[key] = one_series(key, cid, S.tables.real_series(cid, split))
for split in ("train", "eval", "test"):
    series[f"synthetic_Charger98_{split}"] = one_series(None, 98, S.tables.synthetic_table(split, 98))

# many problems in one call: the six real test series (2 998 hours each) at the default grid
keys = [k for k in S.tables.real_series_keys() if k.endswith("_test")]
tabs = [S.tables.real_series(int(k[7:9]), "test") for k in keys]
row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
cfgs = [S.make_config(int(k[7:9]), int(row0[i]), tabs[i].shape[0]) for i, k in enumerate(keys)]
Tb = min(t.shape[0] for t in tabs) - 1
F.solve(tabs, cfgs, 1, 24, F.Grid(), want_argmax=False)
_, batch_ms = timed(lambda: F.solve(tabs, cfgs, 1, Tb, F.Grid(), want_argmax=False))

doc = {"what": "perfect-foresight controller (exact DP of step! on a state grid, 17 x 17 action targets) next to the rule-based controller, "
               "from the reset!(rng = -1) start over each whole series",
       "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
       "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
       "timing_method": "HIP events around foresight.solve (one launch per hour, no host synchronisation) and around foresight.track "
                        "(one launch + the copies of its results), each after a warm-up call; one run, no repetition",
       "mpc_note": "mpc_profit_total is the reference MPC's own objective value on the same series (p_sell * PV_GR - p_buy * (GR_DE + GR_EV), "
                   "linear SoC dynamics, EX_EV priced at costfactor * p_buy in its objective): a neighbour of `profit`, not its equal",
       "not_a_bound": "a discretised value function with a greedy policy is not an upper bound; V0_minus_return shows the discretisation error",
       "batch_of_test_series": {"problems": len(keys), "hours": Tb, "grid": "65x33", "solve_ms": batch_ms,
                                "evaluations": len(keys) * Tb * F.Grid().nodes * F.Grid().actions},
       "series": series}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
for k, v in series.items():
    g = v["grids"]["65x33"]
    print(f"{k:28s} rule {v['rule_based_return']:10.2f}  foresight {g['foresight_return']:10.2f}  V0-ret {g['V0_minus_return']:8.3f}  "
          f"profit {g['profit']:9.2f}  mpc {v.get('mpc_profit_total', float('nan')):9.2f}  solve {g['solve_ms']:8.1f} ms  track {g['track_ms']:7.1f} ms")
print("batch", doc["batch_of_test_series"])

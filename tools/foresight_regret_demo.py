"""WHERE does a controller lose against perfect foresight?  The hourly regret of the rule-based pass and of the receding-horizon pass
(H = 24, a fresh plan every hour) audited against the perfect-foresight values, on every series this project holds (not a benchmark,
not a test).

For the 15 real exogenous series of data/mpc_series.npz and the synthetic Charger98 splits, from the reset!(rng = -1) start over the
whole series at the default grid (65 x 33 nodes, 17 x 17 targets): one foresight.solve, the two passes, ONE foresight.audit of both;
per pass Audit.summary() (return, sum of regret, sum of discretisation, regret by EV phase) and the regret summed by hour of the series
modulo 24 (row 1 = hour 0).  Regret is not a bound: the rule-based controller acts off the action grid, and single hours can be
slightly negative; nothing about sign or order is asserted.

Speed, one process: the HIP-event time of foresight.audit -- device-resident rows, the launch and the one copy back -- and of the launch
alone (shems_foresight_audit_dev into preallocated buffers), each after a warm-up call, the median of five calls alternated with
foresight.track for the same passes (which evaluates the same number of Q's, serially by hour, and copies its rows back):
1 pass x 2 998 hours (Charger98 test) and 80 passes x 1 439 hours (the synthetic Charger98 eval table, 80 start values of Soc_b).

    python tools/foresight_regret_demo.py [out.json]    (default profiles/r13_foresight_regret.json; needs the GPU, does not read oracle/)
"""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
F = importlib.import_module(PKG + ".foresight")
H = importlib.import_module(PKG + ".harness")

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_foresight_regret.json")
GRID = F.Grid()
HORIZON = 24


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def one_series(cid, tab):
    T = tab.shape[0] - 1
    env = S.ShemsBatch(1, T, [tab], [S.make_config(cid, 0, tab.shape[0])]).use_torch_stream()
    values = H.foresight_values(env, GRID)
    _, rule = H.inference(env, track=-1)
    pf_total, _ = H.inference_foresight(env, values=values)
    _, hor = H.inference_foresight(env, GRID, horizon=HORIZON)
    a = H.regret_of(env, np.stack([rule, hor[0]]), values=values)
    s = a.summary()
    hod = np.arange(T) % 24
    doc = {"charger": cid, "hours": T, "perfect_foresight_return": float(pf_total[0]), "V0_at_start": float(a.v_state[0, 0]), "passes": {}}
    for k, name in enumerate(("rule_based", f"horizon_h{HORIZON}")):
        doc["passes"][name] = {**{key: float(v[k]) for key, v in s.items()},
                               "hours_regret_positive": int((a.regret[k] > 0).sum()), "hours_regret_zero": int((a.regret[k] == 0).sum()),
                               "hours_regret_negative": int((a.regret[k] < 0).sum()), "largest_hour": float(a.regret[k].max()),
                               "most_negative_hour": float(a.regret[k].min()),
                               "hours_by_phase": {p: int((a.phase[k] == i).sum()) for i, p in enumerate(F.PHASES)},
                               "regret_by_hour_mod_24": [float(a.regret[k][hod == h].sum()) for h in range(24)]}
    env.close()
    return doc


def speed_case(name, tab, n):
    """audit next to track for the same n passes over the whole series: warm-up, then five alternated calls of each."""
    T = tab.shape[0] - 1
    cfg = S.make_config(98, 0, tab.shape[0])
    env = S.ShemsBatch(n, T, [tab], [cfg]).use_torch_stream()
    values = H.foresight_values(env, GRID)
    env.reset_(-1)
    start = env.state.copy()
    if n > 1:
        start[:, 0] = np.linspace(0.0, float(cfg.soc_max), n).astype(np.float32)

    def track():
        env.state, env.idx, env.step = start, np.ones(n, np.int32), np.zeros(n, np.int32)
        return timed(lambda: F.track(env, values))

    (_, res, _), _ = track()
    d_res = torch.from_numpy(res).cuda()
    L = F._declare(S._capi.lib())
    out = torch.empty((n, T, 3), dtype=torch.float64, device="cuda")
    act = torch.empty((n, T), dtype=torch.int32, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    g = GRID.struct()

    def launch():
        S._capi.check(L.shems_foresight_audit_dev(C.c_void_p(env.view().tables), int(values.total_rows), C.c_void_p(values.d_problems.data_ptr()),
                                                  1, C.byref(g), T, C.c_void_p(values.V.data_ptr()), values.V.numel(), C.c_void_p(d_res.data_ptr()),
                                                  n, None, C.c_void_p(out.data_ptr()), C.c_void_p(act.data_ptr()), C.c_void_p(status.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    a0 = F.audit(values, d_res)
    launch()
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[..., 0].view(np.uint64) == a0.best_q.view(np.uint64)).all() and int(status.abs().sum()) == 0
    t_call, t_launch, t_track = [], [], []
    for _ in range(5):
        t_call.append(timed(lambda: F.audit(values, d_res))[1])
        t_track.append(track()[1])
        t_launch.append(timed(launch)[1])
    env.close()
    return {"series": name, "passes": n, "hours": T, "q_evaluations": n * T * GRID.actions,
            "audit_call_ms": statistics.median(t_call), "audit_launch_ms": statistics.median(t_launch), "track_call_ms": statistics.median(t_track),
            "audit_call_ms_all": t_call, "audit_launch_ms_all": t_launch, "track_call_ms_all": t_track,
            "largest_abs_regret_of_the_tracked_passes": float(np.abs(a0.regret).max())}


spd = {"grid": "65x33x17x17",
       "timing_note": "HIP events on the current stream around the whole Python call (audit: device-resident rows, buffer allocation, status "
                      "memset, the launch, one copy back; track: the launch and the copy back of its rows) and around the entry point alone "
                      "(audit_launch_ms); one warm-up call each, then the median of five calls, audit / track / launch alternated, one process",
       "cases": [speed_case("Charger98_test", S.tables.real_series(98, "test"), 1), speed_case("synthetic_Charger98_eval", S.tables.synthetic_table("eval", 98), 80)]}
print("speed", json.dumps(spd), flush=True)
series = {}
for key in S.tables.real_series_keys():
    cid, split = int(key[7:9]), key.split("_")[1]
    series[key] = one_series(cid, S.tables.real_series(cid, split))
for split in ("train", "eval", "test"):
    series[f"synthetic_Charger98_{split}"] = one_series(98, S.tables.synthetic_table(split, 98))

props = torch.cuda.get_device_properties(0)
doc = {"what": "hourly regret (best Q over the 17 x 17 action grid from the state the pass was in, minus the Q the pass achieved; V of the exact DP "
               "of step! on 65 x 33 nodes) of the rule-based pass and of the receding-horizon pass (H = 24, c = 1) against perfect foresight, from "
               "the reset!(rng = -1) start over each whole series",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "not_a_bound": "regret can be slightly negative in single hours for a controller acting off the action grid; nothing is asserted",
       "identity": "sum of regret = V0_at_start + discretisation[0] - return + sum_{t >= 1} discretisation (best_q[0] = v_state[0] + discretisation[0])",
       "hour_mod_24": "hour of the series modulo 24, row 1 = hour 0", "speed": spd, "series": series}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
for k, v in series.items():
    r, h = v["passes"]["rule_based"], v["passes"][f"horizon_h{HORIZON}"]
    print(f"{k:28s} perfect {v['perfect_foresight_return']:9.2f} | rule {r['return']:9.2f} regret {r['regret']:8.2f} (absent {r['absent']:7.2f} arrival "
          f"{r['arrival']:7.2f} connected {r['connected']:7.2f} departure {r['departure']:7.2f}) | h{HORIZON} {h['return']:9.2f} regret {h['regret']:8.2f}")

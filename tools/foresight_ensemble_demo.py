"""Does HEDGING over several forecasts help the receding-horizon foresight controller?  The controller on the 7-member analog ensemble
(the same hour on each of the last seven days, equal weights) next to the same controller on the true rows and on the one
persistence forecast at lag 24, and to the two yardsticks, on every series this project holds (not a benchmark, not a test).

For the 15 real exogenous series of data/mpc_series.npz and the synthetic Charger98 splits, from the reset!(rng = -1) start over the
whole series at the default grid (65 x 33 nodes, 17 x 17 targets), at (H, c) = (24, 1) and the day-ahead plan (24, 24):
    the return on the true rows, on persistence lag 24 (load + PV, and all four columns), on the analog ensemble (the same two column
    sets), and the rule-based and perfect-foresight returns;
    for the Charger98 test series, Audit.summary() of the persistence pass and of the ensemble pass by EV phase.
Nothing about the order of those returns is asserted: the ensemble controller is the two-stage scenario programme, optimistic about
what is learnt after the first decision, and on a discretised V a wrong forecast can beat the true one.

Speed, on the Charger98 test series (2 998 hours), one process, HIP events, one warm-up call, the median of five calls alternated with
the comparison: the ensemble forward pass (k_fs_track_ens) at K = 1 and K = 7 against foresight.track on forecast values
(k_fs_track, fc = 1); the solve of 7 records in one call against 7 separate calls.

    python tools/foresight_ensemble_demo.py [out.json]    (default profiles/r14_foresight_ensemble.json; needs the GPU, does not read oracle/)
"""
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

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_foresight_ensemble.json")
GRID = F.Grid()
CASES = [(24, 1), (24, 24)]
LAG = 24
LAGS = F.ANALOG_LAGS
K = len(LAGS)
LOAD_PV = ("electkwh", "PV_generation")
ALL4 = LOAD_PV + F.EV_COLUMNS


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def tables_of(tab):
    """[truth, persistence lp, persistence all, 7 analog lp, 7 analog all] and the positions of the two ensembles."""
    tabs = [tab, F.persistence_forecast(tab, LAG, LOAD_PV), F.persistence_forecast(tab, LAG, ALL4)]
    tabs += F.analog_scenarios(tab, LAGS, LOAD_PV) + F.analog_scenarios(tab, LAGS, ALL4)
    return tabs, list(range(3, 3 + K)), list(range(3 + K, 3 + 2 * K))


def parts(tot, res):
    return {"return": float(tot[0]), "profit": float(res[0][:, 6].sum()), "discomfort": float(res[0][:, 7].sum()), "penalty": float(res[0][:, 8].sum())}


def one_series(cid, tab, audit=False):
    T = tab.shape[0] - 1
    cfg = S.make_config(cid, 0, tab.shape[0])
    tabs, ens_lp, ens_all = tables_of(tab)
    env = S.ShemsBatch(1, T, tabs, [cfg]).use_torch_stream()
    rule_total, _ = H.inference(env, track=-1)
    values = H.foresight_values(env, GRID)
    pf_total, _ = H.inference_foresight(env, values=values)
    doc = {"charger": cid, "hours": T, "lag": LAG, "analog_lags": list(LAGS), "rule_based_return": float(rule_total[0]),
           "perfect_foresight_return": float(pf_total[0]), "cases": {}}
    for h, c in CASES:
        row = {"horizon": h, "control": c}
        kept = {}
        for name, kw in (("truth", {}), ("persistence_load_pv", dict(forecast_table=1)), ("persistence_all", dict(forecast_table=2)),
                         ("ensemble_load_pv", dict(scenario_tables=ens_lp)), ("ensemble_all", dict(scenario_tables=ens_all))):
            tot, res = H.inference_foresight(env, GRID, horizon=h, control=c, **kw)
            row[name] = parts(tot, res)
            kept[name] = res[0]
        if audit:                                                            # where do the two passes lose against perfect foresight?
            names = ("persistence_load_pv", "ensemble_load_pv", "persistence_all", "ensemble_all")
            s = H.regret_of(env, np.stack([kept[n] for n in names]), values=values).summary()
            row["audit"] = {n: {key: float(v[k]) for key, v in s.items()} for k, n in enumerate(names)}
        doc["cases"][f"h{h}" + (f"_c{c}" if c != 1 else "")] = row
    env.close()
    return doc


def speed():
    tab = S.tables.real_series(98, "test")
    T = tab.shape[0] - 1
    cfg = S.make_config(98, 0, tab.shape[0])
    tabs, ens_lp, _ = tables_of(tab)
    env = S.ShemsBatch(1, T, tabs, [cfg]).use_torch_stream()
    h, c = 24, 1
    fc = F.solve_horizon(env, [cfg], 1, T, h, c, GRID, want_argmax=False, forecast_table=[ens_lp[0]])
    e1 = F.solve_ensemble(env, [cfg], 1, T, h, c, scenarios=[ens_lp[:1]], grid=GRID)
    e7 = F.solve_ensemble(env, [cfg], 1, T, h, c, scenarios=[ens_lp], grid=GRID)

    def run(values):
        env.reset_(-1)
        return timed(lambda: F.track(env, values, which=0))

    base, _ = run(fc)
    one, _ = run(e1)
    run(e7)
    assert (base[1].view(np.uint64) == one[1].view(np.uint64)).all()        # K = 1 is the forecast pass, byte for byte
    t_fc, t_1, t_7 = [], [], []
    for _ in range(5):
        t_fc.append(run(fc)[1]); t_1.append(run(e1)[1]); t_7.append(run(e7)[1])
    del fc, e1, e7

    def together():
        return F.solve_ensemble(env, [cfg], 1, T, h, c, scenarios=[ens_lp], grid=GRID)

    def apart():
        return [F.solve_horizon(env, [cfg], 1, T, h, c, GRID, want_argmax=False, forecast_table=[k]) for k in ens_lp]

    timed(together); timed(apart)
    s_one, s_sep = [], []
    for _ in range(5):
        s_one.append(timed(together)[1]); s_sep.append(timed(apart)[1])
    env.close()
    med = statistics.median
    return {"series": "Charger98_test", "hours": T, "grid": "65x33x17x17", "horizon": h, "control": c, "scenarios": K,
            "timing_note": "HIP events on the current stream around the whole Python call (track: allocation of its buffers, the launch, the copy "
                           "back of one env's rows; solve: allocation of V, upload of the records, the launch); one warm-up call each, then the "
                           "median of five calls, the variants alternated, one process",
            "track_forecast_ms": med(t_fc), "track_ensemble_k1_ms": med(t_1), "track_ensemble_k7_ms": med(t_7),
            "k7_over_k1": med(t_7) / med(t_1), "k1_over_forecast": med(t_1) / med(t_fc),
            "solve_7_records_one_call_ms": med(s_one), "solve_7_calls_ms": med(s_sep), "one_call_over_7_calls": med(s_one) / med(s_sep),
            "all": {"track_forecast_ms": t_fc, "track_ensemble_k1_ms": t_1, "track_ensemble_k7_ms": t_7, "solve_one_call_ms": s_one, "solve_7_calls_ms": s_sep}}


spd = speed()
print("speed", json.dumps(spd), flush=True)
series = {}
for key in S.tables.real_series_keys():
    cid, split = int(key[7:9]), key.split("_")[1]
    series[key] = one_series(cid, S.tables.real_series(cid, split), audit=(cid == 98 and split == "test"))
    print(key, json.dumps(series[key]["cases"]["h24"]["ensemble_load_pv"]), flush=True)
for split in ("train", "eval", "test"):
    series[f"synthetic_Charger98_{split}"] = one_series(98, S.tables.synthetic_table(split, 98))

props = torch.cuda.get_device_properties(0)
doc = {"what": "receding-horizon foresight controller (H = 24 hours of forecast, a fresh plan every c hours; exact DP of step! on 65 x 33 nodes, "
               "17 x 17 action targets) hedging over the 7-member analog ensemble (lags 24 .. 168 h, equal weights), next to the same controller on "
               "the true rows and on persistence at lag 24, between the rule-based and the perfect-foresight controller, from the reset!(rng = -1) "
               "start over each whole series",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "no_order_asserted": "the ensemble controller is the two-stage scenario programme (optimistic about what is learnt after the first decision); "
                            "the figures are reported, not asserted",
       "causality": "the analog ensemble and persistence at lag 24 are causal for H <= 24",
       "speed": spd, "series": series}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
for k, v in series.items():
    print(f"{k:28s} rule {v['rule_based_return']:9.2f} " +
          " ".join(f"{n} truth {d['truth']['return']:8.2f} p-lp {d['persistence_load_pv']['return']:8.2f} e-lp {d['ensemble_load_pv']['return']:8.2f} "
                   f"p-all {d['persistence_all']['return']:8.2f} e-all {d['ensemble_all']['return']:8.2f}" for n, d in v["cases"].items())
          + f"  perfect {v['perfect_foresight_return']:9.2f}")

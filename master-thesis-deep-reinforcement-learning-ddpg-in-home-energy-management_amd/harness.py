"""Evaluation / tracking harness and on-disk formats.

Reference: inference() (memory_plotting_saving.jl:62-89), write_to_results_file (:167-190),
write_to_tracker_file (:193-212).  File names, column headers and column order are the reference's, so the
thesis notebooks that read `out/tracker/*.csv` and `out/Tracker_Charger.csv` keep working.
"""
from __future__ import annotations

import csv
import ctypes as C
import datetime
import os

import numpy as np

from . import _capi

RESULTS_HEADER = ["index", "c_ev", "EV_target", "EV", "Soc_ev", "rewards", "profit", "discomfort", "penalty", "PV_DE",
                  "B_DE", "GR_DE", "PV_B", "PV_GR", "PV_EV", "B_EV", "GR_EV", "EX_EV", "GR_B", "B_GR", "B", "B_tar", "Soc_b"]
TRACKER_HEADER = ["time", "NUM_EP", "L1", "L2", "BATCH_SIZE", "MEM_SIZE", "MIN_EXP_SIZE", "season", "run", "Job_ID", "seed",
                  "case", "best", "idx", "rewards", "profit", "discomfort", "penalty", "filename"]


def inference(env, agent=None, track=1, num_steps=None, which=0):
    """inference(env; track != 0): one deterministic pass over the data set from reset!(rng = -1)
    (MPS:66-71 -> episode!(..., train=false, track, rng_ep=-1), DDPG.jl:186-242).  track > 0: the actor's
    actions (no noise); track < 0: the rule-based controller action(env, track).  Every env of the batch runs the
    same pass; returns (sum of rewards [N], results [steps][23] float64 of env `which`).

    ONE launch (shems_track_dev: all hours inside the kernel, one workgroup per env) and ONE device-to-host copy of the
    results rows -- no launch, synchronisation or copy per hour."""
    if track > 0 and agent is None:
        raise ValueError("track > 0 needs an agent")
    total, res = _track(env, None if track < 0 else agent.actor, None if track < 0 else agent.s_min, None if track < 0 else agent.s_max,
                        0, track, num_steps, which, hidden=agent.hidden if track > 0 and agent.wide else None)
    return total, res[0]


def inference_many(env, actors, s_min, s_max, num_steps=None, hidden=None):
    """The job's tracking passes in one launch (MAIN:87-105: 40 seeds x {last, best} actor, each a full pass over the data set):
    env e of the batch (len(actors) envs on the same table) runs the pass with actors[e].  actors: [P][129002] float32 (numpy or a
    CUDA tensor); s_min / s_max: [9] (shared) or [P][9].  Returns (sum of rewards [P], results [P][steps][23] float64).
    hidden: (L1, L2) of a network wider than (250, 500) -- the actors then hold that network's own parameter count (ddpg.is_wide)."""
    import torch
    from .ddpg import is_wide, net_size
    wide = hidden is not None and is_wide(hidden)
    na = net_size(9, 2, hidden) if wide else 129002
    dev = torch.device("cuda", torch.cuda.current_device())
    A = torch.as_tensor(np.asarray(actors, np.float32) if not torch.is_tensor(actors) else actors, dtype=torch.float32, device=dev)
    P = A.shape[0]
    if A.dim() != 2 or A.shape[1] != na or env.n != P:
        raise ValueError(f"actors must be [P][{na}] with one env of the batch per actor")
    # one slab row per pass: actor | pad to 16 B | s_min[9] | s_max[9] | pad -- env e finds all three at the same byte stride
    row = -(-na // 4) * 4 + 32
    slab = torch.zeros((P, row), dtype=torch.float32, device=dev)
    slab[:, :na] = A
    o_min, o_max = row - 32, row - 16
    for off, val in ((o_min, s_min), (o_max, s_max)):
        t = torch.as_tensor(np.asarray(val, np.float32) if not torch.is_tensor(val) else val, dtype=torch.float32, device=dev)
        slab[:, off:off + 9] = t if t.dim() == 2 else t[None, :]
    return _track(env, slab[0, :na], slab[0, o_min:o_min + 9], slab[0, o_max:o_max + 9], row * 4, 1, num_steps, -1, keep=slab,
                  hidden=hidden if wide else None)


def _track(env, actor, s_min, s_max, stride, track, num_steps, which, keep=None, hidden=None):
    import torch
    from .ddpg import ActParams, _declare
    _declare()
    n = env.n
    num_steps = env.maxsteps if num_steps is None else int(num_steps)
    env.use_torch_stream()
    env.reset_(-1)
    L = _capi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = n if which < 0 else 1
    res = torch.empty((rows, num_steps, _capi.NRESULT), dtype=torch.float64, device=dev)
    total = torch.empty(n, dtype=torch.float64, device=dev)
    v = env.view()
    p = None
    if track > 0:
        p = ActParams(actor.data_ptr(), s_min.data_ptr(), s_max.data_ptr(), 0.0, 0.0, 0, 0, 0, 0, 0.0, 0.0, 0.0, None, None)
    if track > 0 and hidden is not None:                        # a wide actor (or one forced onto the wide path): its own flat layout
        L.shems_wide_track_dev.argtypes = [C.POINTER(_capi.View), C.POINTER(ActParams), C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.shems_wide_track_dev.restype = C.c_int
        _capi.check(L.shems_wide_track_dev(C.byref(v), C.byref(p), int(hidden[0]), int(hidden[1]), int(stride), num_steps,
                                           C.c_void_p(res.data_ptr()), int(which), C.c_void_p(total.data_ptr()), env._stream()))
    else:
        _capi.check(L.shems_track_dev(C.byref(v), C.byref(p) if p is not None else None, int(stride), 1 if track > 0 else -1, num_steps,
                                      C.c_void_p(res.data_ptr()), int(which), C.c_void_p(total.data_ptr()), env._stream()))
    out, tot = res.cpu().numpy(), total.cpu().numpy()           # the pass's one synchronisation
    env.check_error()
    return tot, out


def foresight_values(env, grid=None):
    """The perfect-foresight solve of inference_foresight on its own: reset!(rng = -1) and the backward sweep for the env's table(s)
    over env.maxsteps hours from row 1, one problem per distinct config of the batch.  The Values serve inference_foresight(values=...)
    and any number of regret_of calls."""
    from . import foresight
    env.use_torch_stream()
    env.reset_(-1)
    cfgs, idx0, _ = foresight.problems_of_env(env, np.ones(env.n, np.int64))
    return foresight.solve(env, cfgs, idx0, env.maxsteps, grid, want_argmax=False)


def inference_foresight(env, grid=None, horizon=None, control=1, forecast_table=None, values=None, scenario_tables=None, weights=None):
    """The perfect-foresight pass over the data set: reset!(rng = -1), the backward sweep for the env's table(s) over env.maxsteps
    hours (foresight.solve: one problem per distinct config of the batch) and the greedy forward pass on the exact env
    (foresight.track), which steps the envs with the ordinary DRL step (track > 0: penalty kept, 23-column rows).  Returns what
    inference_many returns -- (sum of rewards [N], results [N][steps][23] float64) -- so the file writers take it.  horizon: the
    receding-horizon controller instead (foresight.solve_horizon: `horizon` hours of forecast, a fresh plan every `control` hours).
    forecast_table (needs a horizon): the plans read a forecast instead of the true future rows -- one index into the env's own
    tables for every problem, or one entry (index or None) per distinct config of the batch in ascending config order, as
    foresight.problems_of_env lists them; foresight.append_forecasts builds such a table list.
    values: the Values of foresight_values(env, grid) (or of any solve for this batch's problems from row 1) to reuse instead of
    solving again; grid, horizon, control and forecast_table are then not read.
    scenario_tables (needs a horizon, excludes forecast_table): the controller hedges over a forecast ensemble
    (foresight.solve_ensemble) -- the indices of the K scenario tables among the env's own tables for every problem, or one such list
    per distinct config; foresight.append_scenarios builds such a table list.  weights: as solve_ensemble (None: equal)."""
    from . import foresight
    env.use_torch_stream()
    env.reset_(-1)
    cfgs, idx0, poe = foresight.problems_of_env(env, np.ones(env.n, np.int64))
    if forecast_table is not None and horizon is None:
        raise ValueError("a forecast table needs a horizon (the perfect-foresight pass knows the whole series)")
    if scenario_tables is not None or weights is not None:
        if scenario_tables is None:
            raise ValueError("weights need scenario_tables")
        if horizon is None:
            raise ValueError("scenario tables need a horizon (the perfect-foresight pass knows the whole series)")
        if forecast_table is not None:
            raise ValueError("scenario_tables and forecast_table exclude each other (one forecast table is an ensemble of one)")
    if values is not None:
        pass
    elif scenario_tables is not None:
        scen = list(scenario_tables)
        if not scen or np.ndim(scen[0]) == 0:
            scen = [scen] * len(cfgs)
        values = foresight.solve_ensemble(env, cfgs, idx0, env.maxsteps, horizon, control, scenarios=scen, weights=weights, grid=grid)
    elif horizon is None:
        values = foresight.solve(env, cfgs, idx0, env.maxsteps, grid, want_argmax=False)
    else:
        if forecast_table is not None and np.ndim(forecast_table) == 0:
            forecast_table = [forecast_table] * len(cfgs)
        values = foresight.solve_horizon(env, cfgs, idx0, env.maxsteps, horizon, control, grid, want_argmax=False, forecast_table=forecast_table)
    total, results, _ = foresight.track(env, values, poe, which=-1)
    return total, results


REGRET_HEADER = ["index", "Soc_b", "Soc_ev", "c_ev", "rewards", "achieved_q", "best_q", "regret", "v_state", "best_B_tar", "best_EV_tar"]


def regret_of(env, results, values=None, grid=None):
    """The hourly regret of tracked passes of `env`'s data set against perfect foresight (foresight.audit): results is one pass
    [steps][23] (harness.inference, a results file read back) or [P][steps][23] (inference_many, inference_foresight), every pass
    from reset!(rng = -1) over env.maxsteps hours.  A batch with several configs needs one pass per env (pass e is env e's).  values:
    foresight_values(env, grid) to reuse (solved here when None).  Returns a foresight.Audit.  Regret is not a bound: a controller
    acting off the action grid can reach slightly negative values."""
    from . import foresight
    if values is None:
        values = foresight_values(env, grid)
    n = 1 if np.ndim(results) == 2 else int(np.shape(results)[0])
    _, _, poe = foresight.problems_of_env(env, np.ones(env.n, np.int64))
    po = None
    if values.n_problems > 1:
        if n != env.n:
            raise ValueError(f"the batch holds {values.n_problems} problems: regret_of needs one pass per env ({env.n}), not {n}")
        po = poe
    return foresight.audit(values, results, po)


def regret_file_name(results_path):
    """The regret file of a results file: its name with _regret before .csv."""
    root, ext = os.path.splitext(results_path)
    return root + "_regret" + (ext or ".csv")


def write_to_regret_file(audit, results, path, pass_index=0):
    """One pass of an audit as a CSV next to its results file: per hour the row index, the state the pass was in, its reward, the Q it
    achieved, the best Q of the action grid from that state, their difference, V_t at the state and the targets of the best action.
    results: the rows the audit was made of ([steps][23], or [P][steps][23] with pass_index naming the pass)."""
    res = np.asarray(results, np.float64)
    res = res[pass_index] if res.ndim == 3 else res
    e = int(pass_index)
    if res.ndim != 2 or res.shape[1] != len(RESULTS_HEADER) or res.shape[0] != audit.regret.shape[1]:
        raise ValueError(f"results must be the [steps][23] rows of the audited pass ({audit.regret.shape[1]} hours)")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(REGRET_HEADER)
        for t, r in enumerate(res):
            w.writerow([repr(float(x)) for x in (r[0], r[22], r[4], r[1], r[5], audit.achieved_q[e, t], audit.best_q[e, t], audit.regret[e, t],
                                                 audit.v_state[e, t], audit.best_targets[e, t, 0], audit.best_targets[e, t, 1])])
    return path


def foresight_seed(horizon=None, control=1, forecast=None):
    """The tracker's seed column (and the file-name suffix) of a foresight pass: foresight, foresight_h24, foresight_h24_c12; with a
    persistence forecast -- forecast = lag, or (lag, ev) with ev true when the EV columns are forecast too -- foresight_h24_p24,
    foresight_h24_c12_p24ev; with the analog ensemble -- forecast = ("analog", lags, ev) -- foresight_h24_a24-48-72, ..._a24-48-72ev."""
    if horizon is None:
        if forecast is not None:
            raise ValueError("a forecast needs a horizon")
        return "foresight"
    name = f"foresight_h{int(horizon)}" + (f"_c{int(control)}" if int(control) != 1 else "")
    if isinstance(forecast, (tuple, list)) and len(forecast) == 3 and forecast[0] == "analog":
        lags = [int(l) for l in forecast[1]]
        if not lags:
            raise ValueError("an analog ensemble needs at least one lag")
        name += "_a" + "-".join(str(l) for l in lags) + ("ev" if forecast[2] else "")
    elif forecast is not None:
        lag, ev = forecast if isinstance(forecast, (tuple, list)) else (forecast, False)
        name += f"_p{int(lag)}" + ("ev" if ev else "")
    return name


def foresight_file_name(job_id, run, case, out_dir="out/tracker", horizon=None, control=1, forecast=None):
    """The results file of the perfect-foresight pass, next to the rule-based one of results_file_name; with a horizon, of the
    receding-horizon pass: ..._foresight_h{H}.csv, ..._foresight_h{H}_c{c}.csv when control != 1; with a persistence forecast
    (forecast = lag or (lag, ev), see foresight_seed) ..._foresight_h{H}[_c{c}]_p{lag}.csv, _p{lag}ev when the EV columns are forecast;
    with the analog ensemble (forecast = ("analog", lags, ev)) ..._foresight_h{H}[_c{c}]_a{lag}-{lag}-....csv, `ev` appended likewise."""
    return os.path.join(out_dir, f"{job_id}_{run}_results_{case}_{foresight_seed(horizon, control, forecast)}.csv")


def results_file_name(job_id, run, ep_len, num_ep, l1, l2, case, rng, idx, best=False, out_dir="out/tracker"):
    """File names of write_to_results_file (MPS:170-187)."""
    if best:
        return os.path.join(out_dir, f"{job_id}_{run}_results_charger_v1_{ep_len}_{num_ep}_{l1}_{l2}_{case}_{rng}_best.csv")
    if isinstance(idx, (int, np.integer)) and idx == num_ep:
        return os.path.join(out_dir, f"{job_id}_{run}_results_charger_v1_{ep_len}_{num_ep}_{l1}_{l2}_{case}_{rng}_{idx}.csv")
    return os.path.join(out_dir, f"{job_id}_{run}_results_{case}_rule_{idx}.csv")


def write_to_results_file(results, path):
    """CSV.write(path, DataFrame(results), header = the 23 names) (MPS:167-190)."""
    results = np.asarray(results, np.float64)
    if results.ndim != 2 or results.shape[1] != len(RESULTS_HEADER):
        raise ValueError("results must be [steps][23]")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(RESULTS_HEADER)
        for row in results:
            w.writerow([repr(float(x)) for x in row])
    return path


def write_to_tracker_file(results_path, tracker_path="out/Tracker_Charger.csv", *, num_ep, l1=250, l2=500, batch_size=120,
                          mem_size=24000, min_exp_size=24000, season="all", run="eval", job_id=0, seed=0, case="", best=False,
                          idx=0, now=None):
    """Append one row of KPI sums to the overall tracker (MPS:193-212): sums of the rewards / profit / discomfort /
    penalty columns of a results file."""
    with open(results_path, newline="") as fh:
        rd = csv.DictReader(fh)
        sums = {k: 0.0 for k in ("rewards", "profit", "discomfort", "penalty")}
        for row in rd:
            for k in sums:
                sums[k] += float(row[k])
    rows = []
    if os.path.exists(tracker_path):
        with open(tracker_path, newline="") as fh:
            rows = list(csv.reader(fh))[1:]
    now = datetime.datetime.now().isoformat(timespec="milliseconds") if now is None else now
    rows.append([now, num_ep, l1, l2, batch_size, mem_size, min_exp_size, season, run, job_id, seed, case, str(bool(best)).lower(), idx,
                 repr(sums["rewards"]), repr(sums["profit"]), repr(sums["discomfort"]), repr(sums["penalty"]), results_path])
    os.makedirs(os.path.dirname(tracker_path) or ".", exist_ok=True)
    with open(tracker_path, "w", newline="") as fh:            # the reference rewrites the whole file as well
        w = csv.writer(fh)
        w.writerow(TRACKER_HEADER)
        w.writerows(rows)
    return sums

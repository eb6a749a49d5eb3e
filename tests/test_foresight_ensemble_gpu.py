"""The receding-horizon foresight controller hedging over a forecast ensemble, on the GPU (foresight.solve_ensemble: K records of
shems_foresight_solve_forecast_dev; shems_foresight_track_ensemble_dev, k_fs_track_ens): every choice against the NumPy controller of
foresight_ensemble_ref on the oracle along the device's own trajectory, the identities with the single-forecast pass (K = 1, one
scenario twice), K = 16, crafted planes that pin WHICH scenario's next row every lookup reads, four problems in scrambled order, the
refusals inside the kernel, and the host layers on top."""
import csv
import importlib
import os

import numpy as np
import pytest

import foresight_ensemble_ref as ER
import foresight_horizon_ref as FR
import foresight_twin as FT
import util as U

pytestmark = pytest.mark.gpu

W3 = (0.5, 0.25, 0.25)


def _grid(F, shape):
    return F.Grid(shape["nb"], shape["ne"], shape["nab"], shape["nae"])


def _starts(prof):
    """The six starts of the forecast test: Soc_b = 0, soc_max, the rng = -1 midpoint, three Philox draws."""
    return importlib.import_module("test_foresight_forecast_gpu")._starts(prof)


def _tabs_s1(specs):
    return [FT.s1()["tab"]] + [ER.scenario("s1", 0, s) for s in specs]


_SOLVED = {}
S1_ACTIONS = (FT.S1["nab"], FT.S1["nae"])
ACTION_GRIDS = [(5, 3), (9, 9), (17, 17)]    # 15 actions (S1's own); 81: two waves, the second partial; 289: more than the 256 threads


def _solve_s1(specs, w, H, c, actions=S1_ACTIONS):
    """EnsembleValues of S1 with the scenario tables behind the truth, on S1's state grid and the action grid `actions` (default: S1's
    own), solved once per (specs, H, c, actions); the weights are set per call."""
    S, F = U.pkg(), FT.F()
    key = (specs, H, c, actions)
    if key not in _SOLVED:
        _SOLVED[key] = F.solve_ensemble(_tabs_s1(specs), FT.configs(S, "s1"), FT.s1()["idx0"], FT.S1["T"], H, c,
                                        scenarios=[list(range(1, len(specs) + 1))], grid=_grid(F, dict(FT.S1, nab=actions[0], nae=actions[1])))
    base = _SOLVED[key]
    return F.EnsembleValues(base.values, len(specs), F.ensemble_weights(w, 1, len(specs)))


def _env_s1(S, tabs, soc=None):
    d = FT.s1()
    soc = _starts(d["prof"]) if soc is None else np.asarray(soc, np.float32)
    n = len(soc)
    idx = np.full(n, d["idx0"], np.int32)
    env = S.ShemsBatch(n, FT.S1["T"], tabs, FT.configs(S, "s1"))
    env.state, env.idx, env.step = U.obs_of_rows(d["tab"], idx, soc), idx, np.zeros(n, np.int32)
    return env


def _check_against_numpy(env, totals, res, tg, specs, w, V, actions=None):
    """All choices, the rows and rewards replayed through the oracle bitwise, the ordered float64 totals, final state, idx and step."""
    d, T = FT.s1(), FT.S1["T"]
    run = ER.controller("s1", 0, specs, w, V, _starts(d["prof"]), tg=tg, res=res, actions=actions)
    wrong = np.argwhere((run["picks"] != tg).any(axis=2))
    print(f"K = {len(specs)}, w = {tuple(w)}: {len(wrong)} of {tg.shape[0] * T} choices differ from the NumPy controller; returns {totals}")
    assert len(wrong) == 0, wrong[:10]
    assert (U.bits64(totals) == U.bits64(run["totals"])).all()
    assert (U.bits32(env.state) == U.bits32(run["ref"].state())).all()
    assert (env.idx == run["ref"].idx()).all() and (env.step == T).all() and (run["ref"].steps() == T).all()
    return run


@pytest.mark.parametrize("H, c, actions", [pytest.param(H, c, a, id=f"{H}-{c}" + ("" if a == S1_ACTIONS else f"-{a[0]}x{a[1]}"))
                                          for a in ACTION_GRIDS for H, c in [(6, 1), (6, 4)]])     # S1's own grid keeps its ids
def test_choices_equal_the_numpy_controller_on_the_oracle(H, c, actions):
    """S1, six starts, K = 3: persistence of load + PV at lags 3, 6, 9, w = (0.5, 0.25, 0.25).
    The action grid: 5 x 3 is S1's own (less than one wave holds an action; the K planes from the twin).  At 9 x 9 (two waves, the
    second partial) and 17 x 17 (289 actions on 256 threads: threads 0 .. 32 take two, all four waves contribute) the planes are the
    device's own forecast solve on that grid (the solve kernels are held to the twin elsewhere); with the EV absent every ae ties, so
    these grids also hold the first-maximum rule across lanes and across waves."""
    S, F = U.pkg(), FT.F()
    specs = ((3, "lp"), (6, "lp"), (9, "lp"))
    ens = _solve_s1(specs, W3, H, c, actions)
    g = _grid(F, dict(FT.S1, nab=actions[0], nae=actions[1]))
    assert (ens.n_scen, ens.n_problems, ens.horizon, ens.control) == (3, 1, H, c) and (U.bits64(ens.weights) == U.bits64(np.array([W3]))).all()
    n = FT.s1()["tab"].shape[0]
    assert ens.values.forecast_off == [n, 2 * n, 3 * n] and ens.values.argmax is None and ens.values.V.shape[0] == 3
    env = _env_s1(S, _tabs_s1(specs))
    totals, res, tg = F.track(env, ens, None, which=-1)
    assert res.shape == (6, 30, 23) and tg.shape == (6, 30, 2) and totals.shape == (6,)
    planes = [ER.planes("s1", 0, s, H, c) for s in specs] if actions == S1_ACTIONS else list(ens.values.V.cpu().numpy())
    _check_against_numpy(env, totals, res, tg, specs, W3, planes, actions)
    assert np.unique(tg.reshape(-1, 2), axis=0).shape[0] > 1
    # the single-forecast lag-6 controller is another one
    one = F.solve_horizon(_tabs_s1(specs), FT.configs(S, "s1"), FT.s1()["idx0"], 30, H, c, g, want_argmax=False, forecast_table=[2])
    o_env = _env_s1(S, _tabs_s1(specs))
    o_tot, _, _ = F.track(o_env, one)
    assert (U.bits64(o_tot) != U.bits64(totals)).any()
    env.close(); o_env.close()


def test_one_scenario_and_the_same_scenario_twice_leave_the_bytes_of_the_forecast_pass():
    """K = 1 at w = 1.0, and K = 2 with the same scenario twice at w = (0.5, 0.5) (0.5 v + 0.5 v is exact): results, targets and totals
    equal foresight.track on the forecast Values in every byte.  Four-column lag-6 forecast, (H, c) = (6, 1)."""
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    tabs = _tabs_s1(((6, "all"),))
    cfgs, g = FT.configs(S, "s1"), _grid(F, FT.S1)
    fc = F.solve_horizon(tabs, cfgs, d["idx0"], 30, 6, 1, g, want_argmax=False, forecast_table=[1])
    env = _env_s1(S, tabs)
    want = F.track(env, fc)
    env.close()
    for scen, w in (([1], None), ([1], [1.0]), ([1, 1], [0.5, 0.5]), ([1, 1], None)):
        ens = F.solve_ensemble(tabs, cfgs, d["idx0"], 30, 6, 1, scenarios=[scen], weights=w, grid=g)
        env = _env_s1(S, tabs)
        got = F.track(env, ens)
        env.close()
        assert (U.bits64(got[0]) == U.bits64(want[0])).all(), scen
        assert (U.bits64(got[1]) == U.bits64(want[1])).all() and (U.bits32(got[2]) == U.bits32(want[2])).all(), scen


def test_sixteen_scenarios():
    """K = 16: the four columns at lags 1 .. 16, weights 1 / 16, (H, c) = (6, 1)."""
    S, F = U.pkg(), FT.F()
    specs = tuple((lag, "all") for lag in range(1, 17))
    w = (1.0 / 16,) * 16
    ens = _solve_s1(specs, None, 6, 1)
    assert (ens.weights == 1.0 / 16).all() and ens.weights.shape == (1, 16)
    env = _env_s1(S, _tabs_s1(specs))
    totals, res, tg = F.track(env, ens)
    _check_against_numpy(env, totals, res, tg, specs, w, [ER.planes("s1", 0, s, 6, 1) for s in specs])
    env.close()


def test_every_lookup_reads_its_own_scenarios_next_row():
    """On real planes the source of the next row rarely changes a choice, so it is pinned with the crafted planes of the forecast
    test, written into every scenario's record: scenarios {a byte copy of the truth, the EV columns at lag 6}.  At both weightings
    all 180 choices equal the NumPy controller; one that reads every next row from scenario 0 differs from the (0.25, 0.75) run, one
    that reads it from the last scenario from the (0.75, 0.25) run.  On the oracle: 6 of 180 each, from hour 10, with the other
    controller asked along the device's trajectory as here (18 of 180 when it runs on from its own choices)."""
    import torch
    S, F = U.pkg(), FT.F()
    specs = (ER.TRUTH, (6, "ev"))
    planes = ER.crafted_planes("s1", 0)
    base = _solve_s1(specs, None, 6, 1)
    assert base.values.V.shape == (2, 31, 45)
    saved = base.values.V.clone()
    base.values.V.copy_(torch.from_numpy(np.stack([planes, planes])))
    try:
        for w, other in (((0.25, 0.75), "first"), ((0.75, 0.25), "last")):
            ens = _solve_s1(specs, w, 6, 1)
            env = _env_s1(S, _tabs_s1(specs))
            totals, res, tg = F.track(env, ens)
            _check_against_numpy(env, totals, res, tg, specs, w, [planes, planes])
            wrong = ER.controller("s1", 0, specs, w, [planes, planes], _starts(FT.s1()["prof"]), tg=tg, next_from=other)
            differ = np.argwhere((wrong["picks"] != tg).any(axis=2))
            print(f"w = {w}: every next row from the {other} scenario: {len(differ)} of 180 choices differ, first at hour "
                  f"{differ[:, 1].min() if len(differ) else None}")
            assert len(differ) >= 1
            env.close()
    finally:
        base.values.V.copy_(saved)


S2_SPECS = ((3, "all"), (5, "lp"))
S2_W = ((0.75, 0.25), (0.5, 0.5), (0.25, 0.75), (0.625, 0.375))
S2_POE = np.array([2, 0, 3, 1, 1, 3, 0, 2], np.int32)


def _s2_run():
    """S2's four problems, K = 2, (H, c) = (3, 2): row array [t0 .. t3, then the two scenario tables of every problem]; eight envs
    listed in scrambled problem order, the first of a problem from 0.5 soc_max, the second from 0.25 soc_max."""
    S, F = U.pkg(), FT.F()
    d = FT.s2()
    T = FT.S2["T"]
    tabs = list(d["tabs"]) + [ER.scenario("s2", p, s) for p in range(4) for s in S2_SPECS]
    scen = [[4 + 2 * p, 5 + 2 * p] for p in range(4)]
    ens = F.solve_ensemble(tabs, FT.configs(S, "s2"), d["idx0"], T, 3, 2, scenarios=scen, weights=S2_W, grid=_grid(F, FT.S2))
    seen, soc = set(), []
    for p in S2_POE:
        soc.append(np.float32((0.25 if p in seen else 0.5) * float(d["profs"][p].soc_max)))
        seen.add(p)
    soc = np.array(soc, np.float32)
    idx = np.array([d["idx0"][p] for p in S2_POE], np.int32)
    obs = np.concatenate([U.obs_of_rows(d["tabs"][p], [idx[e]], soc[e:e + 1]) for e, p in enumerate(S2_POE)])
    env = S.ShemsBatch(len(S2_POE), T, tabs, FT.configs(S, "s2"), S2_POE.astype(np.uint16))
    env.state, env.idx, env.step = obs, idx, np.zeros(len(S2_POE), np.int32)
    out = F.track(env, ens, S2_POE, which=-1)
    return ens, env, soc, out


def test_s2_four_problems_in_scrambled_order():
    """T = 8, 33 x 9 nodes, 28 actions; every problem has its own table, start row, capacity, reward weights and scenario weights."""
    ens, env, soc, (totals, res, tg) = _s2_run()
    assert ens.values.V.shape[0] == 8 and (U.bits64(ens.weights) == U.bits64(np.array(S2_W))).all()
    T = FT.S2["T"]
    for p in range(4):
        es = np.nonzero(S2_POE == p)[0]
        V = [ER.planes("s2", p, s, 3, 2) for s in S2_SPECS]
        run = ER.controller("s2", p, S2_SPECS, S2_W[p], V, soc[es], tg=tg[es], res=res[es])
        wrong = np.argwhere((run["picks"] != tg[es]).any(axis=2))
        print(f"problem {p}: {len(wrong)} of {len(es) * T} choices differ from the NumPy controller")
        assert len(wrong) == 0, (p, wrong[:10])
        assert (U.bits64(totals[es]) == U.bits64(run["totals"])).all() and (U.bits32(env.state[es]) == U.bits32(run["ref"].state())).all()
        assert (env.idx[es] == FR._problem("s2", p)[2] + T).all()
    assert (env.step == T).all()
    env.close()


def test_two_calls_leave_identical_bytes():
    _, e1, _, a = _s2_run()
    _, e2, _, b = _s2_run()
    assert (U.bits64(a[0]) == U.bits64(b[0])).all() and (U.bits64(a[1]) == U.bits64(b[1])).all() and (U.bits32(a[2]) == U.bits32(b[2])).all()
    assert (U.bits32(e1.state) == U.bits32(e2.state)).all()
    e1.close(); e2.close()


def test_the_kernel_refuses_an_env_off_its_start_row_and_a_missing_scenario_table():
    """An env off its start row raises BoundsError: its obs, idx and step are untouched, the other envs of the call are stepped.  A view
    whose row array lacks only the LAST scenario's table does the same (asked with the Python check put out of the way: the records
    may come from a solve on another array)."""
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    T = FT.S1["T"]
    specs = ((3, "lp"), (6, "lp"), (9, "lp"))
    ens = _solve_s1(specs, W3, 6, 1)
    env = _env_s1(S, _tabs_s1(specs), [0.0, 1.0, 2.0])
    idx = np.array([d["idx0"], d["idx0"] + 1, d["idx0"]], np.int32)
    obs = U.obs_of_rows(d["tab"], idx, np.array([0.0, 1.0, 2.0], np.float32))
    env.state, env.idx, env.step = obs, idx, np.array([0, 5, 0], np.int32)
    with pytest.raises(S._capi.BoundsError):
        F.track(env, ens)
    assert (env.idx == [d["idx0"] + T, d["idx0"] + 1, d["idx0"] + T]).all() and (env.step == [T, 5, T]).all()
    assert (U.bits32(env.state[1]) == U.bits32(obs[1])).all()
    env.close()
    # the truth and the first two scenario tables only
    short = _env_s1(S, _tabs_s1(specs)[:-1], [1.0])
    obs = short.state.copy()
    with pytest.raises(ValueError, match="same tables"):
        F.track(short, ens)
    n = d["tab"].shape[0]
    cut = F.EnsembleValues(F.Values(ens.values.grid, T, ens.values.problems, ens.values.d_problems, ens.values.V, None, forecast_off=ens.values.forecast_off,
                                    total_rows=3 * n), 3, ens.weights)                       # what a caller of the C ABI could hand over
    with pytest.raises(S._capi.BoundsError):
        F.track(short, cut)
    assert (U.bits32(short.state) == U.bits32(obs)).all() and (short.idx == d["idx0"]).all() and (short.step == 0).all()
    short.close()


def test_harness_inference_foresight_with_scenario_tables_and_its_file(tmp_path):
    S, F = U.pkg(), FT.F()
    H = importlib.import_module(U.PKG_NAME + ".harness")
    d = FT.s1()
    T, grid = FT.S1["T"], _grid(F, FT.S1)
    cfgs = FT.configs(S, "s1")
    tabs, index = F.append_scenarios([d["tab"]], (3, 6, 9))
    assert index == [[1, 2, 3]]
    env = S.ShemsBatch(1, T, tabs, cfgs)
    total, res = H.inference_foresight(env, grid, horizon=6, scenario_tables=index[0], weights=W3)
    assert res.shape == (1, T, 23) and total.shape == (1,)
    one = S.ShemsBatch(1, T, tabs, cfgs)
    one.reset_(-1)
    t2, r2, _ = F.track(one, F.solve_ensemble(tabs, cfgs, 1, T, 6, 1, scenarios=index, weights=W3, grid=grid))
    assert (U.bits64(res) == U.bits64(r2)).all() and (U.bits64(total) == U.bits64(t2)).all()
    tl, rl = H.inference_foresight(env, grid, horizon=6, scenario_tables=index)            # one list per distinct config, equal weights
    t0, r0 = H.inference_foresight(env, grid, horizon=6)
    assert (U.bits64(r0) != U.bits64(res)).any() and rl.shape == res.shape
    for kw, word in ((dict(scenario_tables=index[0]), "horizon"), (dict(horizon=6, scenario_tables=index[0], forecast_table=1), "exclude"),
                     (dict(horizon=6, weights=W3), "scenario_tables")):
        with pytest.raises(ValueError, match=word):
            H.inference_foresight(env, grid, **kw)
    with pytest.raises(ValueError, match="ensemble"):
        H.regret_of(env, res, values=F.solve_ensemble(tabs, cfgs, 1, T, 6, 1, scenarios=index, grid=grid))
    path = H.foresight_file_name(7, "eval", "Charger98_x", out_dir=str(tmp_path / "out" / "tracker"), horizon=6, forecast=("analog", (3, 6, 9), False))
    assert os.path.basename(path) == "7_eval_results_Charger98_x_foresight_h6_a3-6-9.csv"
    H.write_to_results_file(res[0], path)
    back = np.array(list(csv.reader(open(path)))[1:], dtype=np.float64)
    assert (U.bits64(back) == U.bits64(res[0])).all()
    env.close(); one.close()


def test_entry_script_writes_the_ensemble_file_after_the_true_one_and_its_regret(tmp_path):
    """SHEMS_FORESIGHT=1, SHEMS_FORESIGHT_HORIZON=6, SHEMS_FORESIGHT_FORECAST=analog:3,6, SHEMS_FORESIGHT_REGRET=1 on the synthetic
    table: the rule-based file, the perfect-foresight file, the true-forecast file followed by the ensemble's, each with its tracker
    row, then one _regret.csv per results file."""
    M = importlib.import_module(U.PKG_NAME + ".main")
    H = importlib.import_module(U.PKG_NAME + ".harness")
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
           "SHEMS_SYNTHETIC_DATA": "1", "SHEMS_TRAIN": "0", "SHEMS_TRACK": "-1", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_HORIZON": "6",
           "SHEMS_FORESIGHT_FORECAST": "analog:3,6", "SHEMS_FORESIGHT_REGRET": "1"}
    cwd0 = os.getcwd()
    try:
        cfg, written = M.main(env, cwd=str(tmp_path), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    stem = f"1179808_eval_results_{cfg.case}_"
    names = ["rule_-1", "foresight", "foresight_h6", "foresight_h6_a3-6"]
    assert [os.path.basename(w) for w in written] == [stem + n + ".csv" for n in names] + [stem + n + "_regret.csv" for n in names]
    tr = list(csv.reader(open(tmp_path / "out/Tracker_Charger.csv")))
    assert len(tr) == 5 and [r[10] for r in tr[2:]] == names[1:] and [r[-1] for r in tr[1:]] == written[:4]
    sums = []
    for w in written[:4]:
        rows = list(csv.reader(open(tmp_path / w)))
        a = np.array(rows[1:], float)
        assert rows[0] == H.RESULTS_HEADER and a.shape == (1439, 23) and (a[:, 0] == np.arange(2, 1441)).all() and np.isfinite(a).all()
        sums.append(a[:, 5].sum())
    assert len(set(sums)) == 4                                              # four different controllers on the same table
    reg = list(csv.reader(open(tmp_path / written[-1])))
    assert reg[0] == H.REGRET_HEADER and len(reg) == 1440 and np.isfinite(np.array(reg[1:], float)).all()

"""The receding-horizon foresight controller planning on a forecast, on the GPU (shems_foresight_solve_forecast_dev, k_fs_window with
fc = 1; shems_foresight_track_forecast_dev, k_fs_track with fc = 1): every stored plane and arg-max against the oracle twin on the composite tables
(bit for bit), identity with solve_horizon when the forecast is the truth, the existing backward sweep on the composite tables at the
largest LDS size, the forward pass against a NumPy controller on the oracle, and the host layers on top."""
import csv
import importlib
import os

import numpy as np
import pytest

import foresight_forecast_ref as FC
import foresight_horizon_ref as FR
import foresight_twin as FT
import philox_np as PH
import util as U
from util import oracle_c

pytestmark = pytest.mark.gpu

S1_CASES = [(1, 1), (6, 1), (6, 4), (12, 1), (30, 30)]


def _grid(F, shape):
    return F.Grid(shape["nb"], shape["ne"], shape["nab"], shape["nae"])


_SOLVED = {}


ACTION_GRIDS = [(5, 3), (9, 9), (17, 17)]    # 15 actions (S1's own); 81: two waves, the second partial; 289: more than the 256 threads


def _forward_cases(hc):
    """(H, c) x ACTION_GRIDS as one parameter list; S1's own action grid keeps the ids the cases had before the grid was a parameter."""
    return [pytest.param(H, c, nab, nae, id=f"{H}-{c}" + ("" if (nab, nae) == ACTION_GRIDS[0] else f"-{nab}x{nae}"))
            for nab, nae in ACTION_GRIDS for H, c in hc]


def _s1(kind, H, c, nab=FT.S1["nab"], nae=FT.S1["nae"]):
    """The device's Values of S1 under (H, c) with the forecast `kind` appended behind the truth (None: solve_horizon on the truth),
    on S1's state grid and the action grid nab x nae (default: S1's own), solved once per process."""
    key = (kind, H, c, nab, nae)
    if key not in _SOLVED:
        S, F = U.pkg(), FT.F()
        d = FT.s1()
        cfgs, T, g = FT.configs(S, "s1"), FT.S1["T"], _grid(F, dict(FT.S1, nab=nab, nae=nae))
        if kind is None:
            _SOLVED[key] = F.solve_horizon([d["tab"]], cfgs, d["idx0"], T, H, c, g)
        else:
            _SOLVED[key] = F.solve_horizon([d["tab"], FC.forecast("s1", 0, kind)], cfgs, d["idx0"], T, H, c, g, forecast_table=[1])
    return _SOLVED[key]


@pytest.mark.parametrize("kind", ["lp", "all"])
@pytest.mark.parametrize("H, c", S1_CASES)
def test_s1_planes_and_argmax_equal_the_twin_on_the_composite_tables(H, c, kind):
    """1 problem, Charger98 eval, T = 30, 9 x 5 nodes, 5 x 3 actions, persistence at lag 6 of load + PV ("lp") and of all four columns
    ("all").  Precondition: the expected planes and arg-max differ from the truth's expectation.  (H, c) = (1, 1) is the one case
    where they cannot: every plan is made at its own hour, whose row is the truth's, and the only forecast value it reads -- the
    arrival overwrite's next row -- moves the state under a zero plane.  There the expectation IS the truth's, and the kernel must
    still reproduce it while reading its next rows from the forecast table."""
    d = FT.s1()
    T = FT.S1["T"]
    eV, eA = FC.expected("s1", 0, kind, H, c)
    tV, tA = FR.expected("s1", 0, H, c)
    if H == 1:
        assert (U.bits64(eV) == U.bits64(tV)).all() and (eA == tA).all()
    else:
        assert (U.bits64(eV) != U.bits64(tV)).any() and (eA != tA).any()
    val = _s1(kind, H, c)
    assert (val.horizon, val.control, val.nsteps, val.forecast_off, val.total_rows) == (H, c, T, [d["tab"].shape[0]], 2 * d["tab"].shape[0])
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    assert V.shape == (1, T + 1, 45) and arg.shape == (1, T, 45)
    same = (U.bits64(V[0]) == U.bits64(eV)).all(axis=1)
    print(f"{kind} (H, c) = ({H}, {c}): planes equal to the twin {int(same.sum())} / {T + 1}; arg-max rows equal "
          f"{int((arg[0] == eA).all(axis=1).sum())} / {T}; planes that differ from the truth's {int((U.bits64(eV) != U.bits64(tV)).any(axis=1).sum())}")
    assert same.all(), np.where(~same)[0]
    assert (arg[0] == eA).all()
    assert (V[0, T] == 0).all()


@pytest.mark.parametrize("H, c", [(6, 4), (30, 1)])
def test_a_forecast_that_is_the_truth_leaves_the_bytes_of_solve_horizon(H, c):
    """forecast_table naming the truth itself (offset 0), a byte copy of the truth behind it, and the copy BEFORE the truth (negative
    offset): all three run k_fs_window under a forecast (fc = 1) and leave what it leaves on the true rows (fc = 0)."""
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    T, g, n = FT.S1["T"], _grid(F, FT.S1), d["tab"].shape[0]
    base = _s1(None, H, c)
    bV, bA = base.V.cpu().numpy(), base.argmax.cpu().numpy()
    assert base.forecast_off == [0]
    copy = FC.forecast("s1", 0, "truth")
    assert copy is not d["tab"] and (U.bits32(copy) == U.bits32(d["tab"])).all()
    for tabs, cfgs, ft, off in (([d["tab"]], FT.configs(S, "s1"), [0], 0), ([d["tab"], copy], FT.configs(S, "s1"), [1], n),
                                ([copy, d["tab"]], [S.make_config(98, n, n)], [0], -n)):
        val = F.solve_horizon(tabs, cfgs, d["idx0"], T, H, c, g, forecast_table=ft)
        assert val.forecast_off == [off]
        assert (U.bits64(val.V.cpu().numpy()) == U.bits64(bV)).all() and (val.argmax.cpu().numpy() == bA).all(), off


def _s2_mixed(want_argmax=True):
    """S2's four problems in one call: row array [F1, t0, t1, t2, t3, F3] -- problem 1 under the load + PV forecast of its table, placed
    BEFORE the truth (negative offset), problem 3 under the four-column forecast of its table behind everything, problems 0 and 2 on
    the truth."""
    S, F = U.pkg(), FT.F()
    d = FT.s2()
    tabs = [FC.forecast("s2", 1, "lp")] + list(d["tabs"]) + [FC.forecast("s2", 3, "all")]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(cid, int(row0[k + 1]), d["tabs"][k].shape[0], **w) for k, (cid, _, _, w) in enumerate(FT.S2_PROBLEMS)]
    val = F.solve_horizon(tabs, cfgs, d["idx0"], FT.S2["T"], 3, 2, _grid(F, FT.S2), want_argmax=want_argmax, forecast_table=[None, 0, None, 5])
    return val, row0


def test_s2_four_problems_with_and_without_forecasts_in_one_call():
    """T = 8, 33 x 9 = 297 nodes, 4 x 7 = 28 actions, (H, c) = (3, 2), lag 3."""
    val, row0 = _s2_mixed()
    assert val.forecast_off == [0, int(row0[0] - row0[2]), 0, int(row0[5] - row0[4])] and val.forecast_off[1] < 0 < val.forecast_off[3]
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    assert V.shape == (4, 9, 297) and arg.shape == (4, 8, 297)
    for p, kind in enumerate(("truth", "lp", "truth", "all")):
        eV, eA = FC.expected("s2", p, kind, 3, 2)
        assert (U.bits64(V[p]) == U.bits64(eV)).all(), p
        assert (arg[p] == eA).all(), p
        tV, tA = FR.expected("s2", p, 3, 2)
        changed = (U.bits64(eV) != U.bits64(tV)).any() or (eA != tA).any()
        print(f"problem {p} ({kind}): planes that differ from the truth's {int((U.bits64(eV) != U.bits64(tV)).any(axis=1).sum())} / 9")
        assert changed == (kind != "truth"), p
    bare, _ = _s2_mixed(want_argmax=False)
    assert bare.argmax is None and (U.bits64(bare.V.cpu().numpy()) == U.bits64(V)).all()


def test_largest_grid_equals_the_backward_sweep_on_the_composite_tables():
    """129 x 65 nodes: two planes = 134 160 bytes of LDS, which k_fs_window gets only through its opt-in.  T = 3, H = 2, c = 1,
    Charger98 eval from row 11 (around an arrival), four-column persistence at lag 2: every plane and arg-max row = row 0 of
    foresight.solve on the composite table of the plan's hour, window by window."""
    S, F = U.pkg(), FT.F()
    tab = U.tables_mod().profile_table(98, "eval")
    fc = FC.persistence(tab, 2, FC.COLS["all"])
    n, idx0, T, H, c = tab.shape[0], 11, 3, 2, 1
    cfgs = [S.make_config(98, 0, n)]
    g = F.Grid(129, 65, 17, 17)
    assert 2 * g.nodes * 8 == 134160
    val = F.solve_horizon([tab, fc], cfgs, idx0, T, H, c, g, forecast_table=[1])
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    j, k = FR.brute_plan(T, H, c)

    def window(made, t, nsteps):
        comp = fc.copy()
        comp[:idx0 + made] = tab[:idx0 + made]
        one = F.solve([comp], cfgs, idx0 + t, nsteps, g)
        return one.V[0, 0].cpu().numpy(), one.argmax[0, 0].cpu().numpy()

    assert (U.bits64(V[0, 0]) == U.bits64(window(0, 0, int(k[0]) + 1)[0])).all()
    for t in range(T):
        want = window(int(j[t]), t + 1, int(k[t]))[0] if k[t] > 0 else np.zeros_like(V[0, 0])
        assert (U.bits64(V[0, t + 1]) == U.bits64(want)).all(), t
        assert (arg[0, t] == window(int(j[t]), t, int(k[t]) + 1)[1]).all(), t
    truth = F.solve_horizon([tab], cfgs, idx0, T, H, c, g)
    assert (U.bits64(truth.V.cpu().numpy()) != U.bits64(V)).any()


def _starts(prof):
    """6 envs: Soc_b = 0, soc_max, the rng = -1 midpoint, three Philox draws (as the existing forward test builds them)."""
    _, draws = PH.reset_draws(77, 0, 3, 2, 1, prof.soc_max)
    return np.array([0.0, prof.soc_max, np.float32(0.5 * float(prof.soc_max))] + list(draws), np.float32)


def _numpy_controller(d, kind, Uplanes, tg, res, next_from, sh=FT.S1):
    """The choices of a NumPy controller on the oracle along the device's own trajectory (replayed through the oracle with the
    device's targets `tg`, rewards and rows compared bitwise when `res` is given): at hour t, 15 candidate envs per env are stepped
    from the true state on the belief of hour t -- the composite table, whose next row is the forecast's (next_from = "forecast") --
    or on the true table (next_from = "truth"); r + interp(U_{t+1}), first maximum.  Returns (choices [n][T][2], the oracle batch
    after the pass, the ordered float64 totals).  sh: the grid (default: S1's own; 15 candidates then)."""
    T = FT.S1["T"]
    tab, prof = d["tab"], d["prof"]
    soc = _starts(prof)
    n = len(soc)
    idx = np.full(n, d["idx0"], np.int32)
    obs = U.obs_of_rows(tab, idx, soc)
    acts = FT.action_grid(sh["nab"], sh["nae"])
    A = len(acts)
    ref = oracle_c.Batch(n, T, tab, prof)
    ref.set_state(obs, idx.astype(np.int64), np.zeros(n, np.int64))
    a_all = np.ascontiguousarray(np.tile(acts, (n, 1)))
    acc = np.zeros(n)
    picks = np.zeros((n, T, 2), np.float32)
    for t in range(T):
        believed = FC.composite("s1", 0, kind, t) if next_from == "forecast" else tab
        cand = oracle_c.Batch(n * A, T, believed, prof)
        cand.set_state(np.repeat(ref.state(), A, axis=0), np.repeat(ref.idx(), A))
        rc, r, o2, _ = cand.step(a_all, 0)
        assert rc == 0
        q = (r + FT.interp(Uplanes[t + 1], sh["nb"], sh["ne"], prof.soc_max, o2[:, 0], o2[:, 1])).reshape(n, A)
        picks[:, t] = acts[np.argmax(q, axis=1)]                            # the first maximum
        rc, r, o, rr = ref.step(tg[:, t], 1, want_results=True)
        assert rc == 0
        if res is not None:
            assert (U.bits64(r) == U.bits64(res[:, t, 5])).all(), t
            assert (U.bits64(rr) == U.bits64(res[:, t])).all(), t
        acc = acc + r
    return picks, ref, acc


def _env_s1(S, kind):
    d = FT.s1()
    T = FT.S1["T"]
    soc = _starts(d["prof"])
    n = len(soc)
    idx = np.full(n, d["idx0"], np.int32)
    obs = U.obs_of_rows(d["tab"], idx, soc)
    env = S.ShemsBatch(n, T, [d["tab"], FC.forecast("s1", 0, kind)], FT.configs(S, "s1"))
    env.state, env.idx, env.step = obs, idx, np.zeros(n, np.int32)
    return env


@pytest.mark.parametrize("H, c, nab, nae", _forward_cases([(6, 1), (6, 4)]))
def test_forward_pass_equals_a_numpy_controller_that_steps_its_candidates_on_the_belief(H, c, nab, nae):
    """foresight.track on the forecast Values, S1, six starts, four-column forecast at lag 6: every choice of every env at every hour,
    the results rows replayed through the oracle bitwise, the ordered float64 totals, the final state and indices.
    The action grid: 5 x 3 is S1's own (less than one wave holds an action; U from the twin).  At 9 x 9 (two waves, the second
    partial) and 17 x 17 (289 actions on 256 threads: threads 0 .. 32 take two, all four waves contribute) U is the device's own
    forecast solve on that grid (the solve kernels are held to the twin elsewhere); with the EV absent every ae ties, so these grids
    also hold the first-maximum rule across lanes and across waves.  At 17 x 17 also: values solved with a forecast table that is a
    byte copy of the truth, appended to the batch, track to the bytes of the pass on solve_horizon's values -- one kernel, fc = 1 and
    fc = 0."""
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    T, sh = FT.S1["T"], dict(FT.S1, nab=nab, nae=nae)
    own = (nab, nae) == (FT.S1["nab"], FT.S1["nae"])
    val = _s1("all", H, c, nab, nae)
    env = _env_s1(S, "all")
    n = env.n
    totals, res, tg = F.track(env, val, None, which=-1)
    assert res.shape == (n, T, 23) and tg.shape == (n, T, 2) and totals.shape == (n,)
    Uplanes = FC.expected("s1", 0, "all", H, c)[0] if own else val.V.cpu().numpy()[0]
    picks, ref, acc = _numpy_controller(d, "all", Uplanes, tg, res, "forecast", sh)
    wrong = np.argwhere((picks != tg).any(axis=2))
    print(f"(H, c) = ({H}, {c}), {nab} x {nae} actions: {len(wrong)} of {n * T} choices differ from the NumPy controller; returns {totals}")
    assert len(wrong) == 0, wrong[:10]
    assert (U.bits32(env.state) == U.bits32(ref.state())).all()
    assert (env.idx == ref.idx()).all() and (env.step == T).all() and (ref.steps() == T).all()
    assert (U.bits64(totals) == U.bits64(acc)).all()                          # the ordered float64 sum
    assert np.unique(tg.reshape(-1, 2), axis=0).shape[0] > 1
    # the truth's controller is another one
    t_env = _env_s1(S, "all")
    t_tot, t_res, t_tg = F.track(t_env, _s1(None, H, c, nab, nae))
    assert (U.bits64(t_tot) != U.bits64(totals)).any()
    env.close(); t_env.close()
    if (nab, nae) == (17, 17):
        c_env = _env_s1(S, "truth")                                          # the batch: the truth and its byte copy behind it
        c_val = F.solve_horizon([d["tab"], FC.forecast("s1", 0, "truth")], FT.configs(S, "s1"), d["idx0"], T, H, c, _grid(F, sh), forecast_table=[1])
        assert c_val.forecast_off == [d["tab"].shape[0]]
        c_tot, c_res, c_tg = F.track(c_env, c_val)
        assert (U.bits64(c_res) == U.bits64(t_res)).all() and (U.bits32(c_tg) == U.bits32(t_tg)).all()
        assert (U.bits64(c_tot) == U.bits64(t_tot)).all()
        c_env.close()


def test_forward_pass_takes_the_next_row_from_the_forecast():
    """On real planes the source of the next row never changes a choice, so it is pinned with crafted planes: the Values of a forecast
    solve on S1 with the EV columns forecast at lag 6, V overwritten in place -- every plane t <= T - 1 becomes 10 Soc_b[node] where
    the node's Soc_ev < 0.75 and -10 Soc_b[node] elsewhere, V[T] = 0.  All 180 choices equal the NumPy controller that reads the next
    row from the forecast, and the one reading it from the truth differs in at least one."""
    import torch
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    T, sh = FT.S1["T"], FT.S1
    g = _grid(F, sh)
    val = F.solve_horizon([d["tab"], FC.forecast("s1", 0, "ev")], FT.configs(S, "s1"), d["idx0"], T, 6, 1, g, forecast_table=[1])
    assert val.forecast_off == [d["tab"].shape[0]]
    sb, se = np.repeat(FT.nodes(sh["nb"], d["prof"].soc_max), sh["ne"]), np.tile(FT.nodes(sh["ne"], 1.0), sh["nb"])
    plane = np.where(se < np.float32(0.75), 10.0 * sb.astype(np.float64), -10.0 * sb.astype(np.float64))
    planes = np.tile(plane, (T + 1, 1))
    planes[T] = 0.0
    val.V.copy_(torch.from_numpy(planes[None]))
    env = _env_s1(S, "ev")
    n = env.n
    totals, res, tg = F.track(env, val, None, which=-1)
    from_forecast, _, _ = _numpy_controller(d, "ev", planes, tg, res, "forecast")
    from_truth, _, _ = _numpy_controller(d, "ev", planes, tg, None, "truth")
    differ = np.argwhere((from_forecast != from_truth).any(axis=2))
    print(f"next row from the truth instead of the forecast: {len(differ)} of {n * T} choices differ, first at hour {differ[:, 1].min() if len(differ) else None}")
    assert len(differ) >= 1
    wrong = np.argwhere((from_forecast != tg).any(axis=2))
    assert len(wrong) == 0, wrong[:10]
    env.close()


def test_forward_pass_refuses_an_env_whose_rows_do_not_hold_the_forecast():
    """The env's batch must hold the tables the solve call saw: another total row count is a ValueError before any launch.  The
    kernel checks for itself that the forecast rows lie inside the ENV's row array (the records may come from a solve on another
    one): asked with the Python check put out of the way, it raises BoundsError and the env is not stepped."""
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    n, T = d["tab"].shape[0], FT.S1["T"]
    val = F.solve_horizon([d["tab"], FC.forecast("s1", 0, "all")], FT.configs(S, "s1"), d["idx0"], T, 6, 1, _grid(F, FT.S1), forecast_table=[1])
    env = S.ShemsBatch(1, T, [d["tab"]], FT.configs(S, "s1"))                 # the truth alone: the forecast table is not in its array
    obs = U.obs_of_rows(d["tab"], [d["idx0"]], np.array([1.0], np.float32))
    env.state, env.idx, env.step = obs, np.array([d["idx0"]], np.int32), np.zeros(1, np.int32)
    with pytest.raises(ValueError, match="same tables"):
        F.track(env, val)
    assert (env.idx == d["idx0"]).all() and (env.step == 0).all()
    assert val.total_rows == 2 * n and val.forecast_off == [n]
    val.total_rows = n                                                      # what a caller of the C ABI could hand over
    with pytest.raises(S._capi.BoundsError):
        F.track(env, val)
    assert (U.bits32(env.state) == U.bits32(obs)).all() and (env.idx == d["idx0"]).all() and (env.step == 0).all()
    env.close()


def test_two_calls_leave_identical_bytes():
    a, _ = _s2_mixed()
    b, _ = _s2_mixed()
    assert (U.bits64(a.V.cpu().numpy()) == U.bits64(b.V.cpu().numpy())).all()
    assert (a.argmax.cpu().numpy() == b.argmax.cpu().numpy()).all()


def test_harness_inference_foresight_with_a_forecast_and_its_file(tmp_path):
    S, F = U.pkg(), FT.F()
    H = importlib.import_module(U.PKG_NAME + ".harness")
    d = FT.s1()
    T, grid = FT.S1["T"], _grid(F, FT.S1)
    cfgs = FT.configs(S, "s1")
    both, index = F.append_forecasts([d["tab"]], 6, FC.NAMES["all"])
    assert index == [1] and (U.bits32(both[1]) == U.bits32(FC.forecast("s1", 0, "all"))).all()
    env = S.ShemsBatch(1, T, both, cfgs)
    total, res = H.inference_foresight(env, grid, horizon=6, forecast_table=index[0])
    assert res.shape == (1, T, 23) and total.shape == (1,)
    one = S.ShemsBatch(1, T, both, cfgs)
    one.reset_(-1)
    t2, r2, _ = F.track(one, F.solve_horizon(both, cfgs, 1, T, 6, 1, grid, forecast_table=index))
    assert (U.bits64(res) == U.bits64(r2)).all() and (U.bits64(total) == U.bits64(t2)).all()
    t0, r0 = H.inference_foresight(env, grid, horizon=6)
    tn, rn = H.inference_foresight(env, grid, horizon=6, forecast_table=[None])
    assert (U.bits64(r0) != U.bits64(res)).any() and (U.bits64(rn) == U.bits64(r0)).all()
    with pytest.raises(ValueError, match="horizon"):
        H.inference_foresight(env, grid, forecast_table=1)
    path = H.foresight_file_name(7, "eval", "Charger98_x", out_dir=str(tmp_path / "out" / "tracker"), horizon=6, forecast=(6, True))
    assert os.path.basename(path) == "7_eval_results_Charger98_x_foresight_h6_p6ev.csv"
    H.write_to_results_file(res[0], path)
    back = np.array(list(csv.reader(open(path)))[1:], dtype=np.float64)
    assert (U.bits64(back) == U.bits64(res[0])).all()
    env.close(); one.close()


def test_entry_script_writes_one_forecast_file_per_horizon_after_the_true_one(tmp_path):
    """SHEMS_FORESIGHT=1, SHEMS_FORESIGHT_HORIZON=6,24, SHEMS_FORESIGHT_FORECAST=persistence:24:ev: the rule-based file, the
    perfect-foresight file, and per horizon the true-forecast file followed by the forecast one, each with its tracker row."""
    M = importlib.import_module(U.PKG_NAME + ".main")
    H = importlib.import_module(U.PKG_NAME + ".harness")
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
           "SHEMS_SYNTHETIC_DATA": "1", "SHEMS_TRAIN": "0", "SHEMS_TRACK": "-1", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_HORIZON": "6,24",
           "SHEMS_FORESIGHT_FORECAST": "persistence:24:ev"}
    cwd0 = os.getcwd()
    try:
        cfg, written = M.main(env, cwd=str(tmp_path), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    stem = f"1179808_eval_results_{cfg.case}_"
    names = ["rule_-1", "foresight", "foresight_h6", "foresight_h6_p24ev", "foresight_h24", "foresight_h24_p24ev"]
    assert [os.path.basename(w) for w in written] == [stem + n + ".csv" for n in names]
    tr = list(csv.reader(open(tmp_path / "out/Tracker_Charger.csv")))
    assert len(tr) == 7 and [r[10] for r in tr[2:]] == names[1:] and [r[-1] for r in tr[1:]] == written
    sums = []
    for w, r in zip(written[1:], tr[2:]):
        rows = list(csv.reader(open(tmp_path / w)))
        a = np.array(rows[1:], float)
        assert rows[0] == H.RESULTS_HEADER and a.shape == (1439, 23) and (a[:, 0] == np.arange(2, 1441)).all() and np.isfinite(a).all()
        assert float(r[14]) == pytest.approx(a[:, 5].sum(), rel=1e-12)
        sums.append(a[:, 5].sum())
    assert len(set(sums)) == 5                                              # five different controllers on the same table

"""The receding-horizon foresight controller on the GPU (shems_foresight_solve_horizon_dev, k_fs_window): every stored plane and
arg-max against the oracle twin solved on each truncated window (bit for bit), against the existing backward sweep on the same device
at the real LDS sizes, the forward pass against a NumPy receding-horizon controller on the oracle, and the host layers on top."""
import csv
import importlib
import os

import numpy as np
import pytest

import foresight_horizon_ref as FR
import foresight_twin as FT
import philox_np as PH
import util as U
from util import oracle_c

pytestmark = pytest.mark.gpu

S1_CASES = [(1, 1), (3, 1), (6, 1), (6, 4), (6, 6), (12, 1)]


def _grid(F, shape):
    return F.Grid(shape["nb"], shape["ne"], shape["nab"], shape["nae"])


_SOLVED = {}


ACTION_GRIDS = [(5, 3), (9, 9), (17, 17)]    # 15 actions (S1's own); 81: two waves, the second partial; 289: more than the 256 threads


def _forward_cases(hc):
    """(H, c) x ACTION_GRIDS as one parameter list; S1's own action grid keeps the ids the cases had before the grid was a parameter."""
    return [pytest.param(H, c, nab, nae, id=f"{H}-{c}" + ("" if (nab, nae) == ACTION_GRIDS[0] else f"-{nab}x{nae}"))
            for nab, nae in ACTION_GRIDS for H, c in hc]


def _s1(H=None, c=1, nab=FT.S1["nab"], nae=FT.S1["nae"]):
    """The device's Values of S1 under (H, c) -- H = None: the existing backward sweep --, on S1's state grid and the action grid
    nab x nae (default: S1's own), solved once per process."""
    if (H, c, nab, nae) not in _SOLVED:
        S, F = U.pkg(), FT.F()
        d = FT.s1()
        args = ([d["tab"]], FT.configs(S, "s1"), d["idx0"], FT.S1["T"])
        g = _grid(F, dict(FT.S1, nab=nab, nae=nae))
        _SOLVED[H, c, nab, nae] = F.solve(*args, g) if H is None else F.solve_horizon(*args, H, c, g)
    return _SOLVED[H, c, nab, nae]


@pytest.mark.parametrize("H, c", S1_CASES)
def test_s1_planes_and_argmax_equal_the_twin_on_every_window(H, c):
    """1 problem, Charger98 eval, T = 30, 9 x 5 nodes, 5 x 3 actions.  V[0][t], t = 1 .. 30, is plane 0 of the twin on the window
    (idx0 + t, k) -- zeros for k = 0 --, the windows truncated at the series end and the ragged last window of c = 4 included; V[0][0]
    and the arg-max likewise.  Not degenerate: every plane 1 .. T - H differs from the full solve's, and for c = 1 exactly the last H
    planes equal it."""
    d = FT.s1()
    T = FT.S1["T"]
    val = _s1(H, c)
    assert (val.horizon, val.control, val.nsteps) == (H, c, T)
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    assert V.shape == (1, T + 1, 45) and arg.shape == (1, T, 45)
    eV, eA = FR.expected("s1", 0, H, c)
    same = (U.bits64(V[0]) == U.bits64(eV)).all(axis=1)
    print(f"(H, c) = ({H}, {c}): planes equal to the twin {int(same.sum())} / {T + 1}; arg-max rows equal {int((arg[0] == eA).all(axis=1).sum())} / {T}")
    assert same.all(), np.where(~same)[0]
    assert (arg[0] == eA).all()
    assert (V[0, T] == 0).all()
    full = (U.bits64(V[0]) == U.bits64(d["V"])).all(axis=1)
    assert not full[1:T - H + 1].any()
    if c == 1:
        assert full[T - H + 1:].all() and int(full[1:].sum()) == H
    if H == 1:
        assert (V[0, 1:] == 0).all()                                        # the myopic controller


@pytest.mark.parametrize("H, c", [(30, 1), (30, 7), (1000, 1)])
def test_horizon_at_least_the_pass_equals_the_full_solve(H, c):
    d = FT.s1()
    val, full = _s1(H, c), _s1()
    assert full.horizon is None and full.control is None
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    assert (U.bits64(V[0]) == U.bits64(d["V"])).all() and (arg[0] == d["arg"]).all()
    assert (U.bits64(V) == U.bits64(full.V.cpu().numpy())).all() and (arg == full.argmax.cpu().numpy()).all()


def _s2(H, c, want_argmax=True):
    S, F = U.pkg(), FT.F()
    d = FT.s2()
    return F.solve_horizon(d["tabs"], FT.configs(S, "s2"), d["idx0"], FT.S2["T"], H, c, _grid(F, FT.S2), want_argmax=want_argmax)


def test_s2_four_problems_in_one_call_equal_the_twin():
    """4 problems in one call, T = 8, 33 x 9 = 297 nodes (not a multiple of the 16 waves), 4 x 7 = 28 actions (a reduction narrower
    than a wave), per-problem capacities and weights, (H, c) = (3, 2): windows made at 0, 2, 4, 6, the last one truncated."""
    d = FT.s2()
    T, H, c = FT.S2["T"], 3, 2
    val = _s2(H, c)
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    assert V.shape == (4, T + 1, 297) and arg.shape == (4, T, 297)
    for p in range(4):
        eV, eA = FR.expected("s2", p, H, c)
        assert (U.bits64(V[p]) == U.bits64(eV)).all(), p
        assert (arg[p] == eA).all(), p
        full = (U.bits64(V[p]) == U.bits64(d["V"][p])).all(axis=1)
        assert list(np.where(full)[0]) == [7, 8], (p, np.where(full)[0])    # only the planes whose plan reaches the end of the pass
    for p, q in ((0, 1), (1, 2), (1, 3), (0, 3)):
        assert (U.bits64(V[p]) != U.bits64(V[q])).any()
    # without the arg-max the planes are the same bytes (the windows then skip their own hour j, except window 0)
    bare = _s2(H, c, want_argmax=False)
    assert bare.argmax is None and (U.bits64(bare.V.cpu().numpy()) == U.bits64(V)).all()


def _against_solve(F, tabs, cfgs, idx0, T, H, c, grid):
    """Device against device: every plane and arg-max row solve_horizon stores = row 0 of the existing backward sweep on that
    window, started on its own."""
    val = F.solve_horizon(tabs, cfgs, idx0, T, H, c, grid)
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    j, k = FR.brute_plan(T, H, c)
    cache = {}

    def window(t, n):
        if (t, n) not in cache:
            one = F.solve(tabs, cfgs, [i + t for i in idx0], n, grid)
            cache[t, n] = one.V[:, 0].cpu().numpy(), one.argmax[:, 0].cpu().numpy()
        return cache[t, n]

    assert (U.bits64(V[:, 0]) == U.bits64(window(0, int(k[0]) + 1)[0])).all()
    for t in range(T):
        want = window(t + 1, int(k[t]))[0] if k[t] > 0 else np.zeros_like(V[:, 0])
        assert (U.bits64(V[:, t + 1]) == U.bits64(want)).all(), t
        assert (arg[:, t] == window(t, int(k[t]) + 1)[1]).all(), t
    assert len(cfgs) == 1 or (U.bits64(V[0, 0]) != U.bits64(V[1, 0])).any()
    return val


def _two_real_problems(S):
    T = U.tables_mod()
    tabs = [T.profile_table(98, "eval"), T.profile_table(5, "eval")]
    cfgs = [S.make_config(98, 0, tabs[0].shape[0]), S.make_config(5, tabs[0].shape[0], tabs[1].shape[0], disc_weight=0.1, disc_pot=1.0)]
    return tabs, cfgs, [11, 107]                                            # windows around an arrival of each table


@pytest.mark.parametrize("H, c", [(3, 1), (4, 2)])
def test_default_grid_equals_the_backward_sweep_on_each_window(H, c):
    """65 x 33 nodes, 17 x 17 actions: two planes = 34 320 bytes of LDS, 2 145 nodes over 16 waves, 289 actions = 4.5 wave-loads."""
    S, F = U.pkg(), FT.F()
    tabs, cfgs, idx0 = _two_real_problems(S)
    _against_solve(F, tabs, cfgs, idx0, 6, H, c, F.Grid())


def test_largest_grid_equals_the_backward_sweep_on_each_window():
    """129 x 65 nodes: two planes = 134 160 bytes of LDS, beyond the 64 KB a kernel gets without the opt-in."""
    S, F = U.pkg(), FT.F()
    tabs, cfgs, idx0 = _two_real_problems(S)
    g = F.Grid(129, 65, 17, 17)
    assert 2 * g.nodes * 8 == 134160
    _against_solve(F, tabs[:1], cfgs[:1], idx0[:1], 3, 2, 1, g)


def _starts(prof):
    """6 envs: Soc_b = 0, soc_max, the rng = -1 midpoint, three Philox draws (as the existing forward test builds them)."""
    _, draws = PH.reset_draws(77, 0, 3, 2, 1, prof.soc_max)
    return np.array([0.0, prof.soc_max, np.float32(0.5 * float(prof.soc_max))] + list(draws), np.float32)


@pytest.mark.parametrize("H, c, nab, nae", _forward_cases([(None, 1), (6, 1), (6, 4)]))
def test_forward_pass_equals_a_numpy_receding_horizon_controller_on_the_oracle(H, c, nab, nae):
    """foresight.track on solve_horizon's Values, S1, six starts.  The results are replayed through the oracle hour by hour (rewards,
    rows, final state, ordered float64 totals), and the target chosen by EVERY env at EVERY hour equals a NumPy controller on the
    oracle: one oracle env per action (15 on S1's own grid) stepped from the env's true state, r + interp(U_{t+1}), first maximum, with U from the twin on the plan's
    truncated window.  H = None runs the same check on the existing backward sweep's Values (U = the full solve's planes): it passes
    on the kernels this feature does not touch, which separates a mistake in this test from one in k_fs_window.
    The action grid: 5 x 3 is S1's own (less than one wave holds an action).  At 9 x 9 (two waves, the second partial) and 17 x 17
    (289 actions on 256 threads: threads 0 .. 32 take two, all four waves contribute) U is the device's own solve on that grid (the
    solve kernels are held to the twin elsewhere); with the EV absent every ae ties, so these grids also hold the first-maximum rule
    across lanes and across waves."""
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    T, sh = FT.S1["T"], dict(FT.S1, nab=nab, nae=nae)
    tab, prof = d["tab"], d["prof"]
    val = _s1(H, c, nab, nae)
    if (nab, nae) == (FT.S1["nab"], FT.S1["nae"]):
        Uplanes = d["V"] if H is None else FR.expected("s1", 0, H, c)[0]
    else:
        Uplanes = val.V.cpu().numpy()[0]
    soc = _starts(prof)
    n = len(soc)
    idx = np.full(n, d["idx0"], np.int32)
    obs = U.obs_of_rows(tab, idx, soc)
    env = S.ShemsBatch(n, T, [tab], FT.configs(S, "s1"))
    env.state, env.idx, env.step = obs, idx, np.zeros(n, np.int32)
    totals, res, tg = F.track(env, val, None, which=-1)
    assert res.shape == (n, T, 23) and tg.shape == (n, T, 2) and totals.shape == (n,)
    acts = FT.action_grid(sh["nab"], sh["nae"])
    A = len(acts)
    ref = oracle_c.Batch(n, T, tab, prof)
    ref.set_state(obs, idx.astype(np.int64), np.zeros(n, np.int64))
    cand = oracle_c.Batch(n * A, T, tab, prof)
    a_all = np.ascontiguousarray(np.tile(acts, (n, 1)))
    acc = np.zeros(n)
    wrong = []
    for t in range(T):
        cand.set_state(np.repeat(ref.state(), A, axis=0), np.repeat(ref.idx(), A))
        rc, r, o2, _ = cand.step(a_all, 0)
        assert rc == 0
        q = (r + FT.interp(Uplanes[t + 1], sh["nb"], sh["ne"], prof.soc_max, o2[:, 0], o2[:, 1])).reshape(n, A)
        pick = acts[np.argmax(q, axis=1)]                                   # the first maximum
        wrong += [(t, e) for e in np.where((pick != tg[:, t]).any(axis=1))[0]]
        rc, r, o, rr = ref.step(tg[:, t], 1, want_results=True)
        assert rc == 0
        assert (U.bits64(r) == U.bits64(res[:, t, 5])).all(), t
        assert (U.bits64(rr) == U.bits64(res[:, t])).all(), t
        acc = acc + r
    print(f"(H, c) = ({H}, {c}), {nab} x {nae} actions: {len(wrong)} of {n * T} choices differ from the NumPy controller; returns {totals}")
    assert not wrong, wrong[:10]
    assert (U.bits32(env.state) == U.bits32(ref.state())).all()
    assert (env.idx == ref.idx()).all() and (env.step == T).all() and (ref.steps() == T).all()
    assert (U.bits64(totals) == U.bits64(acc)).all()                          # the ordered float64 sum
    assert np.unique(tg.reshape(-1, 2), axis=0).shape[0] > 1
    env.close()


def test_two_calls_leave_identical_bytes():
    a = _s2(3, 2)
    b = _s2(3, 2)
    assert (U.bits64(a.V.cpu().numpy()) == U.bits64(b.V.cpu().numpy())).all()
    assert (a.argmax.cpu().numpy() == b.argmax.cpu().numpy()).all()


def test_harness_inference_foresight_with_a_horizon_and_its_files(tmp_path):
    S, F = U.pkg(), FT.F()
    H = importlib.import_module(U.PKG_NAME + ".harness")
    d = FT.s1()
    T, grid = FT.S1["T"], _grid(F, FT.S1)
    cfgs = FT.configs(S, "s1")
    env = S.ShemsBatch(1, T, [d["tab"]], cfgs)
    total, res = H.inference_foresight(env, grid, horizon=6)
    assert res.shape == (1, T, 23) and total.shape == (1,)
    val = F.solve_horizon([d["tab"]], cfgs, 1, T, 6, 1, grid)
    one = S.ShemsBatch(1, T, [d["tab"]], cfgs)
    one.reset_(-1)
    t2, r2, _ = F.track(one, val)
    assert (U.bits64(res) == U.bits64(r2)).all() and (U.bits64(total) == U.bits64(t2)).all()
    assert (env.idx == 1 + T).all() and (U.bits32(env.state) == U.bits32(one.state)).all()
    t4, r4 = H.inference_foresight(env, grid, horizon=6, control=4)
    tf, rf = H.inference_foresight(env, grid)
    assert (U.bits64(r4) != U.bits64(res)).any() and (U.bits64(rf) != U.bits64(res)).any()      # three different controllers
    path = H.foresight_file_name(7, "eval", "Charger98_x", out_dir=str(tmp_path / "out" / "tracker"), horizon=6)
    assert os.path.basename(path) == "7_eval_results_Charger98_x_foresight_h6.csv"
    H.write_to_results_file(res[0], path)
    back = np.array(list(csv.reader(open(path)))[1:], dtype=np.float64)
    assert (U.bits64(back) == U.bits64(res[0])).all()
    sums = H.write_to_tracker_file(path, str(tmp_path / "out" / "Tracker_Charger.csv"), num_ep=1001, seed=H.foresight_seed(6), case="Charger98_x", now="t")
    row = list(csv.reader(open(tmp_path / "out" / "Tracker_Charger.csv")))[1]
    assert row[10] == "foresight_h6" and row[-1] == path
    assert float(row[14]) == sums["rewards"] and sums["rewards"] == pytest.approx(total[0], rel=1e-12)
    env.close(); one.close()


def test_group_foresight_scores_with_a_horizon_equal_direct_track_returns():
    """group.foresight_scores(horizon=12) on the 2-learner eval batch of the existing group test (two chargers, test_runs = 3) = the
    mean of three track returns on solve_horizon's Values, computed directly."""
    S, F = U.pkg(), FT.F()
    G = importlib.import_module(U.PKG_NAME + ".group")
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    T = U.tables_mod()
    ids = (5, 9)
    tabs = [T.pad_rows(T.profile_table(c, "eval"), 1440) for c in ids]
    env = G.eval_batch(tabs, [0, 1], 2, test_runs=3, charger_ids=ids)
    scores = G.foresight_scores(env, test_runs=3, horizon=12)
    assert scores.shape == (2,) and scores.dtype == np.float64
    E = env.n // 2
    for l, c in enumerate(ids):
        blk = S.ShemsBatch(E, 1439, [tabs[l]], [S.make_config(c, 0, 1440)])
        blk.reset_(D.SEED_INI, episode=0)
        idx = blk.idx
        assert (idx == idx[0]).all()
        val = F.solve_horizon([tabs[l]], [S.make_config(c, 0, 1440)], int(idx[0]), 72, 12, 1, F.Grid(), want_argmax=False)
        tot, _, _ = F.track(blk, val)
        assert scores[l] == np.cumsum(tot[:3])[-1] / 3
        blk.close()
    assert scores[0] != scores[1]
    env.close()


def test_entry_script_writes_one_file_per_horizon_after_the_perfect_one(tmp_path):
    """SHEMS_FORESIGHT=1 with SHEMS_FORESIGHT_HORIZON=6,24: exactly the rule-based file, the perfect-foresight file, the h6 file and
    the h24 file, in that order, each with its tracker row."""
    M = importlib.import_module(U.PKG_NAME + ".main")
    H = importlib.import_module(U.PKG_NAME + ".harness")
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
           "SHEMS_SYNTHETIC_DATA": "1", "SHEMS_TRAIN": "0", "SHEMS_TRACK": "-1", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_HORIZON": "6,24"}
    cwd0 = os.getcwd()
    try:
        cfg, written = M.main(env, cwd=str(tmp_path), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    stem = f"1179808_eval_results_{cfg.case}_"
    assert [os.path.basename(w) for w in written] == [stem + "rule_-1.csv", stem + "foresight.csv", stem + "foresight_h6.csv", stem + "foresight_h24.csv"]
    tr = list(csv.reader(open(tmp_path / "out/Tracker_Charger.csv")))
    assert len(tr) == 5 and [r[10] for r in tr[2:]] == ["foresight", "foresight_h6", "foresight_h24"] and [r[-1] for r in tr[1:]] == written
    sums = []
    for w, r in zip(written[1:], tr[2:]):
        rows = list(csv.reader(open(tmp_path / w)))
        a = np.array(rows[1:], float)
        assert rows[0] == H.RESULTS_HEADER and a.shape == (1439, 23) and (a[:, 0] == np.arange(2, 1441)).all() and np.isfinite(a).all()
        assert float(r[14]) == pytest.approx(a[:, 5].sum(), rel=1e-12)
        sums.append(a[:, 5].sum())
    assert len(set(sums)) == 3                                              # three different controllers on the same table

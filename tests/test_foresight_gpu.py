"""The perfect-foresight controller on the GPU: the backward sweep against the float64 oracle twin (bit for bit), the forward pass
replayed through the oracle, the host layers on top (harness, learner groups)."""
import csv
import importlib

import numpy as np
import pytest

import foresight_twin as FT
import philox_np as PH
import util as U
from util import oracle_c

pytestmark = pytest.mark.gpu


def _grid(F, shape):
    return F.Grid(shape["nb"], shape["ne"], shape["nab"], shape["nae"])


_SOLVED = {}


def _solved(which):
    """The device's V of a shape, solved once per process (the forward tests run on it)."""
    if which not in _SOLVED:
        S, F = U.pkg(), FT.F()
        d, shape = (FT.s1(), FT.S1) if which == "s1" else (FT.s2(), FT.S2)
        tabs = [d["tab"]] if which == "s1" else d["tabs"]
        _SOLVED[which] = F.solve(tabs, FT.configs(S, which), d["idx0"], shape["T"], _grid(F, shape))
    return _SOLVED[which]


def test_backward_sweep_s1_equals_the_twin():
    """1 problem, Charger98 eval, 30 hours, 9 x 5 nodes, 5 x 3 actions; the window holds an arrival, an h == 0 row, a PV surplus and
    a PV shortfall."""
    d = FT.s1()
    assert all(FT.window_features(d["tab"], d["idx0"], FT.S1["T"]))
    val = _solved("s1")
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    assert V.shape == (1, 31, 45) and arg.shape == (1, 30, 45)
    assert (U.bits64(V[0]) == U.bits64(d["V"])).all()
    assert (arg[0] == d["arg"]).all()
    assert (V[0, 30] == 0).all() and np.unique(arg).size > 3


def test_backward_sweep_s2_problems_equal_the_twin():
    """4 problems in one call (Charger 98 eval row 9, Charger 5 eval row 97, Charger 1 test row 127, Charger 5 eval row 106; different
    capacities, two with disc_weight 0.1 / disc_pot 1, one with penalty_weight 0.2), 8 hours, 33 x 9 = 297 nodes (a ragged last tile),
    4 x 7 = 28 actions (a reduction narrower than a wave).  On the tables as they are the window of row 9 holds an arrival, those of
    rows 127 and 106 an arrival and a departure; the window of row 97 holds neither (Charger 5's next session starts at row 108),
    which is why row 106 carries the discomfort weights a second time."""
    d = FT.s2()
    feats = [FT.window_features(t, i, FT.S2["T"]) for t, i in zip(d["tabs"], d["idx0"])]
    assert feats[0][0] and feats[2][0] and feats[2][1] and feats[3][0] and feats[3][1]
    assert len({float(p.soc_max) for p in d["profs"]}) > 1 and len({float(p.cap_ev) for p in d["profs"]}) == 3
    val = _solved("s2")
    V, arg = val.V.cpu().numpy(), val.argmax.cpu().numpy()
    assert V.shape == (4, 9, 297) and arg.shape == (4, 8, 297)
    for p in range(4):
        assert (U.bits64(V[p]) == U.bits64(d["V"][p])).all(), p
        assert (arg[p] == d["arg"][p]).all(), p
    assert (U.bits64(V[0]) != U.bits64(V[1])).any() and (U.bits64(V[1]) != U.bits64(V[2])).any() and (U.bits64(V[1]) != U.bits64(V[3])).any()
    # Values.at: the host restatement reads the device's planes as the twin's interpolation does
    x = np.array([0.3, 2.0, 5.9], np.float32), np.array([0.1, 0.55, 1.0], np.float32)
    assert (U.bits64(val.at(1, 3, *x)) == U.bits64(FT.interp(d["V"][1][3], 33, 9, d["profs"][1].soc_max, *x))).all()


@pytest.mark.parametrize("n_problems, npw", [(8, 4), (20, 8)])
def test_several_nodes_per_wave_equal_single_problem_solves(n_problems, npw):
    """A wave takes 8, 4, 2 or 1 nodes one after the other, the most that still leave 1024 workgroups: one or two problems at the
    default 65 x 33 grid run at 1, 8 problems at 4 (135 tiles of 16 nodes each, the last one holding 1 node), 20 problems -- the
    learner-group case -- at 8 (68 tiles of 32, the last one holding 1).  Every problem of the many-problem call must leave the
    bytes its own single-problem call (1 node per wave) leaves, over 2 hours so that hour 0 reads an interpolated V_1."""
    S, F = U.pkg(), FT.F()
    T = U.tables_mod()
    g, hours = F.Grid(), 2
    tiles = lambda k: -(-g.nodes // (4 * k))
    assert tiles(npw) * n_problems >= 1024 and (npw == 8 or tiles(2 * npw) * n_problems < 1024) and tiles(1) < 1024   # the entry point's rule
    assert g.nodes % (4 * npw) == 1
    tabs = [T.profile_table(98, "eval"), T.profile_table(5, "eval")]
    row0 = [0, tabs[0].shape[0]]
    weights = ({}, dict(disc_weight=0.1, disc_pot=1.0), dict(penalty_weight=0.2))
    cfgs, idx0 = [], []
    for p in range(n_problems):
        k = p % 2
        cfgs.append(S.make_config((98, 5)[k], row0[k], tabs[k].shape[0], **weights[p % 3]))
        idx0.append((11, 107)[k] + p // 2)                                  # windows around an arrival of each table
    many = F.solve(tabs, cfgs, idx0, hours, g)
    V, arg = many.V.cpu().numpy(), many.argmax.cpu().numpy()
    assert V.shape == (n_problems, hours + 1, g.nodes)
    for p in range(n_problems):
        one = F.solve(tabs, [cfgs[p]], idx0[p], hours, g)
        assert (U.bits64(one.V.cpu().numpy()[0]) == U.bits64(V[p])).all(), p
        assert (one.argmax.cpu().numpy()[0] == arg[p]).all(), p
    assert np.unique(U.bits64(V[:, 0]), axis=0).shape[0] == n_problems       # no two problems alike: per-problem indexing shows


def test_edges_one_hour_two_by_two_nodes_one_action():
    """T = 1, grid 2 x 2, actions 1 x 1: V_0 is exactly the one-step reward of the target (1, 1) at the four nodes."""
    S, F = U.pkg(), FT.F()
    tab = FT.s1()["tab"]
    prof = oracle_c.profile(98)
    for idx0 in (1, 12, 21):
        val = F.solve([tab], [S.make_config(98, 0, tab.shape[0])], idx0, 1, F.Grid(2, 2, 1, 1))
        sb = np.repeat(np.array([0.0, prof.soc_max], np.float32), 2)
        obs = U.obs_of_rows(tab, np.full(4, idx0), sb)
        obs[:, 1] = np.tile(np.array([0.0, 1.0], np.float32), 2)
        ref = oracle_c.Batch(4, 1, tab, prof)
        ref.set_state(obs, np.full(4, idx0, np.int64))
        rc, r, _, _ = ref.step(np.ones((4, 2), np.float32), 0)
        V = val.V.cpu().numpy()
        assert rc == 0 and V.shape == (1, 2, 4) and (U.bits64(V[0, 0]) == U.bits64(r)).all() and (V[0, 1] == 0).all()
        assert (val.argmax.cpu().numpy() == 0).all()


def _starts(d_profs, idx0s):
    """6 envs per problem: Soc_b = 0, soc_max, the rng = -1 midpoint, three Philox draws."""
    soc, poe = [], []
    for p, prof in enumerate(d_profs):
        _, draws = PH.reset_draws(77 + p, 0, 3, 2, 1, prof.soc_max)
        soc += [0.0, prof.soc_max, np.float32(0.5 * float(prof.soc_max))] + list(draws)
        poe += [p] * 6
    return np.array(soc, np.float32), np.array(poe, np.int32)


@pytest.mark.parametrize("which", ["s1", "s2"])
def test_forward_pass_replayed_through_the_oracle(which):
    S, F = U.pkg(), FT.F()
    d, shape = (FT.s1(), FT.S1) if which == "s1" else (FT.s2(), FT.S2)
    tabs = [d["tab"]] if which == "s1" else d["tabs"]
    profs = [d["prof"]] if which == "s1" else d["profs"]
    idx0s = [d["idx0"]] if which == "s1" else d["idx0"]
    T = shape["T"]
    val = _solved(which)
    soc, poe = _starts(profs, idx0s)
    n = len(soc)
    idx = np.array([idx0s[p] for p in poe], np.int32)
    obs = np.concatenate([U.obs_of_rows(tabs[p], idx[poe == p], soc[poe == p]) for p in range(len(tabs))])
    env = S.ShemsBatch(n, T, tabs, FT.configs(S, which), poe.astype(np.uint16))
    env.state, env.idx, env.step = obs, idx, np.zeros(n, np.int32)
    totals, res, tg = F.track(env, val, poe, which=-1)
    assert res.shape == (n, T, 23) and tg.shape == (n, T, 2) and totals.shape == (n,)
    # the emitted targets are members of the action grid, and the results rows hold them
    grid = val.grid
    assert np.isin(tg[..., 0], grid.b_targets()).all() and np.isin(tg[..., 1], grid.ev_targets()).all()
    assert (res[..., 21] == tg[..., 0]).all() and (res[..., 2] == tg[..., 1]).all()
    # replay through the oracle, hour by hour
    ref = oracle_c.Batch(n, T, tabs, profs, poe.astype(np.int64), poe.astype(np.int64))
    ref.set_state(obs, idx.astype(np.int64), np.zeros(n, np.int64))
    acc = np.zeros(n)
    for t in range(T):
        rc, r, o, rr = ref.step(tg[:, t], 1, want_results=True)
        assert rc == 0
        assert (U.bits64(r) == U.bits64(res[:, t, 5])).all(), t
        assert (U.bits64(rr) == U.bits64(res[:, t])).all(), t
        acc = acc + r
    assert (U.bits32(env.state) == U.bits32(ref.state())).all()
    assert (env.idx == ref.idx()).all() and (env.step == T).all() and (ref.steps() == T).all()
    assert (U.bits64(totals) == U.bits64(acc)).all()                          # the ordered float64 sum
    # hour 0 of an env that starts on a node: the backward sweep's stored arg-max for that node
    arg = val.argmax.cpu().numpy()
    ev_nodes, compared = grid.soc_ev_nodes(), 0
    for e in range(n):
        p = int(poe[e])
        ib = np.where(grid.soc_b_nodes(profs[p].soc_max) == soc[e])[0]
        ie = np.where(ev_nodes == obs[e, 1])[0]
        if ib.size and ie.size:
            a = int(arg[p, 0, ib[0] * grid.ne + ie[0]])
            assert (tg[e, 0] == grid.targets()[a]).all(), e
            compared += 1
    assert compared >= 3 * len(tabs)
    assert np.unique(tg.reshape(-1, 2), axis=0).shape[0] > 1
    env.close()


def test_wrong_start_row_raises_the_env_error_and_steps_nothing():
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    val = _solved("s1")
    env = S.ShemsBatch(3, FT.S1["T"], [d["tab"]], FT.configs(S, "s1"))
    obs = U.obs_of_rows(d["tab"], np.full(3, d["idx0"] + 1), np.array([0.0, 1.0, 2.0], np.float32))
    env.state, env.idx, env.step = obs, np.full(3, d["idx0"] + 1, np.int32), np.array([4, 5, 6], np.int32)
    with pytest.raises(S._capi.BoundsError):
        F.track(env, val)
    assert (U.bits32(env.state) == U.bits32(obs)).all() and (env.idx == d["idx0"] + 1).all() and (env.step == [4, 5, 6]).all()
    # one env of the batch off its start row (and one naming a problem that does not exist): those two are left alone, the third runs
    idx = np.array([d["idx0"], d["idx0"] + 1, d["idx0"]], np.int32)
    obs = U.obs_of_rows(d["tab"], idx, np.array([0.0, 1.0, 2.0], np.float32))
    env.state, env.idx, env.step = obs, idx, np.zeros(3, np.int32)
    with pytest.raises(S._capi.BoundsError):
        F.track(env, val, np.array([0, 0, 1], np.int32))
    assert (env.idx == [d["idx0"] + FT.S1["T"], d["idx0"] + 1, d["idx0"]]).all() and (env.step == [FT.S1["T"], 0, 0]).all()
    assert (U.bits32(env.state[1:]) == U.bits32(obs[1:])).all()
    env.close()


def test_harness_inference_foresight_and_file_round_trip(tmp_path):
    S, F = U.pkg(), FT.F()
    H = importlib.import_module(U.PKG_NAME + ".harness")
    d = FT.s1()
    T, grid = FT.S1["T"], _grid(F, FT.S1)
    cfgs = FT.configs(S, "s1")
    env = S.ShemsBatch(1, T, [d["tab"]], cfgs)
    total, res = H.inference_foresight(env, grid)
    assert res.shape == (1, T, 23) and total.shape == (1,)
    # = solve from row 1 + the forward pass from the reset!(rng = -1) start
    val = F.solve([d["tab"]], cfgs, 1, T, grid)
    if d["idx0"] == 1:
        assert (U.bits64(val.V.cpu().numpy()[0]) == U.bits64(d["V"])).all()
    one = S.ShemsBatch(1, T, [d["tab"]], cfgs)
    one.reset_(-1)
    t2, r2, _ = F.track(one, val)
    assert (U.bits64(res) == U.bits64(r2)).all() and (U.bits64(total) == U.bits64(t2)).all()
    assert (env.idx == 1 + T).all() and (U.bits32(env.state) == U.bits32(one.state)).all()
    path = H.foresight_file_name(7, "eval", "Charger98_x", out_dir=str(tmp_path / "out" / "tracker"))
    H.write_to_results_file(res[0], path)
    back = np.array(list(csv.reader(open(path)))[1:], dtype=np.float64)
    assert (U.bits64(back) == U.bits64(res[0])).all()
    sums = H.write_to_tracker_file(path, str(tmp_path / "out" / "Tracker_Charger.csv"), num_ep=1001, seed="foresight", case="Charger98_x", now="t")
    row = list(csv.reader(open(tmp_path / "out" / "Tracker_Charger.csv")))[1]
    assert row[10] == "foresight" and row[-1] == path
    for k, col in (("rewards", 5), ("profit", 6), ("discomfort", 7), ("penalty", 8)):
        assert sums[k] == pytest.approx(res[0][:, col].sum(), rel=1e-12, abs=1e-12)
    assert float(row[14]) == sums["rewards"] and sums["rewards"] == pytest.approx(total[0], rel=1e-12)
    env.close(); one.close()


def test_group_foresight_scores_equal_direct_track_returns():
    """group.foresight_scores on a 2-learner eval_batch (two chargers, test_runs = 3) = the mean of three track returns computed directly."""
    S, F = U.pkg(), FT.F()
    G = importlib.import_module(U.PKG_NAME + ".group")
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    T = U.tables_mod()
    ids = (5, 9)
    tabs = [T.pad_rows(T.profile_table(c, "eval"), 1440) for c in ids]
    env = G.eval_batch(tabs, [0, 1], 2, test_runs=3, charger_ids=ids)
    scores = G.foresight_scores(env, test_runs=3)
    assert scores.shape == (2,) and scores.dtype == np.float64
    E = env.n // 2
    for l, c in enumerate(ids):
        blk = S.ShemsBatch(E, 1439, [tabs[l]], [S.make_config(c, 0, 1440)])
        blk.reset_(D.SEED_INI, episode=0)                                     # the sweep's fixed key, env indices from 0 in the block
        idx = blk.idx
        assert (idx == idx[0]).all()
        val = F.solve([tabs[l]], [S.make_config(c, 0, 1440)], int(idx[0]), 72, F.Grid())
        tot, _, _ = F.track(blk, val)
        assert scores[l] == np.cumsum(tot[:3])[-1] / 3
        blk.close()
    assert scores[0] != scores[1]
    env.close()


def test_two_solves_leave_identical_bytes():
    S, F = U.pkg(), FT.F()
    d = FT.s2()
    a = _solved("s2")
    b = F.solve(d["tabs"], FT.configs(S, "s2"), d["idx0"], FT.S2["T"], _grid(F, FT.S2))
    assert (U.bits64(a.V.cpu().numpy()) == U.bits64(b.V.cpu().numpy())).all()
    assert (a.argmax.cpu().numpy() == b.argmax.cpu().numpy()).all()


def test_entry_script_writes_the_foresight_file_when_asked(tmp_path):
    """SHEMS_FORESIGHT=1: after the tracking block (here the rule-based pass) main writes <job>_<run>_results_<case>_foresight.csv --
    the pass over the whole eval set, 1 439 hours -- and a tracker row with seed = "foresight"."""
    import os
    M = importlib.import_module(U.PKG_NAME + ".main")
    H = importlib.import_module(U.PKG_NAME + ".harness")
    F = FT.F()
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
           "SHEMS_SYNTHETIC_DATA": "1", "SHEMS_TRAIN": "0", "SHEMS_TRACK": "-1", "SHEMS_FORESIGHT": "1"}
    cwd0 = os.getcwd()
    try:
        cfg, written = M.main(env, cwd=str(tmp_path), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    assert [os.path.basename(w) for w in written] == [f"1179808_eval_results_{cfg.case}_rule_-1.csv", f"1179808_eval_results_{cfg.case}_foresight.csv"]
    rows = list(csv.reader(open(tmp_path / written[1])))
    a = np.array(rows[1:], float)
    assert rows[0] == H.RESULTS_HEADER and a.shape == (1439, 23) and (a[:, 0] == np.arange(2, 1441)).all() and np.isfinite(a).all()
    g = F.Grid()
    assert np.isin(a[:, 21].astype(np.float32), g.b_targets()).all() and np.isin(a[:, 2].astype(np.float32), g.ev_targets()).all()
    tr = list(csv.reader(open(tmp_path / "out/Tracker_Charger.csv")))
    assert len(tr) == 3 and tr[2][10] == "foresight" and tr[2][-1] == written[1] and float(tr[2][14]) == pytest.approx(a[:, 5].sum(), rel=1e-12)

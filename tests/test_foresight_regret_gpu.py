"""The foresight audit on the GPU: shems_foresight_audit_dev against the oracle twin (tests/foresight_regret_ref.py) bit for bit, the
exact zero of a greedy pass, refused rows, and the host layers on top (foresight.audit, harness.regret_of, the entry script)."""
import csv
import importlib
import os

import numpy as np
import pytest

import foresight_regret_ref as RR
import foresight_twin as FT
import util as U
from util import oracle_c

pytestmark = pytest.mark.gpu


def _grid(F, shape):
    return F.Grid(shape["nb"], shape["ne"], shape["nab"], shape["nae"])


def _counts(shape):
    return {k: shape[k] for k in ("nb", "ne", "nab", "nae")}


_SOLVED = {}


def _solved(which):
    """The device's V of a shape, solved once per process."""
    if which not in _SOLVED:
        S, F = U.pkg(), FT.F()
        d, shape = (FT.s1(), FT.S1) if which == "s1" else (FT.s2(), FT.S2)
        tabs = [d["tab"]] if which == "s1" else d["tabs"]
        _SOLVED[which] = F.solve(tabs, FT.configs(S, which), d["idx0"], shape["T"], _grid(F, shape))
    return _SOLVED[which]


def _same(a, out, act, k=None):
    got = np.stack([a.best_q, a.achieved_q, a.v_state], -1)
    sel = slice(None) if k is None else k
    return bool((U.bits64(got[sel]) == U.bits64(out)).all() and (a.best_action[sel] == act).all())


def test_s1_three_passes_in_one_call_equal_the_twin():
    """n = 3, 15 actions (a reduction narrower than a wave), 30 hours (8 tiles of 4 hours, the last one holding 2)."""
    F = FT.F()
    res, took = RR.s1_passes()
    out, act = RR.s1_twin()
    a = F.audit(_solved("s1"), res)
    assert a.best_q.shape == (3, 30) and a.best_action.dtype == np.int32 and a.best_targets.shape == (3, 30, 2)
    assert _same(a, out, act)
    assert (U.bits64(a.regret[1]) == 0).all() and (a.best_action[1] == took).all()
    assert (a.regret[0] > 0).sum() >= 2 and (a.regret[2] > 0).sum() >= 20
    assert (a.best_targets == FT.action_grid(5, 3)[act]).all()
    s = a.summary()
    for e in range(3):
        assert sum(s[p][e] for p in F.PHASES) == pytest.approx(s["regret"][e], abs=1e-12)
        assert s["return"][e] == pytest.approx(res[e][:, 5].sum(), abs=1e-12)
    d = FT.s1()
    h_next = d["tab"][d["idx0"]:d["idx0"] + 30, 0]
    assert [int(x) for x in a.phase[0]] == [RR.phase_of(res[0, t, 1], h_next[t]) for t in range(30)]
    # one pass as [T][23]
    one = F.audit(_solved("s1"), res[2])
    assert one.best_q.shape == (1, 30) and _same(one, out[2:3], act[2:3])


def test_s2_passes_of_four_problems_equal_the_twin():
    """Four problems, 8 hours, 28 actions, five passes with problem_of_pass = [3, 0, 2, 1, 0]."""
    F = FT.F()
    res = RR.s2_passes()
    out, act = RR.s2_twin()
    a = F.audit(_solved("s2"), res, list(RR.S2_PASSES))
    assert a.best_q.shape == (5, 8)
    for e in range(5):
        assert _same(a, out[e], act[e], e), e
    assert np.unique(U.bits64(a.best_q), axis=0).shape[0] == 5               # no two passes alike: per-pass indexing shows
    assert (a.regret > 0).any()


def test_more_than_64_actions_on_the_devices_own_planes():
    """Grid 17 x 9 nodes, 9 x 9 = 81 actions (a lane takes two), T = 13 on Charger98 eval row 11, V from the device's own solve."""
    S, F = U.pkg(), FT.F()
    tab, prof = FT.s1()["tab"], oracle_c.profile(98)
    shape = dict(T=13, nb=17, ne=9, nab=9, nae=9)
    val = F.solve([tab], [S.make_config(98, 0, tab.shape[0])], 11, 13, _grid(F, shape))
    V = val.V.cpu().numpy()[0]
    res = np.stack([RR.rule_pass(tab, prof, 11, 13), RR.random_pass(tab, prof, 11, 13, seed=7, soc_b0=1.25)])
    a = F.audit(val, res)
    for e in range(2):
        out, act = RR.twin_audit(V, res[e], tab, prof, 11, **_counts(shape))
        assert _same(a, out, act, e), e
    assert (a.best_action >= 64).any() and (a.regret[1] > 0).any()


@pytest.mark.parametrize("horizon", [None, (6, 4)])
def test_the_forward_pass_audits_to_exactly_zero(horizon):
    """foresight.track's own rows on S1, audited against the values it followed (solve, and solve_horizon(6, 4)): regret exactly 0.0
    in every hour, best_targets the targets track returned."""
    S, F = U.pkg(), FT.F()
    d, T = FT.s1(), FT.S1["T"]
    cfgs = FT.configs(S, "s1")
    val = _solved("s1") if horizon is None else F.solve_horizon([d["tab"]], cfgs, d["idx0"], T, horizon[0], horizon[1], _grid(F, FT.S1))
    soc = np.array([0.5 * float(d["prof"].soc_max), 0.0, 1.7], np.float32)
    env = S.ShemsBatch(3, T, [d["tab"]], cfgs)
    env.state, env.idx, env.step = U.obs_of_rows(d["tab"], np.full(3, d["idx0"]), soc), np.full(3, d["idx0"], np.int32), np.zeros(3, np.int32)
    _, res, tg = F.track(env, val)
    a = F.audit(val, res)
    assert (U.bits64(a.regret) == 0).all()
    assert (a.best_targets == tg).all() and np.unique(tg.reshape(-1, 2), axis=0).shape[0] > 1
    env.close()


def test_bad_rows_are_flagged_and_leave_the_clean_pass_alone():
    S, F = U.pkg(), FT.F()
    res, _ = RR.s1_passes()
    out, act = RR.s1_twin()
    shifted = res[2].copy()
    shifted[7, 0] += 1
    rows = np.stack([res[0], shifted, res[2]])
    o, a, status, _, _, _ = F._audit_device(_solved("s1"), rows, [0, 0, 9])
    assert list(status) == [0, S._capi.ERR_INDEX, S._capi.ERR_INDEX]
    assert (U.bits64(o[0]) == U.bits64(out[0])).all() and (a[0] == act[0]).all()       # the clean pass
    keep = np.arange(30) != 7
    assert np.isnan(o[1, 7]).all() and a[1, 7] == -1
    assert (U.bits64(o[1][keep]) == U.bits64(out[2][keep])).all() and (a[1][keep] == act[2][keep]).all()
    assert np.isnan(o[2]).all() and (a[2] == -1).all()
    with pytest.raises(S._capi.BoundsError, match="pass 1 .*first hour 7"):
        F.audit(_solved("s1"), rows, [0, 0, 9])
    with pytest.raises(S._capi.BoundsError, match="pass 2 "):
        F.audit(_solved("s1"), rows[[0, 2, 2]], [0, 0, 9])


def test_a_cuda_tensor_and_numpy_rows_give_the_same_bytes():
    import torch
    F = FT.F()
    res, _ = RR.s1_passes()
    a = F.audit(_solved("s1"), res)
    b = F.audit(_solved("s1"), torch.from_numpy(res).cuda())
    for name in ("best_q", "achieved_q", "v_state", "regret", "discretisation", "rewards"):
        assert (U.bits64(getattr(a, name)) == U.bits64(getattr(b, name))).all(), name
    assert (a.best_action == b.best_action).all() and (a.phase == b.phase).all() and (a.best_targets == b.best_targets).all()
    with pytest.raises(ValueError, match="float64 CUDA"):
        F.audit(_solved("s1"), torch.from_numpy(res))


def test_harness_regret_of_rule_pass_and_two_actors_equal_the_twin():
    """harness.regret_of on harness.inference(env, track=-1) over 30 hours, and on a two-actor inference_many with seeded random
    actors: both equal the twin on the twin's planes from row 1 (which the device's solve reproduces bit for bit)."""
    S, F = U.pkg(), FT.F()
    H = importlib.import_module(U.PKG_NAME + ".harness")
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    d, T, grid = FT.s1(), FT.S1["T"], _grid(F, FT.S1)
    tab, prof = d["tab"], d["prof"]
    V = d["V"] if d["idx0"] == 1 else FT.twin_solve(tab, prof, 1, **FT.S1)[0]
    cfgs = FT.configs(S, "s1")
    env = S.ShemsBatch(1, T, [tab], cfgs)
    _, res = H.inference(env, None, track=-1)
    assert res.shape == (T, 23)
    values = H.foresight_values(env, grid)
    assert (U.bits64(values.V.cpu().numpy()[0]) == U.bits64(V)).all()
    a = H.regret_of(env, res, values=values)
    out, act = RR.twin_audit(V, res, tab, prof, 1, **_counts(FT.S1))
    assert _same(a, out[None], act[None])
    b = H.regret_of(env, res, grid=grid)                                     # solving for itself
    assert _same(b, out[None], act[None])
    # the foresight pass on the same values: today's bytes, and regret exactly 0
    t0, r0 = H.inference_foresight(env, grid)
    t1, r1 = H.inference_foresight(env, values=values)
    assert (U.bits64(r0) == U.bits64(r1)).all() and (U.bits64(t0) == U.bits64(t1)).all()
    assert (U.bits64(H.regret_of(env, r1, values=values).regret) == 0).all()
    env.close()
    st = tab[:, [1, 1, 0, 2, 3, 4, 5, 6, 7]].copy()
    st[:, 0] = np.linspace(0, 6.75, len(st))
    actors = []
    for seed in (4, 5):
        p = D.init_params(seed, 9, 2, 0)
        p[128000:129000] *= 50
        actors.append(p)
    many = S.ShemsBatch(2, T, [tab], cfgs)
    _, resm = H.inference_many(many, np.stack(actors), st.min(0), st.max(0))
    assert resm.shape == (2, T, 23) and (U.bits64(resm[0]) != U.bits64(resm[1])).any()
    c = H.regret_of(many, resm, grid=grid)
    for e in range(2):
        out, act = RR.twin_audit(V, resm[e], tab, prof, 1, **_counts(FT.S1))
        assert _same(c, out, act, e), e
    many.close()


def test_entry_script_writes_the_regret_files_when_asked(tmp_path):
    """SHEMS_FORESIGHT_REGRET=1 on a one-episode job: a _regret.csv next to the rule-based and the foresight results files, whose rows
    parse back to the audit of those files' rows; without the variable the file list is today's."""
    M = importlib.import_module(U.PKG_NAME + ".main")
    H = importlib.import_module(U.PKG_NAME + ".harness")
    S = U.pkg()
    base = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "1", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
            "SHEMS_SYNTHETIC_DATA": "1", "SHEMS_TRAIN": "0", "SHEMS_TRACK": "-1", "SHEMS_FORESIGHT": "1"}
    cwd0 = os.getcwd()
    try:
        os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b")
        cfg, plain = M.main(base, cwd=str(tmp_path / "a"), log=lambda *_: None)
        cfg, written = M.main({**base, "SHEMS_FORESIGHT_REGRET": "1"}, cwd=str(tmp_path / "b"), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    names = [f"1179808_eval_results_{cfg.case}_rule_-1.csv", f"1179808_eval_results_{cfg.case}_foresight.csv"]
    assert [os.path.basename(w) for w in plain] == names
    assert sorted(os.listdir(tmp_path / "a" / "out" / "tracker")) == sorted(names)
    assert [os.path.basename(w) for w in written] == names + [n[:-4] + "_regret.csv" for n in names]
    for n in names:                                                          # the results files themselves are today's bytes
        assert open(tmp_path / "a" / "out" / "tracker" / n, "rb").read() == open(tmp_path / "b" / "out" / "tracker" / n, "rb").read()
    rows = [np.array(list(csv.reader(open(tmp_path / "b" / w)))[1:], np.float64) for w in written[:2]]
    tab = S.tables.load_csv(str(tmp_path / "b" / M.data_path(cfg, "eval")))
    env = S.ShemsBatch(1, 1439, [tab], [S.make_config(cfg.charger_id, 0, tab.shape[0])])
    a = H.regret_of(env, np.stack(rows))
    env.close()
    for k in range(2):
        raw = list(csv.reader(open(tmp_path / "b" / written[2 + k])))
        back = np.array(raw[1:], np.float64)
        assert raw[0] == H.REGRET_HEADER and back.shape == (1439, 11)
        want = np.stack([rows[k][:, 0], rows[k][:, 22], rows[k][:, 4], rows[k][:, 1], rows[k][:, 5], a.achieved_q[k], a.best_q[k], a.regret[k],
                         a.v_state[k], a.best_targets[k, :, 0].astype(np.float64), a.best_targets[k, :, 1].astype(np.float64)], 1)
        assert (U.bits64(back) == U.bits64(want)).all(), k
    assert (U.bits64(a.regret[1]) == 0).all() and (a.regret[0] > 0).any()   # the foresight pass against its own values

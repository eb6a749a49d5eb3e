"""The foresight audit (hourly regret of a tracked pass) without a GPU: a stand-alone host build of the header's definition against
the oracle twin on S1's three trajectories (bit for bit), the numbers the issue quotes as conditions that the inputs exercise the
feature, the telescoping identity, Audit.summary's phase sums, every refusal of the Python layer and of the entry point, the file name
and the CSV header."""
import ctypes as C
import csv
import importlib
import os
import subprocess

import numpy as np
import pytest

import foresight_regret_ref as RR
import foresight_twin as FT
import util as U


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _grid(F, shape):
    return F.Grid(shape["nb"], shape["ne"], shape["nab"], shape["nae"])


def _hostcheck(tmp_path):
    exe = str(tmp_path / "foresight_regret_hostcheck")
    src = os.path.join(U.ROOT, "tests", "hostcheck", "foresight_regret_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(U.ROOT, "include"), "-o", exe, src])
    return exe


def _run_hostcheck(exe, path, n, T):
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    q, act, status = np.zeros((n, T, 3), np.uint64), np.full((n, T), -7, np.int32), np.zeros((n, T), np.int32)
    nan = int(U.bits64(np.array([np.nan]))[0])
    for line in out.stdout.split("\n"):
        w = line.split()
        if w:
            e, t = int(w[0]), int(w[1])
            q[e, t] = [nan if x == "nan" else int(x, 16) for x in w[2:5]]
            act[e, t], status[e, t] = int(w[5]), int(w[6])
    return q, act, status


def test_host_build_of_the_definition_equals_the_twin_on_s1(tmp_path):
    """S1 (Charger98 eval, 30 hours, 9 x 5 nodes, 5 x 3 actions, start Soc_b = 0.5 soc_max): the rule-based pass, the greedy pass of
    the same V and the random-target pass, audited by a g++ build of csrc/shems_foresight_core.h, equal the twin bit for bit.  A
    fourth pass whose hour-7 row carries a shifted index is refused in that hour alone."""
    S, F = U.pkg(), FT.F()
    exe = _hostcheck(tmp_path)
    d, sh = FT.s1(), FT.S1
    g = _grid(F, sh)
    T, nrow = sh["T"], d["tab"].shape[0]
    res, _ = RR.s1_passes()
    bad = res[0].copy()
    bad[7, 0] += 1
    allp = np.concatenate([res, bad[None]])
    probs = F.make_problems([S.make_config(98, 0, nrow)], d["idx0"], T, g, nrow)
    path = str(tmp_path / "in.bin")
    with open(path, "wb") as f:
        f.write(np.array([nrow, g.nb, g.ne, g.nab, g.nae, T, 4], np.int32).tobytes())
        f.write(bytes(probs[0]))
        f.write(np.ascontiguousarray(d["tab"], np.float32).tobytes())
        f.write(np.ascontiguousarray(d["V"], np.float64).tobytes())
        f.write(np.ascontiguousarray(allp, np.float64).tobytes())
    q, act, status = _run_hostcheck(exe, path, 4, T)
    eq, ea = RR.s1_twin()
    assert (q[:3] == U.bits64(eq)).all() and (act[:3] == ea).all() and (status[:3] == 0).all()
    keep = np.arange(T) != 7
    # the hour before reads the NEXT row's state only, which the shifted index leaves alone
    assert (q[3][keep] == U.bits64(eq[0])[keep]).all() and (act[3][keep] == ea[0][keep]).all()
    assert act[3, 7] == -1 and status[3, 7] == S._capi.ERR_INDEX and (status[3][keep] == 0).all()
    assert np.isnan(q[3, 7].view(np.float64)).all()


def test_the_twin_on_s1_shows_what_the_issue_quotes():
    """Conditions that the inputs exercise the feature (the issue's table): the rule pass has >= 2 hours of positive regret and 28 of
    regret exactly 0; the random pass >= 20 positive hours; the greedy pass exactly 0.0 in all 30 hours with best_action the action
    it took."""
    out, act = RR.s1_twin()
    res, took = RR.s1_passes()
    regret = out[..., 0] - out[..., 1]
    for k, name in enumerate(("rule", "greedy", "random")):
        print(f"{name}: return {res[k][:, 5].sum():.4f}, regret > 0 in {(regret[k] > 0).sum()} hours, == 0 in {(regret[k] == 0).sum()}, "
              f"< 0 in {(regret[k] < 0).sum()}, sum {regret[k].sum():.5f}, max {regret[k].max():.4f}")
    assert (regret[0] > 0).sum() >= 2 and (regret[0] == 0).sum() == 28
    assert (regret[2] > 0).sum() >= 20
    assert (U.bits64(regret[1]) == 0).all() and (act[1] == took).all()
    assert len({int(a) for a in took}) > 2


def test_regrets_sum_to_the_gap_plus_the_discretisation_term():
    """sum_t regret = best_q[0] - return + sum_{t >= 1} discretisation within 1e-10 * max(1, max |V|): T additions of values of that
    size in float64."""
    d = FT.s1()
    out, _ = RR.s1_twin()
    res, _ = RR.s1_passes()
    tol = 1e-10 * max(1.0, float(np.abs(d["V"]).max()))
    for k in range(3):
        regret, disc = out[k, :, 0] - out[k, :, 1], out[k, :, 0] - out[k, :, 2]
        gap = regret.sum() - (out[k, 0, 0] - res[k][:, 5].sum() + disc[1:].sum())
        print(f"pass {k}: identity off by {gap:.3e} (bound {tol:.3e})")
        assert abs(gap) <= tol


def test_summary_phase_sums_add_up_and_s1_has_three_phases():
    F = FT.F()
    d, sh = FT.s1(), FT.S1
    out, act = RR.s1_twin()
    res, _ = RR.s1_passes()
    T = sh["T"]
    h_next = np.tile(d["tab"][d["idx0"]:d["idx0"] + T, 0], (3, 1))               # h_countdown of table row idx + 1
    ph = F.phases(res[..., 1], h_next)
    assert ph.shape == (3, T) and F.PHASES == ("absent", "arrival", "connected", "departure")
    for e in range(3):
        assert [int(x) for x in ph[e]] == [RR.phase_of(res[e, t, 1], h_next[e, t]) for t in range(T)]
    assert len(set(int(x) for x in ph[0])) >= 3
    a = F.Audit(out, act, _grid(F, sh).targets(), np.ascontiguousarray(res[..., 5]), ph)
    s = a.summary()
    assert (U.bits64(a.regret) == U.bits64(out[..., 0] - out[..., 1])).all() and (U.bits64(a.discretisation) == U.bits64(out[..., 0] - out[..., 2])).all()
    assert (a.best_targets == FT.action_grid(sh["nab"], sh["nae"])[act]).all() and a.best_targets.shape == (3, T, 2)
    for e in range(3):
        assert s["return"][e] == pytest.approx(res[e][:, 5].sum(), abs=1e-12)
        assert s["regret"][e] == pytest.approx(a.regret[e].sum(), abs=1e-12) and s["discretisation"][e] == pytest.approx(a.discretisation[e].sum(), abs=1e-12)
        assert sum(s[p][e] for p in F.PHASES) == pytest.approx(s["regret"][e], abs=1e-12)
        for k, p in enumerate(F.PHASES):
            assert s[p][e] == pytest.approx(a.regret[e][ph[e] == k].sum(), abs=1e-12)
    assert sum(1 for p in F.PHASES if s[p][2] != 0) >= 2


def test_audit_refuses_before_the_library_is_asked(monkeypatch):
    S, F = U.pkg(), FT.F()

    def no_lib():
        raise AssertionError("refused before the library is loaded")

    monkeypatch.setattr(S._capi, "lib", no_lib)
    g = F.Grid(9, 5, 5, 3)
    good = np.zeros((2, 5, 23))
    with pytest.raises(ValueError, match="forecast"):
        F.audit(F.Values(g, 5, [None], None, None, None, forecast_off=[40], total_rows=80), good)
    val = F.Values(g, 5, [None], None, None, None, total_rows=40)
    with pytest.raises(ValueError, match="T = 6.*5"):
        F.audit(val, np.zeros((2, 6, 23)))
    with pytest.raises(ValueError, match="T = 4.*5"):
        F.audit(val, np.zeros((4, 23)))
    for shape in ((2, 5, 22), (5, 24), (23,), (1, 2, 5, 23)):
        with pytest.raises(ValueError, match="results must be"):
            F.audit(val, np.zeros(shape))
    for po in ([0], [0, 0, 0], [[0, 0]], 0):
        with pytest.raises(ValueError, match="problem_of_pass"):
            F.audit(val, good, po)
    with pytest.raises(ValueError, match="passes"):
        F.audit(val, np.zeros((0, 5, 23)))
    with pytest.raises(AssertionError, match="before the library"):          # what is well formed does reach the library
        F.audit(val, good, [0, 0])


def test_entry_script_refuses_regret_without_foresight():
    M = importlib.import_module(U.PKG_NAME + ".main")
    assert M.foresight_regret({}) is False and M.foresight_regret({"SHEMS_FORESIGHT": "1"}) is False
    assert M.foresight_regret({"SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_REGRET": "1"}) is True
    assert M.foresight_regret({"SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_REGRET": "0"}) is False
    for env in ({"SHEMS_FORESIGHT_REGRET": "1"}, {"SHEMS_FORESIGHT_REGRET": "1", "SHEMS_FORESIGHT": "0"}):
        with pytest.raises(ValueError, match="SHEMS_FORESIGHT_REGRET.*SHEMS_FORESIGHT=1"):
            M.foresight_regret(env)
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_FORESIGHT_REGRET": "1"}
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_REGRET"):
        M.main(env, cwd="/nonexistent-directory", log=lambda *_: None)     # refused before the device or the directory is touched
    assert os.getcwd() == cwd0


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """Every SHEMS_ERR_ARG case of shems_foresight_audit_dev returns before the first HIP call, with a message (host memory stands
    in for the device pointers, which are never dereferenced on these paths)."""
    S, F = U.pkg(), FT.F()
    L = F._declare(S._capi.lib())
    g = F.Grid(9, 5, 5, 3)
    T, n = 5, 2
    tab, V = np.zeros((40, 8), np.float32), np.zeros((T + 1) * g.nodes)
    probs = F.make_problems([S.make_config(98, 0, 40)], 1, T, g, 40)
    res, out, act, status = np.zeros((n, T, 23)), np.zeros((n, T, 3)), np.zeros((n, T), np.int32), np.zeros(n, np.int32)

    def call(**kw):
        a = dict(tables=_ptr(tab), total_rows=40, prob=C.cast(probs, C.c_void_p), n_prob=1, grid=g.struct(), T=T, V=_ptr(V), vd=V.size,
                 res=_ptr(res), n=n, po=None, out=_ptr(out), act=_ptr(act), status=_ptr(status))
        a.update(kw)
        gs = a["grid"]
        rc = L.shems_foresight_audit_dev(a["tables"], a["total_rows"], a["prob"], a["n_prob"], C.byref(gs) if gs is not None else None, a["T"],
                                         a["V"], a["vd"], a["res"], a["n"], a["po"], a["out"], a["act"], a["status"], None)
        return rc, L.shems_last_error().decode()

    cases = [(dict(grid=None), "grid is NULL"), (dict(grid=F.GridStruct(1, 5, 5, 3)), "state grid"), (dict(grid=F.GridStruct(9, 5, 0, 3)), "action grid"),
             (dict(grid=F.GridStruct(200, 100, 5, 3), vd=10 ** 9), "150000"), (dict(T=0), "T = 0"), (dict(T=-3), "T = -3"),
             (dict(tables=None), "NULL"), (dict(total_rows=1), "2 table rows"), (dict(prob=None), "NULL"), (dict(n_prob=0), "no problem"),
             (dict(V=None), "NULL"), (dict(n=0), "n_pass = 0"), (dict(n=-1), "n_pass = -1"), (dict(n=65536), "n_pass = 65536"),
             (dict(res=None), "NULL"), (dict(out=None), "NULL"), (dict(act=None), "NULL"), (dict(status=None), "NULL"),
             (dict(vd=V.size - 1), "V buffer"), (dict(n_prob=2), "V buffer")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == S._capi.ERR_ARG and "shems_foresight_audit_dev" in msg and word in msg, (kw, msg)
    assert (status == 0).all() and (out == 0).all()
    assert L.shems_abi_version() == 1
    assert "shems_foresight_audit_dev" in S._capi.exported_symbols()


def test_regret_file_name_and_header(tmp_path):
    H = importlib.import_module(U.PKG_NAME + ".harness")
    F = FT.F()
    assert H.regret_file_name("out/tracker/7_eval_results_Charger98_x_foresight_h24.csv") == "out/tracker/7_eval_results_Charger98_x_foresight_h24_regret.csv"
    assert H.regret_file_name(os.path.join("a.b", "c_rule_-1.csv")) == os.path.join("a.b", "c_rule_-1_regret.csv")
    assert H.REGRET_HEADER == ["index", "Soc_b", "Soc_ev", "c_ev", "rewards", "achieved_q", "best_q", "regret", "v_state", "best_B_tar", "best_EV_tar"]
    sh = FT.S1
    out, act = RR.s1_twin()
    res, _ = RR.s1_passes()
    a = F.Audit(out, act, _grid(F, sh).targets(), np.ascontiguousarray(res[..., 5]), np.zeros(act.shape, np.int8))
    path = H.write_to_regret_file(a, res, str(tmp_path / "o" / "x_regret.csv"), pass_index=2)
    rows = list(csv.reader(open(path)))
    back = np.array(rows[1:], np.float64)
    assert rows[0] == H.REGRET_HEADER and back.shape == (sh["T"], 11)
    want = np.stack([res[2][:, 0], res[2][:, 22], res[2][:, 4], res[2][:, 1], res[2][:, 5], out[2, :, 1], out[2, :, 0], out[2, :, 0] - out[2, :, 1],
                     out[2, :, 2], a.best_targets[2, :, 0].astype(np.float64), a.best_targets[2, :, 1].astype(np.float64)], 1)
    assert (U.bits64(back) == U.bits64(want)).all()
    with pytest.raises(ValueError):
        H.write_to_regret_file(a, res[0][:-1], str(tmp_path / "o" / "y.csv"))

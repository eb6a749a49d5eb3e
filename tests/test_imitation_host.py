"""Demonstrations from tracked passes and the supervised update, without a GPU: a stand-alone host build of the header's definition
against the NumPy twin on S1's three trajectories (bit for bit, index labels and target labels, a wrapping ring), the label formula on
a 4-point axis, refused hours, every refusal of the entry point and of the Python layer, the twin's clone step against PyTorch
autograd, and the entry script's switch."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import ddpg_oracle as DO
import foresight_regret_ref as RR
import foresight_twin as FT
import imitation_ref as IR
import util as U


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _hostcheck(tmp_path):
    exe = str(tmp_path / "imitation_hostcheck")
    src = os.path.join(U.ROOT, "tests", "hostcheck", "imitation_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(U.ROOT, "include"), "-o", exe, src])
    return exe


def _run(exe, tmp_path, F, S, tab, idx0, grid, results, capacity, pos, targets=None, best_action=None):
    """Writes the input, runs the host build and returns (returncode, slot [n][T], s bits [n][T][9], a bits [n][T][2], status [n][T])."""
    res = np.ascontiguousarray(results, np.float64)
    n, T, _ = res.shape
    nrow = tab.shape[0]
    probs = F.make_problems([S.make_config(98, 0, nrow)], idx0, T, grid, nrow)
    path = str(tmp_path / "in.bin")
    with open(path, "wb") as f:
        f.write(np.array([nrow, grid.nb, grid.ne, grid.nab, grid.nae, T, n, 0 if targets is not None else 1], np.int32).tobytes())
        f.write(np.array([capacity, pos], np.int64).tobytes())
        f.write(bytes(probs[0]))
        f.write(np.ascontiguousarray(tab, np.float32).tobytes())
        f.write(res.tobytes())
        f.write(np.ascontiguousarray(targets, np.float32).tobytes() if targets is not None else np.ascontiguousarray(best_action, np.int32).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True)
    slot, status = np.full((n, T), -7, np.int64), np.zeros((n, T), np.int32)
    s, a = np.zeros((n, T, 9), np.uint32), np.zeros((n, T, 2), np.uint32)
    if out.returncode == 0:
        for line in out.stdout.split("\n"):
            w = line.split()
            if w:
                e, t = int(w[0]), int(w[1])
                slot[e, t] = int(w[2])
                if slot[e, t] < 0:
                    status[e, t] = int(w[3])
                else:
                    s[e, t] = [int(x, 16) for x in w[3:12]]
                    a[e, t] = [int(x, 16) for x in w[12:14]]
    return out, slot, s, a, status


def _s1(F):
    d, sh = FT.s1(), FT.S1
    return d, sh, F.Grid(sh["nb"], sh["ne"], sh["nab"], sh["nae"])


def test_host_build_of_the_definition_equals_the_twin_on_s1(tmp_path):
    """S1's rule-based, greedy and random passes into a ring of 128 slots from slot 100 (the 90 pairs wrap), once with the audit's
    action indices and once with the targets of those actions: a g++ build of fs_demo_hour / fs_demo_slot equals the twin bit for
    bit.  The labels are k/4 and k/2, dyadic, so scale_action of the label is the target exactly."""
    S, F = U.pkg(), FT.F()
    exe = _hostcheck(tmp_path)
    d, sh, g = _s1(F)
    res, _ = RR.s1_passes()
    _, best = RR.s1_twin()
    tgt = FT.action_grid(sh["nab"], sh["nae"])[best]                        # [3][30][2]
    for kw in (dict(best_action=best), dict(targets=tgt)):
        out, slot, s, a, status = _run(exe, tmp_path, F, S, d["tab"], d["idx0"], g, res, 128, 100, **kw)
        assert out.returncode == 0, out.stderr
        ws, wS, wA, wst = IR.twin_demos(res, d["tab"], d["idx0"], sh["nab"], sh["nae"], pos=100, capacity=128, **kw)
        assert (wst == 0).all() and (status == 0).all()
        assert (slot == ws).all() and (s == U.bits32(wS)).all() and (a == U.bits32(wA)).all()
        assert slot[0, 0] == 100 and slot[0, 28] == 0 and slot[2, 29] == 61 and len(np.unique(slot)) == 90      # wraps, no slot twice
        assert (U.bits32(IR.scale_action(wA)) == U.bits32(tgt)).all()       # dyadic labels: the inverse of scale_action is exact
        assert (wA.min() == -1.0) and (wA.max() == 1.0)                     # labels at the ends of the action range saturate the tanh
    # the observation is what the env showed before the step: obs_of_rows on the start row for hour 0, the table's columns after
    assert (U.bits32(wS[:, 0]) == U.bits32(np.repeat(U.obs_of_rows(d["tab"], np.array([d["idx0"]]),
                                                                   np.array([0.5 * float(d["prof"].soc_max)], np.float32)), 3, 0))).all()
    assert (U.bits32(wS[0, :, 3:]) == U.bits32(d["tab"][d["idx0"] - 1:d["idx0"] - 1 + sh["T"], 2:])).all()


def test_a_four_point_axis_is_held_to_the_label_formula(tmp_path):
    """Thirds are not dyadic: the label is float32(2.0 * float64(target) - 1.0) and nothing more is claimed (scale_action of it may be
    one float32 rounding away from the target)."""
    S, F = U.pkg(), FT.F()
    exe = _hostcheck(tmp_path)
    d, sh, _ = _s1(F)
    g = F.Grid(sh["nb"], sh["ne"], 4, 4)
    res, _ = RR.s1_passes()
    act = (np.arange(90).reshape(3, 30) * 7) % 16
    out, slot, s, a, status = _run(exe, tmp_path, F, S, d["tab"], d["idx0"], g, res, 90, 0, best_action=act)
    assert out.returncode == 0, out.stderr
    third = FT.targets(4)
    want = np.stack([IR.label(third[act // 4]), IR.label(third[act % 4])], -1)
    assert (a == U.bits32(want)).all() and (status == 0).all() and (slot == np.arange(90).reshape(3, 30)).all()
    assert np.abs(IR.scale_action(want) - np.stack([third[act // 4], third[act % 4]], -1)).max() <= np.spacing(np.float32(1.0))
    _, _, wA, _ = IR.twin_demos(res, d["tab"], d["idx0"], 4, 4, best_action=act)
    assert (a == U.bits32(wA)).all()


def test_refused_hours_leave_their_slot_and_flag_the_pass(tmp_path):
    S, F = U.pkg(), FT.F()
    exe = _hostcheck(tmp_path)
    d, sh, g = _s1(F)
    res, _ = RR.s1_passes()
    _, best = RR.s1_twin()
    bad = res.copy()
    bad[1, 7, 0] += 1                                                       # a shifted row index
    bad[2, 3, 0] = np.nan
    act = best.copy()
    act[0, 11] = -1                                                         # the audit's "no action"
    act[0, 12] = sh["nab"] * sh["nae"]                                      # past the grid
    out, slot, s, a, status = _run(exe, tmp_path, F, S, d["tab"], d["idx0"], g, bad, 128, 100, best_action=act)
    assert out.returncode == 0, out.stderr
    ws, wS, wA, wst = IR.twin_demos(bad, d["tab"], d["idx0"], sh["nab"], sh["nae"], best_action=act, pos=100, capacity=128)
    assert (wst == S._capi.ERR_INDEX).all()
    refused = [(0, 11), (0, 12), (1, 7), (2, 3)]
    for e, t in refused:
        assert slot[e, t] == -1 and status[e, t] == S._capi.ERR_INDEX and ws[e, t] == -1
    keep = np.ones((3, 30), bool)
    keep[tuple(zip(*refused))] = False
    assert (slot[keep] == ws[keep]).all() and (s[keep] == U.bits32(wS)[keep]).all() and (a[keep] == U.bits32(wA)[keep]).all()
    S0, A0 = np.full((128, 9), 7.5, np.float32), np.full((128, 2), -7.5, np.float32)
    rs, ra = IR.fill(ws, wS, wA, 128, (S0, A0))
    for e, t in refused:                                                    # the slot the hour would have taken keeps its sentinel
        k = (100 + e * 30 + t) % 128
        assert (rs[k] == 7.5).all() and (ra[k] == -7.5).all()
    assert (rs != 7.5).any(1).sum() == 86
    # with targets an index of -1 plays no part: only the row check refuses
    tgt = FT.action_grid(sh["nab"], sh["nae"])[best]
    out, slot, *_ = _run(exe, tmp_path, F, S, d["tab"], d["idx0"], g, bad, 128, 100, targets=tgt)
    assert (np.argwhere(slot < 0) == [[1, 7], [2, 3]]).all()


def test_host_build_refuses_what_the_ring_cannot_hold(tmp_path):
    S, F = U.pkg(), FT.F()
    exe = _hostcheck(tmp_path)
    d, sh, g = _s1(F)
    res, _ = RR.s1_passes()
    _, best = RR.s1_twin()
    for cap, pos, word in ((89, 0, "ring 2"), (90, 90, "ring 3"), (90, -1, "ring 3"), (0, 0, "ring 1")):
        out, *_ = _run(exe, tmp_path, F, S, d["tab"], d["idx0"], g, res, cap, pos, best_action=best)
        assert out.returncode == 3 and out.stdout.strip() == word, (cap, pos, out.stdout)


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """Every SHEMS_ERR_ARG case of shems_foresight_demos_dev returns before the first HIP call, with a message (host memory stands in
    for the device pointers, which are never dereferenced on these paths)."""
    S, F = U.pkg(), FT.F()
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    L = I._declare(S._capi.lib())
    g = F.Grid(9, 5, 5, 3)
    T, n, cap = 5, 2, 16
    tab = np.zeros((40, 8), np.float32)
    probs = F.make_problems([S.make_config(98, 0, 40)], 1, T, g, 40)
    res, tgt, act, status = np.zeros((n, T, 23)), np.zeros((n, T, 2), np.float32), np.zeros((n, T), np.int32), np.zeros(n, np.int32)
    rs_, ra_, rr_, r2_, rd_ = np.zeros((cap, 9), np.float32), np.zeros((cap, 2), np.float32), np.zeros(cap, np.float32), np.zeros((cap, 9), np.float32), np.zeros(cap, np.uint8)

    def ring(capacity=cap, s=rs_, a=ra_):
        return S._capi.Replay(capacity, s.ctypes.data if s is not None else None, a.ctypes.data if a is not None else None, rr_.ctypes.data,
                              r2_.ctypes.data, rd_.ctypes.data)

    def call(**kw):
        a = dict(tables=_ptr(tab), total_rows=40, prob=C.cast(probs, C.c_void_p), n_prob=1, grid=g.struct(), T=T, res=_ptr(res), n=n, po=None,
                 tgt=_ptr(tgt), act=None, ring=ring(), pos=0, status=_ptr(status))
        a.update(kw)
        gs, rg = a["grid"], a["ring"]
        rc = L.shems_foresight_demos_dev(a["tables"], a["total_rows"], a["prob"], a["n_prob"], C.byref(gs) if gs is not None else None, a["T"],
                                         a["res"], a["n"], a["po"], a["tgt"], a["act"], C.byref(rg) if rg is not None else None, a["pos"],
                                         a["status"], None)
        return rc, L.shems_last_error().decode()

    cases = [(dict(grid=None), "grid is NULL"), (dict(grid=F.GridStruct(1, 5, 5, 3)), "state grid"), (dict(grid=F.GridStruct(9, 5, 0, 3)), "action grid"),
             (dict(grid=F.GridStruct(200, 100, 5, 3)), "150000"), (dict(T=0), "T = 0"), (dict(T=-3), "T = -3"),
             (dict(tables=None), "NULL"), (dict(total_rows=1), "2 table rows"), (dict(prob=None), "NULL"), (dict(n_prob=0), "no problem"),
             (dict(n=0), "n_pass = 0"), (dict(n=-1), "n_pass = -1"), (dict(n=65536), "n_pass = 65536"),
             (dict(res=None), "NULL"), (dict(status=None), "NULL"),
             (dict(act=_ptr(act)), "both"), (dict(tgt=None), "neither"),
             (dict(ring=None), "NULL ring"), (dict(ring=ring(s=None)), "without s or a"), (dict(ring=ring(a=None)), "without s or a"),
             (dict(ring=ring(capacity=0)), "capacity is 0"), (dict(ring=ring(capacity=9)), "10 pairs"), (dict(n=4), "20 pairs"),
             (dict(pos=-1), "pos = -1"), (dict(pos=cap), f"pos = {cap}")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == S._capi.ERR_ARG and "shems_foresight_demos_dev" in msg and word in msg, (kw, msg)
    assert (status == 0).all() and not rs_.any() and not ra_.any()
    assert {"shems_foresight_demos_dev", "shems_ddpg_clone_update"} <= set(S._capi.exported_symbols())


def test_python_layer_refuses_before_the_library_is_asked(monkeypatch):
    S, F = U.pkg(), FT.F()
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    M = importlib.import_module(U.PKG_NAME + ".main")

    def no_lib():
        raise AssertionError("refused before the library is loaded")

    monkeypatch.setattr(S._capi, "lib", no_lib)
    g = F.Grid(9, 5, 5, 3)
    good = np.zeros((2, 5, 23))
    belief = F.Values(g, 5, [None], None, None, None, forecast_off=[40], total_rows=80)
    with pytest.raises(ValueError, match="forecast"):
        I.from_pass(belief, good, None)
    ens = F.EnsembleValues(F.Values(g, 5, [None, None], None, None, None, forecast_off=[40, 80], total_rows=120), 2, np.full((1, 2), 0.5))
    for fn in (lambda: I.from_pass(ens, good, None), lambda: I.dagger(None, None, ens, None, 2, 3)):
        with pytest.raises(ValueError, match="ensemble"):
            fn()
    val = F.Values(g, 5, [None], None, None, None, total_rows=40)
    with pytest.raises(ValueError, match="T = 6.*5"):
        I.from_pass(val, np.zeros((2, 6, 23)), None)
    for r, s in ((0, 5), (2, 0)):
        with pytest.raises(ValueError, match="at least one"):
            I.dagger(None, None, val, None, r, s)
    # the entry script's switch
    assert M.foresight_imitate({}) is None and M.foresight_imitate({"SHEMS_FORESIGHT": "1"}) is None
    assert M.foresight_imitate({"SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_IMITATE": "3x200"}) == (3, 200)
    for raw in ("3", "x", "3x", "0x5", "3x0", "axb", "1x2x3"):
        with pytest.raises(ValueError, match="SHEMS_FORESIGHT_IMITATE"):
            M.foresight_imitate({"SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_IMITATE": raw})
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_IMITATE.*SHEMS_FORESIGHT=1"):
        M.foresight_imitate({"SHEMS_FORESIGHT_IMITATE": "2x2"})
    assert M.imitation_file_name(7, "eval", "Charger98_x") == os.path.join("out/tracker", "7_eval_results_Charger98_x_imitation.csv")
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_IMITATE"):
        M.main({"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_FORESIGHT_IMITATE": "2x2"}, cwd="/nonexistent-directory", log=lambda *_: None)
    assert os.getcwd() == cwd0


def test_twin_clone_gradient_equals_autograd():
    """The twin's d Flux.mse(actor(x), a_demo) / d actor against PyTorch autograd in float64, and the loss's normalisation (the mean
    over 2 * batch elements)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    p = DO.init_params(7, 9, 2, 0)
    p[128000:129000] *= 30.0
    B = 7
    s = rng.random((B, 9)).astype(np.float32)
    a = np.clip(rng.normal(0, 1, (B, 2)), -1, 1).astype(np.float32)
    lo, hi = np.zeros(9, np.float32), np.ones(9, np.float32)
    g, loss = IR.clone_grad(p, s, a, lo, hi, dtype=np.float64)
    P = torch.tensor(p.astype(np.float64), requires_grad=True)
    W1, b1, W2, b2, W3, b3 = (P[lo_:hi_] for _, lo_, hi_ in DO.blocks(9, 2))
    x = torch.tensor(DO.normalize(s, lo, hi).astype(np.float64))
    y = torch.tanh(torch.relu(torch.relu(x @ W1.reshape(9, 250) + b1) @ W2.reshape(250, 500) + b2) @ W3.reshape(500, 2) + b3)
    l = ((y - torch.tensor(a.astype(np.float64))) ** 2).mean()
    l.backward()
    assert abs(loss - float(l.detach())) < 1e-14
    assert np.abs(g - P.grad.numpy()).max() < 1e-14 and np.abs(g).max() > 1e-4
    L = IR.CloneLearner(p, lo, hi)
    before = L.actor.copy()
    L.clone(s, a, B, seed=5, tick=0, batch=4, tau=1.0)
    assert (L.actor != before).any() and (U.bits32(L.actor_t) == U.bits32(L.actor)).all()      # tau = 1: 1 p + 0 t

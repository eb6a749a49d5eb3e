"""The perfect-foresight controller without a GPU: the recursion of csrc/shems_foresight_core.h compiled as host C++ against a float64
NumPy twin on the C oracle (bit for bit), the host restatements of foresight.py, argument refusals, file name, MPC fixture."""
import ctypes as C
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import foresight_twin as FT
import util as U


def _hostcheck():
    d = os.path.join(U.ROOT, "tests", "hostcheck")
    so, src = os.path.join(d, "libforesight_hostcheck.so"), os.path.join(d, "foresight_hostcheck.cpp")
    deps = [src] + [os.path.join(U.ROOT, U.PKG_NAME, "csrc", h) for h in ("shems_core.h", "shems_foresight_core.h")] + \
        [os.path.join(U.ROOT, "include", "shems_hip.h")]
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(U.ROOT, "include"), "-o", so, src])
    return C.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_build_of_the_recursion_equals_the_oracle_twin_on_s1():
    """Shape S1 (Charger98 eval, 30 hours, 9 x 5 nodes, 5 x 3 actions): every V plane and every arg-max index of the header's host
    build equals the twin's, bit for bit."""
    S, F = U.pkg(), FT.F()
    d = FT.s1()
    assert all(FT.window_features(d["tab"], d["idx0"], FT.S1["T"]))        # arrival, h == 0, g_e > d_e, g_e <= d_e
    print("S1 window starts at row", d["idx0"])
    g = F.Grid(FT.S1["nb"], FT.S1["ne"], FT.S1["nab"], FT.S1["nae"])
    probs = F.make_problems(FT.configs(S, "s1"), d["idx0"], FT.S1["T"], g, d["tab"].shape[0])
    T, N = FT.S1["T"], g.nodes
    V, arg = np.full((T + 1, N), np.nan), np.full((T, N), -1, np.int32)
    L = _hostcheck()
    gs = g.struct()
    tab = np.ascontiguousarray(d["tab"], np.float32)
    assert L.fhc_solve(_ptr(tab), C.byref(probs[0]), C.byref(gs), T, _ptr(V), _ptr(arg)) == 0
    assert (U.bits64(V) == U.bits64(d["V"])).all()
    assert (arg == d["arg"]).all()
    assert np.unique(arg).size > 3 and (V[0] != V[0][0]).any()             # not a degenerate comparison


def test_host_restatements_of_nodes_targets_and_interpolation():
    S, F = U.pkg(), FT.F()
    L = _hostcheck()
    rng = np.random.default_rng(5)
    for (nb, ne, nab, nae), cid in (((9, 5, 5, 3), 98), ((33, 9, 4, 7), 5), ((65, 33, 17, 17), 1), ((2, 2, 1, 1), 4)):
        g = F.Grid(nb, ne, nab, nae)
        cfg = S.make_config(cid, 0, 100)
        p = F.make_problems([cfg], 1, 5, g)
        sb, se, bt, et = (np.zeros(k, np.float32) for k in (nb, ne, nab, nae))
        gs = g.struct()
        L.fhc_nodes(C.byref(p[0]), C.byref(gs), _ptr(sb), _ptr(se), _ptr(bt), _ptr(et))
        for mine, twin, c in ((g.soc_b_nodes(cfg.soc_max), FT.nodes(nb, cfg.soc_max), sb), (g.soc_ev_nodes(), FT.nodes(ne, 1.0), se),
                              (g.b_targets(), FT.targets(nab), bt), (g.ev_targets(), FT.targets(nae), et)):
            assert (U.bits32(mine) == U.bits32(c)).all() and (U.bits32(twin) == U.bits32(c)).all()
        assert sb[-1] == np.float32(cfg.soc_max) and se[-1] == 1.0 and sb[0] == 0.0 and bt[-1] == 1.0
        assert (g.targets() == FT.action_grid(nab, nae)).all() and g.targets().shape == (nab * nae, 2)
        # interpolation: on the nodes, between them, and outside the grid (clamped to the edge cell)
        plane = rng.standard_normal(nb * ne)
        xb = np.concatenate([np.repeat(sb, ne), (rng.random(200) * 1.2 - 0.1) * cfg.soc_max]).astype(np.float32)
        xe = np.concatenate([np.tile(se, nb), rng.random(200) * 1.2 - 0.1]).astype(np.float32)
        out = np.zeros(len(xb))
        L.fhc_value(_ptr(plane), C.byref(p[0]), C.byref(gs), _ptr(xb), _ptr(xe), len(xb), _ptr(out))
        assert (U.bits64(F.interpolate(plane, g, cfg.soc_max, xb, xe)) == U.bits64(out)).all()
        assert (U.bits64(FT.interp(plane, nb, ne, cfg.soc_max, xb, xe)) == U.bits64(out)).all()
        assert (U.bits64(out[:nb * ne]) == U.bits64(plane)).all()          # a node reads its own value exactly
    assert F.Grid().nodes == 65 * 33 and F.Grid().actions == 289
    mid = np.float32(0.5 * float(S.make_config(98, 0, 10).soc_max))         # reset!(rng = -1): 0.5 * soc_max is a node of the default grid
    assert mid in F.Grid().soc_b_nodes(S.make_config(98, 0, 10).soc_max)


def test_grid_and_solve_refuse_bad_arguments():
    S, F = U.pkg(), FT.F()
    for bad in ((1, 5, 3, 3), (5, 1, 3, 3), (5, 5, 0, 3), (5, 5, 3, 0), (200, 200, 3, 3)):
        with pytest.raises(ValueError):
            F.Grid(*bad)
    tab = U.tables_mod().synthetic_table("eval", 98)
    cfg = S.make_config(98, 0, tab.shape[0])
    g = F.Grid(9, 5, 5, 3)
    for kw in (dict(idx0=1, nsteps=0), dict(idx0=0, nsteps=5), dict(idx0=tab.shape[0] - 4, nsteps=5), dict(idx0=[1, 2], nsteps=5)):
        with pytest.raises(ValueError):
            F.solve([tab], [cfg], grid=g, **kw)                             # refused on the host, before any device work
    with pytest.raises(ValueError):
        F.solve([tab], [], 1, 5, g)
    with pytest.raises(ValueError):
        F.solve([tab], [S.make_config(98, 10, tab.shape[0])], 1, 5, g)     # the config names rows beyond the uploaded tables
    with pytest.raises(ValueError):
        F.solve([tab[:, :7]], [cfg], 1, 5, g)
    assert F.make_problems([cfg], tab.shape[0] - 5, 5, g)[0].idx0 == tab.shape[0] - 5      # the last window that fits


def test_entry_points_refuse_bad_arguments_before_any_launch(built_lib):
    """Every SHEMS_ERR_ARG case of shems_foresight_solve_dev returns before the first HIP call, with a message: that can be asked
    without a device (the pointers are never dereferenced on these paths; host memory stands in for them)."""
    S, F = U.pkg(), FT.F()
    L = F._declare(S._capi.lib())
    tab = np.zeros((40, 8), np.float32)
    cfg = S.make_config(98, 0, 40)
    g = F.Grid(9, 5, 5, 3)
    T, N = 5, g.nodes
    V = np.zeros((T + 1) * N)
    probs = F.make_problems([cfg], 1, T, g, 40)

    def call(grid=None, T=T, probs=probs, vd=V.size):
        gs = grid if grid is not None else g.struct()
        rc = L.shems_foresight_solve_dev(_ptr(tab), 40, probs, C.cast(probs, C.c_void_p), 1, C.byref(gs), T, _ptr(V), vd, None, None)
        return rc, L.shems_last_error().decode()

    for grid, word in ((F.GridStruct(1, 5, 5, 3), "state grid"), (F.GridStruct(9, 1, 5, 3), "state grid"), (F.GridStruct(9, 5, 0, 3), "action grid"),
                       (F.GridStruct(9, 5, 5, 0), "action grid")):
        rc, msg = call(grid=grid)
        assert rc == S._capi.ERR_ARG and word in msg, msg
    rc, msg = call(T=0)
    assert rc == S._capi.ERR_ARG and "horizon" in msg
    off = F.make_problems([cfg], 1, T, g, 40)
    off[0].idx0 = 36                                                        # rows 36 .. 41 of 40
    rc, msg = call(probs=off)
    assert rc == S._capi.ERR_ARG and "runs off its table" in msg
    off[0].idx0 = 0
    assert call(probs=off)[0] == S._capi.ERR_ARG
    rc, msg = call(vd=V.size - 1)
    assert rc == S._capi.ERR_ARG and "V buffer" in msg
    wrong = F.make_problems([cfg], 1, T, g, 40)
    wrong[0].cfg.soc_max = 0.0
    rc, msg = call(probs=wrong)
    assert rc == S._capi.ERR_ARG and "soc_max" in msg


def test_foresight_file_name_and_mpc_fixture():
    H = importlib.import_module(U.PKG_NAME + ".harness")
    name = H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=os.path.join("out", "tracker"))
    assert name == os.path.join("out", "tracker", "11709800_eval_results_Charger98_dw0.01_foresight.csv")
    fx = json.load(open(os.path.join(U.ROOT, "tests", "golden", "mpc_profit_sums.json")))
    T = U.tables_mod()
    assert tuple(sorted(fx)) == T.real_series_keys()
    for k, v in fx.items():
        assert v["rows"] == T.real_series(int(k[7:9]), k.split("_")[1]).shape[0]          # one row per MPC decision
        assert v["profits_is"] in ("total_repeated", "per_hour", "running_total") and np.isfinite([v["profits_sum"], v["ext_ev_sum"]]).all()
        if v["profits_is"] == "total_repeated":
            assert v["profits_sum"] == pytest.approx(v["rows"] * v["profit_total"], rel=1e-9)

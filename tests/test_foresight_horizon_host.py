"""The receding-horizon foresight controller without a GPU: the schedule (foresight.horizon_plan and the header's helpers compiled as
host C++) against the brute-force definition, a host loop over the helpers against the oracle twin on every truncated window (bit
for bit), every refusal of the Python layer and of the entry point, file names, the entry script's variables."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import foresight_horizon_ref as FR
import foresight_twin as FT
import util as U

CASES = [(T, H, c) for T in (1, 8, 30) for H in range(1, T + 4) for c in range(1, H + 1)]


def _hostcheck():
    d = os.path.join(U.ROOT, "tests", "hostcheck")
    so, src = os.path.join(d, "libforesight_horizon_hostcheck.so"), os.path.join(d, "foresight_horizon_hostcheck.cpp")
    deps = [src] + [os.path.join(U.ROOT, U.PKG_NAME, "csrc", h) for h in ("shems_core.h", "shems_foresight_core.h")] + \
        [os.path.join(U.ROOT, "include", "shems_hip.h")]
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(U.ROOT, "include"), "-o", so, src])
    return C.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_horizon_plan_equals_the_brute_force_definition():
    F = FT.F()
    for T, H, c in CASES:
        j, k = F.horizon_plan(T, H, c)
        bj, bk = FR.brute_plan(T, H, c)
        assert j.shape == (T,) and k.shape == (T,) and (j == bj).all() and (k == bk).all(), (T, H, c)
        assert (k >= 0).all() and (k <= H - 1).all() and k[-1] == 0
    assert (F.horizon_plan(8, 3)[0] == np.arange(8)).all()                   # control defaults to 1
    for bad in ((0, 1, 1), (5, 0, 1), (5, 3, 0), (5, 3, 4)):
        with pytest.raises(ValueError):
            F.horizon_plan(*bad)


def test_header_schedule_helpers_equal_horizon_plan_and_keep_every_plane_once():
    """The SHEMS_HD helpers the kernel and the entry point share: j and the look-ahead length of every hour as horizon_plan gives
    them; the windows' (j, hi, first hour, keep) from the definition; every plane 0 .. T and (when asked for) every arg-max 0 .. T - 1
    kept by exactly one window -- without arg-max plane 0 still comes from window 0."""
    F, L = FT.F(), _hostcheck()
    for T, H, c in CASES:
        j, k = np.zeros(T, np.int64), np.zeros(T, np.int64)
        L.fhh_plan(T, H, c, _ptr(j), _ptr(k))
        pj, pk = F.horizon_plan(T, H, c)
        assert (j == pj).all() and (k == pk).all(), (T, H, c)
        for want in (1, 0):
            W = -(-T // c)
            win, pf, af = np.zeros((W, 4), np.int32), np.zeros(T + 1, np.int32), np.zeros(T, np.int32)
            assert L.fhh_windows(T, H, c, want, _ptr(win), _ptr(pf), _ptr(af)) == W
            for w in range(W):
                made = w * c
                assert tuple(win[w]) == (made, min(made + H, T), made if (want or made == 0) else made + 1, min(made + c, T)), (T, H, c, w)
            assert (pf == 1).all() and (af == want).all(), (T, H, c, want)
    # sizes near the top of an int: no sum in the helpers overflows
    big = 2 ** 31 - 1
    j, k = np.zeros(8, np.int64), np.zeros(8, np.int64)
    L.fhh_plan(8, big, big, _ptr(j), _ptr(k))
    assert (j == 0).all() and (k == 7 - np.arange(8)).all()


def test_host_loop_over_the_helpers_equals_the_twin_on_every_truncated_window():
    """S1 with (H, c) = (6, 4): windows made at 0, 4, .., 28 -- the last two truncated at the series end, the last one ragged (2 of 4
    hours).  V and arg-max of the header's host build equal, bit for bit, the twin solved on each window on its own."""
    S, F, L = U.pkg(), FT.F(), _hostcheck()
    d = FT.s1()
    g = F.Grid(FT.S1["nb"], FT.S1["ne"], FT.S1["nab"], FT.S1["nae"])
    T, N, H, c = FT.S1["T"], g.nodes, 6, 4
    probs = F.make_problems(FT.configs(S, "s1"), d["idx0"], T, g, d["tab"].shape[0])
    gs = g.struct()
    tab = np.ascontiguousarray(d["tab"], np.float32)
    V, arg = np.full((T + 1, N), np.nan), np.full((T, N), -1, np.int32)
    assert L.fhh_solve_horizon(_ptr(tab), C.byref(probs[0]), C.byref(gs), T, H, c, _ptr(V), _ptr(arg)) == 0
    eV, eA = FR.expected("s1", 0, H, c)
    assert (U.bits64(V) == U.bits64(eV)).all() and (arg == eA).all()
    assert (V[T] == 0).all() and (U.bits64(V[1:T - H + 1]) != U.bits64(d["V"][1:T - H + 1])).any(axis=1).all()      # not the full solve
    # without arg-max the planes are the same (hour j is then swept by window 0 only)
    V2 = np.full((T + 1, N), np.nan)
    assert L.fhh_solve_horizon(_ptr(tab), C.byref(probs[0]), C.byref(gs), T, H, c, _ptr(V2), None) == 0
    assert (U.bits64(V2) == U.bits64(eV)).all()
    # H >= T: the full solve, whatever c
    for HH, cc in ((30, 7), (1000, 1)):
        V3, a3 = np.full((T + 1, N), np.nan), np.full((T, N), -1, np.int32)
        assert L.fhh_solve_horizon(_ptr(tab), C.byref(probs[0]), C.byref(gs), T, HH, cc, _ptr(V3), _ptr(a3)) == 0
        assert (U.bits64(V3) == U.bits64(d["V"])).all() and (a3 == d["arg"]).all()


def test_solve_horizon_refuses_bad_arguments_on_the_host():
    S, F = U.pkg(), FT.F()
    tab = U.tables_mod().synthetic_table("eval", 98)
    cfg = S.make_config(98, 0, tab.shape[0])
    g = F.Grid(9, 5, 5, 3)
    for kw, word in ((dict(horizon=0), "horizon"), (dict(horizon=3, control=0), "control"), (dict(horizon=3, control=4), "control"),
                     (dict(horizon=None), "horizon")):
        with pytest.raises(ValueError, match=word):
            F.solve_horizon([tab], [cfg], 1, 5, grid=g, **kw)
    with pytest.raises(ValueError, match="160000.*150000"):                 # two planes of 100 x 100 nodes; one plane is admitted
        F.solve_horizon([tab], [cfg], 1, 5, 3, grid=F.Grid(100, 100, 3, 3))
    for kw in (dict(idx0=1, nsteps=0), dict(idx0=0, nsteps=5), dict(idx0=tab.shape[0] - 4, nsteps=5), dict(idx0=[1, 2], nsteps=5)):
        with pytest.raises(ValueError):
            F.solve_horizon([tab], [cfg], horizon=3, grid=g, **kw)          # what solve refuses
    with pytest.raises(ValueError):
        F.solve_horizon([tab], [], 1, 5, 3, grid=g)
    H = importlib.import_module(U.PKG_NAME + ".harness")
    G = importlib.import_module(U.PKG_NAME + ".group")
    import inspect
    for fn in (H.inference_foresight, G.foresight_scores):
        sig = inspect.signature(fn).parameters
        assert sig["horizon"].default is None and sig["control"].default == 1


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """Every SHEMS_ERR_ARG case of shems_foresight_solve_horizon_dev returns before the first HIP call, with a message: that can be
    asked without a device (the pointers are never dereferenced on these paths; host memory stands in for them)."""
    S, F = U.pkg(), FT.F()
    L = F._declare(S._capi.lib())
    tab = np.zeros((40, 8), np.float32)
    cfg = S.make_config(98, 0, 40)
    g = F.Grid(9, 5, 5, 3)
    T = 5
    V = np.zeros((T + 1) * 129 * 65)
    probs = F.make_problems([cfg], 1, T, g, 40)

    def call(grid=None, T=T, probs=probs, vd=(T + 1) * g.nodes, H=3, c=1):
        gs = grid if grid is not None else g.struct()
        rc = L.shems_foresight_solve_horizon_dev(_ptr(tab), 40, probs, C.cast(probs, C.c_void_p), 1, C.byref(gs), T, H, c, _ptr(V), vd, None, None)
        return rc, L.shems_last_error().decode()

    for kw, word in ((dict(H=0), "horizon"), (dict(H=-2), "horizon"), (dict(c=0), "control"), (dict(H=3, c=4), "control")):
        rc, msg = call(**kw)
        assert rc == S._capi.ERR_ARG and word in msg and "shems_foresight_solve_horizon_dev" in msg, msg
    # the two-plane LDS limit: 100 x 100 nodes = 160 000 bytes is refused with both numbers; 129 x 65 = 134 160 bytes passes the
    # argument check (asked with a V buffer one float64 short, so that the call still returns before any HIP call)
    rc, msg = call(grid=F.GridStruct(100, 100, 5, 3), vd=(T + 1) * 10000)
    assert rc == S._capi.ERR_ARG and "160000" in msg and "150000" in msg, msg
    rc, msg = call(grid=F.GridStruct(129, 65, 5, 3), vd=(T + 1) * 129 * 65 - 1)
    assert rc == S._capi.ERR_ARG and "V buffer" in msg, msg
    assert F.Grid(100, 100).nodes * 8 <= F.MAX_PLANE_BYTES                  # solve's one-plane limit admits what two planes do not
    # everything solve_dev refuses
    for grid, word in ((F.GridStruct(1, 5, 5, 3), "state grid"), (F.GridStruct(9, 1, 5, 3), "state grid"), (F.GridStruct(9, 5, 0, 3), "action grid"),
                       (F.GridStruct(9, 5, 5, 0), "action grid"), (F.GridStruct(200, 200, 3, 3), "LDS")):
        rc, msg = call(grid=grid)
        assert rc == S._capi.ERR_ARG and word in msg, msg
    rc, msg = call(T=0)
    assert rc == S._capi.ERR_ARG and "at least 1 hour" in msg
    off = F.make_problems([cfg], 1, T, g, 40)
    off[0].idx0 = 36                                                        # rows 36 .. 41 of 40
    rc, msg = call(probs=off)
    assert rc == S._capi.ERR_ARG and "runs off its table" in msg
    off[0].idx0 = 0
    assert call(probs=off)[0] == S._capi.ERR_ARG
    rc, msg = call(vd=(T + 1) * g.nodes - 1)
    assert rc == S._capi.ERR_ARG and "V buffer" in msg
    wrong = F.make_problems([cfg], 1, T, g, 40)
    wrong[0].cfg.soc_max = 0.0
    rc, msg = call(probs=wrong)
    assert rc == S._capi.ERR_ARG and "soc_max" in msg
    assert L.shems_abi_version() == 1


def test_file_names_and_tracker_seeds_carry_the_horizon():
    H = importlib.import_module(U.PKG_NAME + ".harness")
    d = os.path.join("out", "tracker")
    base = os.path.join(d, "11709800_eval_results_Charger98_dw0.01_foresight")
    assert H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=d) == base + ".csv"
    assert H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=d, horizon=None, control=1) == base + ".csv"
    assert H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=d, horizon=24) == base + "_h24.csv"
    assert H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=d, horizon=24, control=1) == base + "_h24.csv"
    assert H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=d, horizon=24, control=12) == base + "_h24_c12.csv"
    assert (H.foresight_seed(), H.foresight_seed(24), H.foresight_seed(24, 12)) == ("foresight", "foresight_h24", "foresight_h24_c12")


def test_entry_script_reads_horizon_and_control_and_refuses_malformed_values():
    M = importlib.import_module(U.PKG_NAME + ".main")
    assert M.foresight_horizons({}) == ([], 1)
    assert M.foresight_horizons({"SHEMS_FORESIGHT_HORIZON": "24"}) == ([24], 1)
    assert M.foresight_horizons({"SHEMS_FORESIGHT_HORIZON": "6,24", "SHEMS_FORESIGHT_CONTROL": "6"}) == ([6, 24], 6)
    assert M.foresight_horizons({"SHEMS_FORESIGHT_HORIZON": " 48 , 12 "}) == ([48, 12], 1)
    for env, name in (({"SHEMS_FORESIGHT_HORIZON": "a"}, "SHEMS_FORESIGHT_HORIZON"), ({"SHEMS_FORESIGHT_HORIZON": "6,,24"}, "SHEMS_FORESIGHT_HORIZON"),
                      ({"SHEMS_FORESIGHT_HORIZON": ""}, "SHEMS_FORESIGHT_HORIZON"), ({"SHEMS_FORESIGHT_HORIZON": "0"}, "SHEMS_FORESIGHT_HORIZON"),
                      ({"SHEMS_FORESIGHT_HORIZON": "6.5"}, "SHEMS_FORESIGHT_HORIZON"),
                      ({"SHEMS_FORESIGHT_HORIZON": "6", "SHEMS_FORESIGHT_CONTROL": "x"}, "SHEMS_FORESIGHT_CONTROL"),
                      ({"SHEMS_FORESIGHT_HORIZON": "6", "SHEMS_FORESIGHT_CONTROL": "0"}, "SHEMS_FORESIGHT_CONTROL"),
                      ({"SHEMS_FORESIGHT_HORIZON": "6,24", "SHEMS_FORESIGHT_CONTROL": "12"}, "SHEMS_FORESIGHT_CONTROL"),
                      ({"SHEMS_FORESIGHT_CONTROL": "2"}, "SHEMS_FORESIGHT_CONTROL")):
        with pytest.raises(ValueError, match=name):
            M.foresight_horizons(env)
    # main refuses them before it touches the device or the working directory
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_HORIZON": "six"}
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_HORIZON"):
        M.main(env, cwd="/nonexistent-directory", log=lambda *_: None)
    assert os.getcwd() == cwd0

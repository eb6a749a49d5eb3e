"""The foresight controller on a forecast, without a GPU: persistence_forecast row by row, the record layout, the reference side
itself (forecast = truth reproduces the receding-horizon expectation; the forecasts change the planes), a stand-alone host build of
the header swept under the belief against the oracle twin on the composite tables (bit for bit), every refusal of the Python layer
and of the new entry point, file names, the entry script's variable."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import foresight_forecast_ref as FC
import foresight_horizon_ref as FR
import foresight_twin as FT
import util as U


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_persistence_forecast_row_by_row():
    F, T = FT.F(), U.tables_mod()
    tab = T.profile_table(98, "eval")
    for lag, kind in ((6, "lp"), (6, "all"), (3, "ev"), (1, "lp"), (tab.shape[0] - 1, "all")):
        got = F.persistence_forecast(tab, lag, FC.NAMES[kind])
        assert got.dtype == np.float32 and got.shape == tab.shape and got.flags["C_CONTIGUOUS"]
        assert (U.bits32(got) == U.bits32(FC.persistence(tab, lag, FC.COLS[kind]))).all(), (lag, kind)
        other = [k for k in range(8) if k not in FC.COLS[kind]]
        assert (U.bits32(got[:, other]) == U.bits32(tab[:, other])).all() and (U.bits32(got[:lag]) == U.bits32(tab[:lag])).all()
    d = F.persistence_forecast(tab)                                         # lag 24, load and PV
    assert (U.bits32(d) == U.bits32(FC.persistence(tab, 24, (2, 3)))).all() and (d != tab).any()
    assert F.persistence_forecast(tab) is not tab and (tab == T.profile_table(98, "eval")).all()     # the input is left alone
    assert [T.COLUMNS.index(n) for n in FC.NAMES["all"]] == [2, 3, 0, 1] and F.EV_COLUMNS == FC.NAMES["ev"]
    for kw in (dict(lag=0), dict(lag=-3), dict(lag=tab.shape[0]), dict(columns=("electkwh", "pv"))):
        with pytest.raises(ValueError):
            F.persistence_forecast(tab, **kw)
    with pytest.raises(ValueError):
        F.persistence_forecast(tab[:, :7])
    both, index = F.append_forecasts([tab, tab[:50]], 6, FC.NAMES["all"])
    assert len(both) == 4 and index == [2, 3] and both[0] is tab
    assert (U.bits32(both[2]) == U.bits32(FC.persistence(tab, 6, FC.COLS["all"]))).all() and both[3].shape == (50, 8)


def test_record_layout_keeps_its_size_and_names_the_offset():
    F = FT.F()
    P = F.Problem
    assert C.sizeof(P) == 72 and P.forecast_off.offset == 52 and P.forecast_off.size == 4
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("cfg", 0), ("idx0", 48), ("forecast_off", 52), ("scale_b", 56), ("hb", 64)]
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    assert "int32_t forecast_off;" in hdr and "shems_foresight_solve_forecast_dev(" in hdr and "shems_foresight_track_forecast_dev(" in hdr
    assert F.belief_offset(3, 3, 7) == 0 and F.belief_offset(4, 3, 7) == 7 and F.belief_offset(2, 3, -7) == 0 and F.belief_offset(9, 0, -7) == -7


@pytest.mark.parametrize("H, c", [(1, 1), (6, 1), (6, 4), (12, 1), (30, 30)])
def test_reference_with_the_truth_as_forecast_is_the_receding_horizon_expectation(H, c):
    eV, eA = FR.expected("s1", 0, H, c)
    V, A = FC.expected("s1", 0, "truth", H, c)
    assert (U.bits64(V) == U.bits64(eV)).all() and (A == eA).all()


@pytest.mark.parametrize("kind", ["lp", "all"])
def test_reference_under_a_forecast_differs_from_the_truth(kind):
    """The inputs exercise the feature: under the lag-6 forecasts most planes and many arg-max entries of S1 change."""
    for H, c in ((6, 1), (6, 4), (12, 1), (30, 30)):
        eV, eA = FR.expected("s1", 0, H, c)
        V, A = FC.expected("s1", 0, kind, H, c)
        planes = int((U.bits64(V) != U.bits64(eV)).any(axis=1).sum())
        print(f"{kind} (H, c) = ({H}, {c}): {planes} of 31 planes differ, {int((A != eA).sum())} of 1350 arg-max entries, max |dV| {np.abs(V - eV).max():.3f}")
        assert planes >= 20 and (A != eA).sum() >= 100


def _hostcheck(tmp_path):
    exe = str(tmp_path / "foresight_forecast_hostcheck")
    src = os.path.join(U.ROOT, "tests", "hostcheck", "foresight_forecast_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(U.ROOT, "include"), "-o", exe, src])
    return exe


def _run_hostcheck(exe, path, H, c, T, N):
    out = subprocess.run([exe, path, str(H), str(c)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    V, A = np.zeros((T + 1, N), np.uint64), np.full((T, N), -1, np.int32)
    for line in out.stdout.split("\n"):
        w = line.split()
        if w and w[0] == "V":
            V[int(w[1]), int(w[2])] = int(w[3], 16)
        elif w:
            A[int(w[1]), int(w[2])] = int(w[3])
    return V, A


def test_host_build_of_the_header_under_the_belief_equals_the_twin(tmp_path):
    """S1 with the four-column lag-6 forecast: a serial loop over the windows that takes every row where fs_belief_off says, built
    with g++ as a stand-alone program, prints the planes the entry point would leave; they equal the twin on the composite tables bit
    for bit, with the forecast table behind the truth (positive offset) and before it (negative offset)."""
    S, F = U.pkg(), FT.F()
    exe = _hostcheck(tmp_path)
    d = FT.s1()
    sh = FT.S1
    g = F.Grid(sh["nb"], sh["ne"], sh["nab"], sh["nae"])
    T, N, nrow = sh["T"], g.nodes, d["tab"].shape[0]
    fc = FC.forecast("s1", 0, "all")
    for order, row0, off in ((("tab", "fc"), 0, nrow), (("fc", "tab"), nrow, -nrow)):
        rows = np.ascontiguousarray(np.concatenate([d["tab"] if o == "tab" else fc for o in order], 0), np.float32)
        probs = F.make_problems([S.make_config(98, row0, nrow)], d["idx0"], T, g, 2 * nrow)
        probs[0].forecast_off = off
        path = str(tmp_path / f"in_{row0}.bin")
        with open(path, "wb") as f:
            f.write(np.array([2 * nrow, g.nb, g.ne, g.nab, g.nae, T], np.int32).tobytes())
            f.write(bytes(probs[0]))
            f.write(rows.tobytes())
        for H, c in ((6, 1), (6, 4), (30, 30)):
            V, A = _run_hostcheck(exe, path, H, c, T, N)
            eV, eA = FC.expected("s1", 0, "all", H, c)
            assert (V == U.bits64(eV)).all() and (A == eA).all(), (order, H, c)
    # forecast_off = 0: the receding-horizon planes on the truth
    probs[0].forecast_off = 0
    with open(path, "wb") as f:
        f.write(np.array([2 * nrow, g.nb, g.nae * 0 + g.ne, g.nab, g.nae, T], np.int32).tobytes())
        f.write(bytes(probs[0]))
        f.write(rows.tobytes())
    V, A = _run_hostcheck(exe, path, 6, 4, T, N)
    eV, eA = FR.expected("s1", 0, 6, 4)
    assert (V == U.bits64(eV)).all() and (A == eA).all()


def test_solve_horizon_refuses_a_bad_forecast_table_on_the_host():
    S, F = U.pkg(), FT.F()
    tab = U.tables_mod().synthetic_table("eval", 98)
    n = tab.shape[0]
    cfg = S.make_config(98, 0, n)
    g = F.Grid(9, 5, 5, 3)
    fc = F.persistence_forecast(tab, 6)
    for ft, word in (([2], "outside"), ([-1], "outside"), ([1, 1], "entries"), ([], "entries")):
        with pytest.raises(ValueError, match=word):
            F.solve_horizon([tab, fc], [cfg], 1, 5, 3, grid=g, forecast_table=ft)
    with pytest.raises(ValueError, match="rows"):
        F.solve_horizon([tab, fc[:-1]], [cfg], 1, 5, 3, grid=g, forecast_table=[1])
    # what solve_horizon refuses is refused with a forecast too
    for kw, word in ((dict(horizon=0), "horizon"), (dict(horizon=3, control=4), "control")):
        with pytest.raises(ValueError, match=word):
            F.solve_horizon([tab, fc], [cfg], 1, 5, grid=g, forecast_table=[1], **kw)
    with pytest.raises(ValueError, match="160000.*150000"):
        F.solve_horizon([tab, fc], [cfg], 1, 5, 3, grid=F.Grid(100, 100, 3, 3), forecast_table=[1])
    H = importlib.import_module(U.PKG_NAME + ".harness")
    import inspect
    assert inspect.signature(H.inference_foresight).parameters["forecast_table"].default is None
    assert inspect.signature(F.solve_horizon).parameters["forecast_table"].default is None
    # the offsets Python hands down: the table's first row minus the problem's
    probs = F.make_problems([cfg, S.make_config(98, 2 * n, n)], 1, 5, g, 3 * n)
    assert F._forecast_offsets([1, 1], probs, [0, n, 2 * n], [n, n, n]) == [n, -n]
    assert F._forecast_offsets([None, 2], probs, [0, n, 2 * n], [n, n, n]) == [0, 0]


def test_track_refuses_values_solved_on_another_row_array():
    """track reads the ENV's rows: values whose forecast offsets were formed on a row array of another length are a ValueError, raised
    before the library is asked for anything."""
    F = FT.F()

    class Env:
        n, table_row0, table_nrow = 1, np.array([0]), np.array([40])

        def use_torch_stream(self):
            raise AssertionError("refused before the env is touched")

    g = F.Grid(9, 5, 5, 3)
    val = F.Values(g, 5, [None], None, None, None, forecast_off=[40], total_rows=80)
    assert val.forecast_off == [40] and F.Values(g, 5, [None], None, None, None).forecast_off == [0]
    with pytest.raises(ValueError, match="80.*40"):
        F.track(Env(), val)


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """Every SHEMS_ERR_ARG case of shems_foresight_solve_forecast_dev returns before the first HIP call, with a message (host memory
    stands in for the device pointers, which are never dereferenced on these paths)."""
    S, F = U.pkg(), FT.F()
    L = F._declare(S._capi.lib())
    tab = np.zeros((120, 8), np.float32)
    g = F.Grid(9, 5, 5, 3)
    T = 5
    V = np.zeros((T + 1) * 129 * 65)

    def probs_at(row0, off):
        p = F.make_problems([S.make_config(98, row0, 40)], 1, T, g, 120)
        p[0].forecast_off = off
        return p

    def call(probs, grid=None, H=3, c=1, vd=(T + 1) * g.nodes, fn="shems_foresight_solve_forecast_dev"):
        gs = grid if grid is not None else g.struct()
        rc = getattr(L, fn)(_ptr(tab), 120, probs, C.cast(probs, C.c_void_p), 1, C.byref(gs), T, H, c, _ptr(V), vd, None, None)
        return rc, L.shems_last_error().decode()

    # a forecast table running off either end of the array: past the end, before the start through a negative offset, one row each way
    for row0, off, lo, hi in ((40, 41, 81, 121), (40, 80, 120, 160), (40, -41, -1, 39), (0, -1, -1, 39), (80, 1, 81, 121)):
        rc, msg = call(probs_at(row0, off))
        assert rc == S._capi.ERR_ARG and "shems_foresight_solve_forecast_dev" in msg and "problem 0" in msg and "forecast" in msg, msg
        assert f"{lo} .. {hi} of 120" in msg, msg
    # the edges that fit pass this check (asked with a V buffer one float64 short, so that the call still returns before any HIP call)
    for row0, off in ((40, 40), (40, -40), (40, 0), (0, 80), (80, -80)):
        rc, msg = call(probs_at(row0, off), vd=(T + 1) * g.nodes - 1)
        assert rc == S._capi.ERR_ARG and "V buffer" in msg, msg
    good = probs_at(40, 40)
    for kw, word in ((dict(H=0), "horizon"), (dict(H=-2), "horizon"), (dict(c=0), "control"), (dict(H=3, c=4), "control")):
        rc, msg = call(good, **kw)
        assert rc == S._capi.ERR_ARG and word in msg and "shems_foresight_solve_forecast_dev" in msg, msg
    rc, msg = call(good, grid=F.GridStruct(100, 100, 5, 3), vd=(T + 1) * 10000)
    assert rc == S._capi.ERR_ARG and "160000" in msg and "150000" in msg, msg
    rc, msg = call(good, grid=F.GridStruct(129, 65, 5, 3), vd=(T + 1) * 129 * 65 - 1)
    assert rc == S._capi.ERR_ARG and "V buffer" in msg, msg
    # what fs_check_solve refuses for every solve call
    rc, msg = call(good, grid=F.GridStruct(1, 5, 5, 3))
    assert rc == S._capi.ERR_ARG and "state grid" in msg
    off = probs_at(40, 40)
    off[0].idx0 = 36
    rc, msg = call(off)
    assert rc == S._capi.ERR_ARG and "runs off its table" in msg
    # the other window entry point does not read the member: an offset that would leave the array is no refusal there
    rc, msg = call(probs_at(40, 4000), vd=(T + 1) * g.nodes - 1, fn="shems_foresight_solve_horizon_dev")
    assert rc == S._capi.ERR_ARG and "V buffer" in msg, msg
    assert L.shems_abi_version() == 1
    assert {"shems_foresight_solve_forecast_dev", "shems_foresight_track_forecast_dev"} <= set(S._capi.exported_symbols())


def test_file_names_and_tracker_seeds_carry_the_forecast():
    H = importlib.import_module(U.PKG_NAME + ".harness")
    d = os.path.join("out", "tracker")
    base = os.path.join(d, "11709800_eval_results_Charger98_dw0.01_foresight")
    name = lambda **kw: H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=d, **kw)
    assert name() == base + ".csv" and name(horizon=24) == base + "_h24.csv" and name(horizon=24, control=12) == base + "_h24_c12.csv"
    assert name(horizon=24, forecast=None) == base + "_h24.csv"
    assert name(horizon=24, forecast=24) == base + "_h24_p24.csv"
    assert name(horizon=24, forecast=(24, False)) == base + "_h24_p24.csv"
    assert name(horizon=24, control=12, forecast=(6, False)) == base + "_h24_c12_p6.csv"
    assert name(horizon=6, forecast=(24, True)) == base + "_h6_p24ev.csv"
    assert name(horizon=48, control=24, forecast=(24, True)) == base + "_h48_c24_p24ev.csv"
    assert (H.foresight_seed(24, 1, 24), H.foresight_seed(24, 12, (24, True))) == ("foresight_h24_p24", "foresight_h24_c12_p24ev")
    with pytest.raises(ValueError):
        H.foresight_seed(None, 1, 24)


def test_entry_script_reads_the_forecast_and_refuses_malformed_values():
    M = importlib.import_module(U.PKG_NAME + ".main")
    h = {"SHEMS_FORESIGHT_HORIZON": "6,24"}
    assert M.foresight_forecast({}) is None and M.foresight_forecast(h) is None
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "persistence"}) == (24, False)
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "persistence:6"}) == (6, False)
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "persistence:48:ev"}) == (48, True)
    for raw in ("", "naive", "persistence:", "persistence:x", "persistence:0", "persistence:-2", "persistence:6:EV", "persistence:6:ev:1",
                "persistence:ev", "persistence:6.5"):
        with pytest.raises(ValueError, match="SHEMS_FORESIGHT_FORECAST"):
            M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": raw})
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_FORECAST.*SHEMS_FORESIGHT_HORIZON"):
        M.foresight_forecast({"SHEMS_FORESIGHT_FORECAST": "persistence"})
    # main refuses them before it touches the device or the working directory
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_FORECAST": "persistence:6"}
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_FORECAST"):
        M.main(env, cwd="/nonexistent-directory", log=lambda *_: None)
    assert os.getcwd() == cwd0

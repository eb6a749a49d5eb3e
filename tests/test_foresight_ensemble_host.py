"""The foresight controller on a forecast ensemble, without a GPU: analog_scenarios / append_scenarios row by row, the reference side
itself (K = 1 is the forecast controller; the S1 figures; the inputs exercise the feature), a stand-alone host build of the header
(fs_step / fs_q_ens) against the NumPy twin bit for bit, every refusal of the Python layer and of the new entry point, file names, the
entry script's variable."""
import ctypes as C
import importlib
import inspect
import os
import subprocess

import numpy as np
import pytest

import foresight_ensemble_ref as ER
import foresight_forecast_ref as FC
import foresight_twin as FT
import util as U

LP, ALL = FC.NAMES["lp"], FC.NAMES["all"]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_analog_scenarios_and_append_scenarios_row_by_row():
    F, T = FT.F(), U.tables_mod()
    tab = T.profile_table(98, "eval")
    assert F.ANALOG_LAGS == (24, 48, 72, 96, 120, 144, 168) and F.MAX_SCENARIOS == 16
    sig = inspect.signature(F.analog_scenarios).parameters
    assert sig["lags"].default == F.ANALOG_LAGS and sig["columns"].default == ("electkwh", "PV_generation")
    sc = F.analog_scenarios(tab)
    assert len(sc) == 7
    for lag, got in zip(F.ANALOG_LAGS, sc):
        assert got.dtype == np.float32 and got.shape == tab.shape
        assert (U.bits32(got) == U.bits32(FC.persistence(tab, lag, FC.COLS["lp"]))).all(), lag
        assert (U.bits32(got[:lag]) == U.bits32(tab[:lag])).all()           # rows below the lag are the truth's
    for lags, kind in (((3, 6, 9), "all"), ((1,), "ev"), ((9, 3), "lp")):
        sc = F.analog_scenarios(tab, lags, FC.NAMES[kind])
        assert len(sc) == len(lags)
        for lag, got in zip(lags, sc):
            assert (U.bits32(got) == U.bits32(FC.persistence(tab, lag, FC.COLS[kind]))).all(), (lag, kind)
    for kw in (dict(lags=()), dict(lags=(0,)), dict(lags=(3, tab.shape[0])), dict(columns=("pv",))):
        with pytest.raises(ValueError):
            F.analog_scenarios(tab, **kw)
    both, index = F.append_scenarios([tab, tab[:50]], (3, 6, 9), ALL)
    assert len(both) == 8 and index == [[2, 3, 4], [5, 6, 7]] and both[0] is tab
    for k, lag in enumerate((3, 6, 9)):
        assert (U.bits32(both[2 + k]) == U.bits32(FC.persistence(tab, lag, FC.COLS["all"]))).all()
        assert (U.bits32(both[5 + k]) == U.bits32(FC.persistence(tab[:50], lag, FC.COLS["all"]))).all()
    one, index = F.append_scenarios(tab, (2,))
    assert len(one) == 2 and index == [[1]]
    assert "causal" in F.analog_scenarios.__doc__ and "truth" in F.analog_scenarios.__doc__


@pytest.mark.parametrize("H, c", [(6, 1), (6, 4)])
def test_reference_with_one_scenario_is_the_forecast_controller(H, c):
    """K = 1, w = 1.0 on the four-column lag-6 scenario: the planes are foresight_forecast_ref's, and along the run's own trajectory
    the NumPy controller of the forecast tests takes the same 180 choices."""
    TG = importlib.import_module("test_foresight_forecast_gpu")
    d = FT.s1()
    V = ER.planes("s1", 0, (6, "all"), H, c)
    eV = FC.expected("s1", 0, "all", H, c)[0]
    assert (U.bits64(V) == U.bits64(eV)).all()
    assert (U.bits32(ER.scenario("s1", 0, (6, "all"))) == U.bits32(FC.forecast("s1", 0, "all"))).all()
    for j in (0, 7, 29):
        assert (U.bits32(ER.composite("s1", 0, (6, "all"), j)) == U.bits32(FC.composite("s1", 0, "all", j))).all()
    run = ER.controller("s1", 0, [(6, "all")], [1.0], [V], TG._starts(d["prof"]))
    picks, ref, acc = TG._numpy_controller(d, "all", eV, run["picks"], None, "forecast")
    assert run["picks"].shape == (6, 30, 2) and (picks == run["picks"]).all()
    assert (U.bits64(acc) == U.bits64(run["totals"])).all() and (U.bits32(ref.state()) == U.bits32(run["ref"].state())).all()
    # the same scenario twice at (0.5, 0.5): 0.5 v + 0.5 v is exact
    two = ER.controller("s1", 0, [(6, "all")] * 2, [0.5, 0.5], [V, V], TG._starts(d["prof"]))
    assert (two["picks"] == run["picks"]).all() and (U.bits64(two["q"]) == U.bits64(run["q"])).all()


# the returns of the issue's table: truth, lag 3, lag 6, lag 9, ensemble (3, 6, 9) at w = (0.5, 0.25, 0.25), from Soc_b = 0.5 soc_max
S1_RETURNS = {("lp", 6, 1): (-20.54, -21.34, -20.75, -19.53, -20.117559), ("lp", 6, 4): (-22.11, -21.86, -21.13, -20.62, -21.192895),
              ("lp", 12, 1): (-16.00, -16.68, -17.94, -17.11, -17.274939), ("all", 6, 1): (-20.54, -26.21, -54.27, -53.34, -53.833413),
              ("all", 6, 4): (-22.11, -55.08, -54.27, -53.83, -54.332466), ("all", 12, 1): (-16.00, -21.80, -53.33, -53.34, -53.334331)}


@pytest.mark.parametrize("kind, H, c", sorted(S1_RETURNS))
def test_s1_returns_and_the_inputs_exercise_the_feature(kind, H, c):
    """The twin's ensemble return to 1e-6 and the members' to the two decimals they were recorded with; the ensemble's return differs
    from every single member's and its choices differ from each member's in at least one hour.  No order is asserted: the ensemble is
    neither best nor worst of its row."""
    want = S1_RETURNS[kind, H, c]
    specs = ((3, kind), (6, kind), (9, kind))
    ens = ER.s1_run(specs, (0.5, 0.25, 0.25), H, c)
    members = [ER.s1_run((s,), (1.0,), H, c) for s in specs]
    truth = ER.s1_run((ER.TRUTH,), (1.0,), H, c)
    got = [truth["totals"][0]] + [m["totals"][0] for m in members] + [ens["totals"][0]]
    differ = [int((m["picks"] != ens["picks"]).any(axis=2).sum()) for m in members]
    print(f"{kind} (H, c) = ({H}, {c}): returns {[round(float(x), 6) for x in got]}; hours whose choice differs from lag 3 / 6 / 9: {differ}")
    assert abs(got[4] - want[4]) < 1e-6
    for g, w in zip(got[:4], want[:4]):
        assert abs(g - w) < 0.005 + 1e-9
    assert all(U.bits64(m["totals"])[0] != U.bits64(ens["totals"])[0] for m in members)
    assert min(differ) >= 1


def _hostcheck(tmp_path):
    exe = str(tmp_path / "foresight_ensemble_hostcheck")
    src = os.path.join(U.ROOT, "tests", "hostcheck", "foresight_ensemble_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(U.ROOT, "include"), "-o", exe, src])
    return exe


def test_host_build_of_the_header_gives_the_bits_of_the_twin(tmp_path):
    """S1, scenarios lag 3, 6, 9 of all four columns, w = (0.5, 0.25, 0.25), (H, c) = (6, 1) and (6, 4): fs_step + fs_q_ens, built
    with g++ as a stand-alone program, on the planes the twin wrote to a file, along the twin's trajectory: Qbar of all 15 actions at
    all 30 hours, bit for bit.  The scenario tables lie behind the truth; a second layout puts one of them BEFORE it."""
    S, F = U.pkg(), FT.F()
    exe = _hostcheck(tmp_path)
    d = FT.s1()
    sh = FT.S1
    g = F.Grid(sh["nb"], sh["ne"], sh["nab"], sh["nae"])
    T, nrow = sh["T"], d["tab"].shape[0]
    specs, w = ((3, "all"), (6, "all"), (9, "all")), (0.5, 0.25, 0.25)
    sc = [ER.scenario("s1", 0, s) for s in specs]
    for H, c in ((6, 1), (6, 4)):
        run = ER.s1_run(specs, w, H, c)
        V = np.stack([ER.planes("s1", 0, s, H, c) for s in specs])
        for order, row0, offs in (([d["tab"]] + sc, 0, (nrow, 2 * nrow, 3 * nrow)), ([sc[1], d["tab"], sc[0], sc[2]], nrow, (nrow, -nrow, 2 * nrow))):
            rows = np.ascontiguousarray(np.concatenate(order, 0), np.float32)
            probs = F.make_problems([S.make_config(98, row0, nrow)] * 3, d["idx0"], T, g, 4 * nrow)
            for k in range(3):
                probs[k].forecast_off = offs[k]
            path = str(tmp_path / f"in_{H}_{c}_{row0}.bin")
            with open(path, "wb") as f:
                f.write(np.array([4 * nrow, g.nb, g.ne, g.nab, g.nae, T, 3], np.int32).tobytes())
                f.write(bytes(probs))
                f.write(np.array(w, np.float64).tobytes())
                f.write(rows.tobytes())
                f.write(np.ascontiguousarray(V, np.float64).tobytes())
                f.write(np.ascontiguousarray(run["obs"][0], np.float32).tobytes())
            out = subprocess.run([exe, path], capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            got = np.zeros((T, g.actions), np.uint64)
            seen = 0
            for line in out.stdout.split("\n"):
                x = line.split()
                if x:
                    got[int(x[0]), int(x[1])] = int(x[2], 16)
                    seen += 1
            assert seen == T * g.actions
            same = got == U.bits64(run["q"][0])
            print(f"(H, c) = ({H}, {c}), truth at row {row0}: {int(same.sum())} of {same.size} Qbar equal to the twin's bits")
            assert same.all(), np.argwhere(~same)[:10]


def test_solve_ensemble_refuses_on_the_host_before_any_device_work():
    S, F = U.pkg(), FT.F()
    tab = U.tables_mod().synthetic_table("eval", 98)
    n = tab.shape[0]
    cfg = S.make_config(98, 0, n)
    g = F.Grid(9, 5, 5, 3)
    both, index = F.append_scenarios([tab], (3, 6, 9))
    call = lambda tabs=both, cfgs=(cfg,), **kw: F.solve_ensemble(tabs, list(cfgs), 1, 5, kw.pop("horizon", 3), grid=g, **kw)
    two = F.append_scenarios([tab, tab], (3, 6))
    cfg2 = [S.make_config(98, 0, n), S.make_config(98, n, n)]
    for kw, word in ((dict(scenarios=[[1, 2], [3]], tabs=two[0], cfgs=cfg2), "ragged"), (dict(scenarios=[[]]), "1 .. 16"),
                     (dict(scenarios=[[1] * 17]), "1 .. 16"), (dict(scenarios=None), "scenarios"), (dict(scenarios=[[1], [2]]), "2 lists for 1"),
                     (dict(scenarios=index, weights=[0.5, 0.5]), "weights"), (dict(scenarios=index, weights=[[0.5, 0.25, 0.25]] * 2), "weights"),
                     (dict(scenarios=index, weights=[0.5, 0.0, 0.5]), "scenario 1.*weight"), (dict(scenarios=index, weights=[0.5, 0.5, -1.0]), "scenario 2.*weight"),
                     (dict(scenarios=index, weights=[np.nan, 0.5, 0.5]), "scenario 0.*weight"), (dict(scenarios=index, weights=[0.5, np.inf, 0.5]), "scenario 1.*weight"),
                     (dict(scenarios=[[1, 2, 4]]), "scenario 2.*outside"), (dict(scenarios=[[-1, 2, 3]]), "scenario 0.*outside"),
                     (dict(scenarios=[[1, 2]], tabs=[tab, both[1], both[2][:-1]]), "scenario 1.*rows"),
                     (dict(scenarios=index, horizon=None), "horizon"), (dict(scenarios=index, horizon=0), "horizon"),
                     (dict(scenarios=index, horizon=3, control=4), "control")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    # the weights handed down: normalised per problem, equal by default
    assert (F.ensemble_weights(None, 2, 4) == 0.25).all() and F.ensemble_weights(None, 2, 4).shape == (2, 4)
    assert (U.bits64(F.ensemble_weights([2.0, 1.0, 1.0], 2, 3)) == U.bits64(np.array([[0.5, 0.25, 0.25]] * 2))).all()
    assert (U.bits64(F.ensemble_weights([[3, 1], [1, 3]], 2, 2)) == U.bits64(np.array([[0.75, 0.25], [0.25, 0.75]]))).all()
    assert (F.ensemble_weights([1.0] * 16, 1, 16) == 1.0 / 16).all()
    sig = inspect.signature(F.solve_ensemble).parameters
    assert sig["control"].default == 1 and sig["weights"].default is None and sig["grid"].default is None


def test_track_and_audit_refuse_ensemble_values_they_cannot_take():
    F = FT.F()
    H = importlib.import_module(U.PKG_NAME + ".harness")

    class Env:
        n, table_row0, table_nrow = 1, np.array([0]), np.array([40])

        def use_torch_stream(self):
            raise AssertionError("refused before the env is touched")

        reset_ = use_torch_stream

    g = F.Grid(9, 5, 5, 3)
    inner = F.Values(g, 5, [None, None], None, None, None, forecast_off=[40, 80], total_rows=120)
    ens = F.EnsembleValues(inner, 2, [[0.5, 0.5]])
    assert (ens.n_scen, ens.n_problems, ens.nsteps, ens.total_rows) == (2, 1, 5, 120) and ens.weights.dtype == np.float64
    with pytest.raises(ValueError, match="120.*40"):
        F.track(Env(), ens)
    with pytest.raises(ValueError, match="ensemble"):
        F.audit(ens, np.zeros((5, 23)))
    sig = inspect.signature(H.inference_foresight).parameters
    assert sig["scenario_tables"].default is None and sig["weights"].default is None
    assert list(sig)[:6] == ["env", "grid", "horizon", "control", "forecast_table", "values"]


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """Every SHEMS_ERR_ARG case of shems_foresight_track_ensemble_dev returns before the first HIP call, with a message (host memory
    stands in for the device pointers, which are never dereferenced on these paths)."""
    S, F = U.pkg(), FT.F()
    L = F._declare(S._capi.lib())
    g = F.Grid(9, 5, 5, 3)
    T, P, K = 5, 2, 3
    buf = np.zeros(4096)
    good_w = np.full((P, K), 1.0 / 3)
    name = "shems_foresight_track_ensemble_dev"

    def view(**kw):
        v = S._capi.View(n_envs=4, maxsteps=T, n_cfg=1, obs=buf.ctypes.data, idx=buf.ctypes.data, step=buf.ctypes.data, cfg_of_env=None,
                         cfgs=buf.ctypes.data, tables=buf.ctypes.data, total_rows=120, err=buf.ctypes.data)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def call(v=None, prob=True, n_prob=P, K=K, w=good_w, dw=True, grid=None, T=T, V=True, vd=None, results_env=-1):
        gs = grid if grid is not None else g.struct()
        v = view() if v is None else v
        vd = n_prob * K * (T + 1) * gs.nb * gs.ne if vd is None else vd
        rc = L.shems_foresight_track_ensemble_dev(C.byref(v), _ptr(buf) if prob else None, n_prob, K, None if w is None else _ptr(w), _ptr(buf) if dw else None,
                                                  None, C.byref(gs), T, _ptr(buf) if V else None, vd, None, results_env, None, None, None)
        return rc, L.shems_last_error().decode()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == S._capi.ERR_ARG and name in msg and word in msg, (kw, msg)

    # everything track_forecast_dev refuses
    refused("shems_view", v=view(n_envs=0))
    refused("shems_view", v=view(obs=None))
    refused("cfg_of_env", v=view(n_cfg=2))
    refused("state grid", grid=F.GridStruct(1, 5, 5, 3))
    refused("action grid", grid=F.GridStruct(9, 5, 0, 3))
    refused("LDS", grid=F.GridStruct(200, 100, 5, 3))
    refused("T = 0", T=0)
    refused("NULL buffer or no problem", prob=False)
    refused("NULL buffer or no problem", n_prob=0)
    refused("NULL buffer or no problem", V=False)
    refused("results_env 4", results_env=4)
    # the ensemble's own
    for k in (0, -1, 17):
        refused(f"n_scen = {k}", K=k, w=np.ones((P, 17)), vd=10 ** 9)
    refused("NULL weight", w=None)
    refused("NULL weight", dw=False)
    for bad in (0.0, -0.25, np.nan, np.inf, -np.inf):
        w = good_w.copy()
        w[1, 2] = bad
        refused("problem 1, scenario 2", w=w)
    w = good_w.copy()
    w[0, 0] = 0.0
    refused("problem 0, scenario 0", w=w)
    need = P * K * (T + 1) * g.nodes
    refused(f"need {need}", vd=need - 1)
    refused("V buffer", vd=P * (T + 1) * g.nodes)                            # what track_forecast_dev would ask for is not enough
    # 1 and 16 scenarios pass the count check (asked with a V buffer one float64 short, so that the call still returns before any HIP call)
    for k in (1, 16):
        refused("V buffer", K=k, w=np.ones((P, 16)), vd=P * k * (T + 1) * g.nodes - 1)
    assert L.shems_abi_version() == 1


def test_header_names_the_entry_point_and_the_definition():
    S = U.pkg()
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    assert "shems_foresight_track_ensemble_dev(" in hdr
    comment = hdr.split("shems_foresight_track_ensemble_dev(")[0].rsplit("*/", 2)[1]       # the comment right above the prototype
    assert "LU1:283-316, 343-485" in comment and "LU1:264-281" in comment and "n_scen" in comment
    assert "shems_foresight_track_ensemble_dev" in S._capi.exported_symbols()
    core = open(os.path.join(os.path.dirname(S.__file__), "csrc", "shems_foresight_core.h")).read()
    after_audit = core.split("fs_audit_v_state")[-1]
    assert "fs_step(" in after_audit and "fs_q_ens(" in after_audit and "optimistic" in after_audit.lower()
    assert core.count("SHEMS_HD double fs_q(") == 1


def test_file_names_and_tracker_seeds_carry_the_ensemble():
    H = importlib.import_module(U.PKG_NAME + ".harness")
    d = os.path.join("out", "tracker")
    base = os.path.join(d, "11709800_eval_results_Charger98_dw0.01_foresight")
    name = lambda **kw: H.foresight_file_name(11709800, "eval", "Charger98_dw0.01", out_dir=d, **kw)
    assert name(horizon=24, forecast=("analog", (24, 48, 72), False)) == base + "_h24_a24-48-72.csv"
    assert name(horizon=24, forecast=("analog", [24, 48, 72], True)) == base + "_h24_a24-48-72ev.csv"
    assert name(horizon=48, control=24, forecast=("analog", (24,), False)) == base + "_h48_c24_a24.csv"
    assert H.foresight_seed(6, 1, ("analog", (3, 6), False)) == "foresight_h6_a3-6"
    assert H.foresight_seed(6, 2, ("analog", (3, 6), True)) == "foresight_h6_c2_a3-6ev"
    # what was there stays
    assert name() == base + ".csv" and name(horizon=24) == base + "_h24.csv" and name(horizon=24, forecast=(24, True)) == base + "_h24_p24ev.csv"
    assert name(horizon=24, forecast=24) == base + "_h24_p24.csv"
    for kw in (dict(horizon=None, forecast=("analog", (24,), False)), dict(horizon=24, forecast=("analog", (), False))):
        with pytest.raises(ValueError):
            H.foresight_seed(kw["horizon"], 1, kw["forecast"])


def test_entry_script_reads_the_ensemble_and_refuses_malformed_values():
    M = importlib.import_module(U.PKG_NAME + ".main")
    h = {"SHEMS_FORESIGHT_HORIZON": "6,24"}
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "analog:24,48,72"}) == ("analog", (24, 48, 72), False)
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "analog:3,6:ev"}) == ("analog", (3, 6), True)
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "analog:24"}) == ("analog", (24,), False)
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "analog:" + ",".join(str(k) for k in range(1, 17))})[1] == tuple(range(1, 17))
    assert M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": "persistence:48:ev"}) == (48, True) and M.foresight_forecast(h) is None
    for raw in ("analog", "analog:", "analog:x", "analog:24,", "analog:0,24", "analog:-3", "analog:24:EV", "analog:24:ev:1", "analog:ev",
                "analog:2.5", "analog:" + ",".join(["24"] * 17), "analogue:24"):
        with pytest.raises(ValueError, match="SHEMS_FORESIGHT_FORECAST"):
            M.foresight_forecast({**h, "SHEMS_FORESIGHT_FORECAST": raw})
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_FORECAST.*SHEMS_FORESIGHT_HORIZON"):
        M.foresight_forecast({"SHEMS_FORESIGHT_FORECAST": "analog:24,48"})
    # main refuses them before it touches the device or the working directory
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_FORECAST": "analog:3,6"}
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_FORECAST"):
        M.main(env, cwd="/nonexistent-directory", log=lambda *_: None)
    assert os.getcwd() == cwd0

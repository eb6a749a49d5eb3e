"""Transitions and returns-to-go from tracked passes, without a GPU: a stand-alone host build of the header's definition against the
NumPy twin on S1's three trajectories (bit for bit, both modes, a wrapping ring), the recurrence against a plain Python loop, refused
hours and refused passes, every refusal of the entry point and of the Python layer, and the entry script's switch."""
import ctypes as C
import importlib
import os
import subprocess
import types

import numpy as np
import pytest

import foresight_regret_ref as RR
import foresight_twin as FT
import util as U
import warmstart_ref as WR

GAMMA = 0.99


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _hostcheck(tmp_path):
    exe = str(tmp_path / "warmstart_hostcheck")
    src = os.path.join(U.ROOT, "tests", "hostcheck", "warmstart_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(U.ROOT, "include"), "-o", exe, src])
    return exe


def _run(exe, tmp_path, results, mode, tail, capacity, pos, gamma=GAMMA):
    """Writes the input, runs the host build on S1's problem and returns (process, dict shaped like the twin's, with uint32 / uint64
    bit patterns in s, a, r, s2 and G)."""
    S, F = U.pkg(), FT.F()
    d, sh = FT.s1(), FT.S1
    res = np.ascontiguousarray(results, np.float64)
    n, T, _ = res.shape
    nrow = d["tab"].shape[0]
    probs = F.make_problems([S.make_config(98, 0, nrow)], d["idx0"], T, F.Grid(sh["nb"], sh["ne"], sh["nab"], sh["nae"]), nrow)
    path = str(tmp_path / "in.bin")
    with open(path, "wb") as f:
        f.write(np.array([nrow, T, n, mode, tail, 0], np.int32).tobytes())
        f.write(np.array([gamma, 0], np.float32).tobytes())
        f.write(np.array([capacity, pos], np.int64).tobytes())
        f.write(bytes(probs[0]))
        f.write(np.ascontiguousarray(d["tab"], np.float32).tobytes())
        f.write(res.tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True)
    keep = T - tail
    got = dict(slot=np.full((n, keep), -7, np.int64), s=np.zeros((n, keep, 9), np.uint32), s2=np.zeros((n, keep, 9), np.uint32),
               a=np.zeros((n, keep, 2), np.uint32), r=np.zeros((n, keep), np.uint32), done=np.zeros((n, keep), np.uint8),
               status=np.full(n, 99, np.int32), G=np.zeros((n, T), np.uint64))
    if out.returncode == 0:
        for line in out.stdout.split("\n"):
            w = line.split()
            if not w:
                continue
            if w[0] == "G":
                got["G"][int(w[1])] = [int(x, 16) for x in w[2:]]
            elif w[0] == "status":
                got["status"][int(w[1])] = int(w[2])
            else:
                e, t = int(w[0]), int(w[1])
                got["slot"][e, t] = int(w[2])
                if got["slot"][e, t] >= 0:
                    v = [int(x, 16) for x in w[3:24]]
                    got["s"][e, t], got["a"][e, t], got["r"][e, t], got["s2"][e, t], got["done"][e, t] = v[:9], v[9:11], v[11], v[12:], int(w[24])
    return out, got


def _twin(res, mode, tail, capacity, pos, gamma=GAMMA):
    d = FT.s1()
    n = len(res)
    return WR.twin_transitions(res, [d["tab"]] * n, [d["idx0"]] * n, mode, gamma, tail, pos=pos, capacity=capacity)


def _same(got, tw):
    ok = tw["slot"] >= 0
    return ((got["slot"] == tw["slot"]).all() and (got["status"] == tw["status"]).all() and (got["G"] == U.bits64(tw["G"])).all() and
            all((got[k][ok] == U.bits32(tw[k])[ok]).all() for k in ("s", "a", "r", "s2")) and (got["done"][ok] == tw["done"][ok]).all())


@pytest.mark.parametrize("mode,tail,count", [(WR.TD, 1, 87), (WR.MC, 5, 75)])
def test_host_build_of_the_definition_equals_the_twin_on_s1(tmp_path, mode, tail, count):
    """S1's rule-based, greedy and random passes (the rule-based rows are used mechanically) into a ring of 128 slots from slot 100:
    slots, all five arrays, G as float64 bits and status of a g++ build of the header equal the twin."""
    exe = _hostcheck(tmp_path)
    res, _ = RR.s1_passes()
    out, got = _run(exe, tmp_path, res, mode, tail, 128, 100)
    assert out.returncode == 0, out.stderr
    tw = _twin(res, mode, tail, 128, 100)
    assert (tw["status"] == 0).all() and (tw["slot"] >= 0).all() and tw["slot"].size == count
    assert _same(got, tw)
    assert tw["slot"][0, 0] == 100 and len(np.unique(tw["slot"])) == count and tw["slot"].min() == 0       # wraps, no slot twice
    assert (tw["done"] == (1 if mode == WR.MC else 0)).all()
    # s2 of hour t is s of hour t + 1, and the greedy pass's actions are labels of the action grid it chose from
    assert (U.bits32(tw["s2"][:, :-1]) == U.bits32(tw["s"][:, 1:])).all()
    lab = WR.IR.label(FT.action_grid(FT.S1["nab"], FT.S1["nae"]))
    assert all((lab == x).all(1).any() for x in tw["a"][1])
    if mode == WR.TD:
        assert (U.bits32(tw["r"]) == U.bits32(res[:, :29, 5].astype(np.float32))).all()
    else:
        assert (U.bits32(tw["r"]) == U.bits32(tw["G"][:, :25].astype(np.float32))).all()


def test_returns_equal_a_plain_loop_in_the_same_order():
    res, _ = RR.s1_passes()
    g = float(np.float32(GAMMA))
    for e in range(3):
        r = [float(x) for x in res[e, :, 5]]
        G = [0.0] * len(r)
        G[-1] = r[-1]
        for t in range(len(r) - 2, -1, -1):
            G[t] = r[t] + g * G[t + 1]
        assert (U.bits64(WR.returns(res[e, :, 5], GAMMA)) == U.bits64(np.array(G))).all()
    # the order matters: summing forwards with powers of gamma is a different number somewhere
    fwd = np.array([sum(g ** (u - t) * res[0, u, 5] for u in range(t, 30)) for t in range(30)])
    assert np.abs(fwd - WR.returns(res[0, :, 5], GAMMA)).max() < 1e-9 and (U.bits64(fwd) != U.bits64(WR.returns(res[0, :, 5], GAMMA))).any()
    assert (WR.returns([1.0, 2.0, 4.0], 0.0) == [1.0, 2.0, 4.0]).all() and (WR.returns([1.0, 2.0, 4.0], 1.0) == [7.0, 6.0, 4.0]).all()


def test_td_a_corrupted_row_refuses_two_hours_and_a_nan_reward_one(tmp_path):
    S = U.pkg()
    exe = _hostcheck(tmp_path)
    res, _ = RR.s1_passes()
    bad = res.copy()
    bad[1, 7, 0] += 1                                                       # a shifted row index: hours 6 (its successor) and 7
    bad[2, 12, 5] = np.nan                                                  # a reward that is not finite: hour 12 alone
    out, got = _run(exe, tmp_path, bad, WR.TD, 1, 128, 100)
    assert out.returncode == 0, out.stderr
    tw = _twin(bad, WR.TD, 1, 128, 100)
    assert _same(got, tw)
    assert (np.argwhere(got["slot"] < 0) == [[1, 6], [1, 7], [2, 12]]).all()
    assert (got["status"] == [0, S._capi.ERR_INDEX, S._capi.ERR_INDEX]).all()
    ring = WR.fill(tw, 128, WR.sentinel_arrays(128, 0xA5))
    for e, t in ((1, 6), (1, 7), (2, 12)):                                  # the slot the hour would have taken keeps its sentinel
        k = (100 + e * 29 + t) % 128
        assert all((ring[key][k:k + 1].view(np.uint8) == 0xA5).all() for key in ring)
    assert (ring["done"] == 0).sum() == 84
    # the last row of a pass is a successor only: corrupting it refuses hour T - 2
    bad = res.copy()
    bad[0, 29, 0] = np.nan
    out, got = _run(exe, tmp_path, bad, WR.TD, 1, 128, 100)
    assert (np.argwhere(got["slot"] < 0) == [[0, 28]]).all() and _same(got, _twin(bad, WR.TD, 1, 128, 100))


def test_mc_either_refuses_the_whole_pass_and_the_others_are_written(tmp_path):
    S = U.pkg()
    exe = _hostcheck(tmp_path)
    res, _ = RR.s1_passes()
    for e, t, c, v in ((1, 7, 0, res[1, 7, 0] + 1), (2, 12, 5, np.inf), (0, 29, 5, np.nan), (0, 28, 0, np.nan)):
        bad = res.copy()
        bad[e, t, c] = v
        out, got = _run(exe, tmp_path, bad, WR.MC, 5, 128, 100)
        assert out.returncode == 0, out.stderr
        tw = _twin(bad, WR.MC, 5, 128, 100)
        assert _same(got, tw)
        want = np.zeros(3, np.int32)
        want[e] = S._capi.ERR_INDEX
        assert (got["status"] == want).all() and (got["slot"][e] == -1).all() and (np.delete(got["slot"], e, 0) >= 0).all()
        assert np.isnan(tw["G"][e]).all() and np.isfinite(np.delete(tw["G"], e, 0)).all()
        ring = WR.fill(tw, 128, WR.sentinel_arrays(128, 0xA5))
        assert (ring["done"] == 1).sum() == 50


def test_host_build_refuses_what_the_ring_cannot_hold(tmp_path):
    exe = _hostcheck(tmp_path)
    res, _ = RR.s1_passes()
    for cap, pos, word in ((86, 0, "ring 2"), (87, 87, "ring 3"), (87, -1, "ring 3"), (0, 0, "ring 1")):
        out, _ = _run(exe, tmp_path, res, WR.TD, 1, cap, pos)
        assert out.returncode == 3 and out.stdout.strip() == word, (cap, pos, out.stdout)
    out, got = _run(exe, tmp_path, res, WR.TD, 1, 87, 86)
    assert out.returncode == 0 and got["slot"][0, 0] == 86 and got["slot"][0, 1] == 0


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """Every SHEMS_ERR_ARG case of shems_foresight_transitions_dev returns before the first HIP call, with a message (host memory
    stands in for the device pointers, which are never dereferenced on these paths)."""
    S, F = U.pkg(), FT.F()
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    L = I._declare(S._capi.lib())
    T, n, cap = 5, 2, 16
    tab = np.zeros((40, 8), np.float32)
    probs = F.make_problems([S.make_config(98, 0, 40)], 1, T, F.Grid(9, 5, 5, 3), 40)
    res, ret, status = np.zeros((n, T, 23)), np.zeros((n, T)), np.zeros(n, np.int32)
    arr = dict(s=np.zeros((cap, 9), np.float32), a=np.zeros((cap, 2), np.float32), r=np.zeros(cap, np.float32),
               s2=np.zeros((cap, 9), np.float32), done=np.zeros(cap, np.uint8))

    def ring(capacity=cap, without=None):
        return S._capi.Replay(capacity, *(arr[k].ctypes.data if k != without else None for k in ("s", "a", "r", "s2", "done")))

    def call(**kw):
        a = dict(tables=_ptr(tab), total_rows=40, prob=C.cast(probs, C.c_void_p), n_prob=1, T=T, res=_ptr(res), n=n, po=None, mode=0,
                 gamma=0.99, tail=1, ret=_ptr(ret), ring=ring(), pos=0, status=_ptr(status))
        a.update(kw)
        rg = a["ring"]
        rc = L.shems_foresight_transitions_dev(a["tables"], a["total_rows"], a["prob"], a["n_prob"], a["T"], a["res"], a["n"], a["po"],
                                               a["mode"], a["gamma"], a["tail"], a["ret"], C.byref(rg) if rg is not None else None,
                                               a["pos"], a["status"], None)
        return rc, L.shems_last_error().decode()

    cases = [(dict(T=1), "T = 1"), (dict(T=0), "T = 0"), (dict(tail=0), "tail = 0"), (dict(tail=T), f"tail = {T}"), (dict(tail=-2), "tail = -2"),
             (dict(mode=2), "mode = 2"), (dict(mode=-1), "mode = -1"), (dict(mode=1, ret=None), "MC mode needs d_returns"),
             (dict(gamma=-0.5), "gamma"), (dict(gamma=1.5), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(gamma=float("inf")), "gamma"),
             (dict(tables=None), "NULL"), (dict(total_rows=1), "2 table rows"), (dict(prob=None), "NULL"), (dict(n_prob=0), "no problem"),
             (dict(n=0), "n_pass = 0"), (dict(n=-1), "n_pass = -1"), (dict(n=65536), "n_pass = 65536"),
             (dict(res=None), "NULL"), (dict(status=None), "NULL"), (dict(ring=None), "NULL ring")] + \
            [(dict(ring=ring(without=k)), "without all of") for k in arr] + \
            [(dict(ring=ring(capacity=0)), "capacity is 0"), (dict(ring=ring(capacity=7)), "8 transitions"), (dict(n=5), "20 transitions"),
             (dict(tail=3, n=9), "18 transitions"), (dict(pos=-1), "pos = -1"), (dict(pos=cap), f"pos = {cap}")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == S._capi.ERR_ARG and "shems_foresight_transitions_dev" in msg and word in msg, (kw, msg)
    assert (status == 0).all() and not any(v.any() for v in arr.values()) and not ret.any()
    assert {"shems_foresight_transitions_dev", "shems_ddpg_critic_update"} <= set(S._capi.exported_symbols())


def test_python_layer_refuses_before_the_library_is_asked(monkeypatch):
    S, F = U.pkg(), FT.F()
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    M = importlib.import_module(U.PKG_NAME + ".main")

    def no_lib():
        raise AssertionError("refused before the library is loaded")

    monkeypatch.setattr(S._capi, "lib", no_lib)
    val = F.Values(F.Grid(9, 5, 5, 3), 5, [None], None, None, None, total_rows=40)
    with pytest.raises(ValueError, match="neither 'td' nor 'mc'"):
        I.transitions(val, np.zeros((2, 5, 23)), None, mode="sarsa")
    with pytest.raises(ValueError, match=r"\[n\]\[5\]\[23\]"):
        I.transitions(val, np.zeros((2, 6, 23)), None)
    with pytest.raises(ValueError, match="at least one"):
        I.warm_start(None, None, val, None, None, 2, 3, 0)
    with pytest.raises(ValueError, match="neither 'td' nor 'mc'"):
        I.warm_start(None, None, val, None, None, 2, 3, 5, mode="x")
    assert I.default_tail("td", 0.99, 30) == 1 and I.default_tail("mc", 0.99, 30) == 29 and I.default_tail("mc", 0.99, 2998) == 459
    assert I.default_tail("mc", 0.5, 30) == 7 and I.default_tail("mc", 0.0, 30) == 1 and I.default_tail("mc", 1.0, 30) == 29
    assert 0.99 ** 459 <= 0.01 < 0.99 ** 458
    # evaluate refuses what clone refuses, before it touches a buffer
    ns = lambda **kw: types.SimpleNamespace(**dict(dict(wide=False, hidden=(250, 500), batch=120, MAX_PASS_BATCH=128,
                                                        sync=types.SimpleNamespace(world=1), _before_param_write=None), **kw))
    for agent, word in ((ns(wide=True, hidden=(300, 600)), "300"), (ns(hidden=(300, 600)), "300"), (ns(batch=129), "129"),
                        (ns(sync=types.SimpleNamespace(world=2)), "replicas"), (ns(_before_param_write=lambda: None), "learner group")):
        with pytest.raises(NotImplementedError, match="evaluate.*" + word):
            D.Agent.evaluate(agent, None)
    # the entry script's switch
    on = {"SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_IMITATE": "2x3"}
    assert M.foresight_warmstart({}) is None and M.foresight_warmstart(on) is None
    assert M.foresight_warmstart(dict(on, SHEMS_FORESIGHT_WARMSTART="50")) == (50, "mc")
    assert M.foresight_warmstart(dict(on, SHEMS_FORESIGHT_WARMSTART="7:td")) == (7, "td")
    assert M.foresight_warmstart(dict(on, SHEMS_FORESIGHT_WARMSTART="7:MC")) == (7, "mc")
    for raw in ("", "x", "5:", "5:sarsa", "5:td:mc", "0", "-3:td", "2.5", ":td"):
        with pytest.raises(ValueError, match="SHEMS_FORESIGHT_WARMSTART"):
            M.foresight_warmstart(dict(on, SHEMS_FORESIGHT_WARMSTART=raw))
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_WARMSTART.*SHEMS_FORESIGHT_IMITATE"):
        M.foresight_warmstart({"SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_WARMSTART": "5"})
    assert M.warmstart_file_name(7, "eval", "Charger98_x") == os.path.join("out/tracker", "7_eval_results_Charger98_x_warmstart.csv")
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_WARMSTART"):
        M.main({"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_WARMSTART": "5"},
               cwd="/nonexistent-directory", log=lambda *_: None)
    assert os.getcwd() == cwd0

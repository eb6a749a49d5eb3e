"""Multi-step (n-step) returns without a GPU: the NumPy twin (tests/nstep_ref.py) against a host build of csrc/shems_nstep_core.h bit
for bit on every case the GPU test runs, the return's accuracy, the host-side discount, the slab layouts, the C struct, the exports,
the refusals and the entry-script switch."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

import nstep_cases as NC
import nstep_ref as NR
import util as U

f32, f64 = np.float32, np.float64


def _hostcheck(tmp_path, sanitize=False):
    exe = str(tmp_path / ("nstep_hostcheck_san" if sanitize else "nstep_hostcheck"))
    src = os.path.join(U.ROOT, "tests", "hostcheck", "nstep_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] +
                          (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + ["-o", exe, src])
    return exe


def _run(exe, tmp_path, mode, case, blocks):
    path = str(tmp_path / "nstep_in.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<7qf", mode, case["n"], case["T"], case["episodes"], case.get("window", 1), case["capacity"], case["pos0"],
                            float(case["gamma"])))
        for b in blocks:
            for k in ("s", "a", "r", "s2", "done"):
                f.write(np.ascontiguousarray(b[k]).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = {}
    for line in out.stdout.strip().split("\n"):
        k, *w = line.split()
        rows[k] = w
    cap = case["capacity"]
    word = lambda k, shape: np.array([int(x, 16) for x in rows[k]], np.uint64).astype(np.uint32).view(f32).reshape(shape)
    ring = dict(s=word("s", (cap, 9)), a=word("a", (cap, 2)), r=word("r", (cap,)), s2=word("s2", (cap, 9)),
                done=np.array([int(x, 16) for x in rows["done"]], np.uint8))
    return ring, int(rows["pushed"][0]), int(rows["gamma_n"][0], 16)


def _check_all(exe, tmp_path, fold_names=None, bulk_names=None):
    seen = 0
    for name, case in NC.fold_cases():
        if fold_names is not None and name not in fold_names:
            continue
        stages = NC.staging(case)
        ring, pushed, gn = _run(exe, tmp_path, 0, case, stages)
        want, want_pushed = NC.fold_twin(case, stages)
        assert NC.ring_bytes(ring) == NC.ring_bytes(want) and pushed == want_pushed, name
        assert gn == U.bits32(np.array([NR.nstep_gamma(case["gamma"], case["n"])]))[0], name
        assert pushed - case["pos0"] == case["episodes"] * (case["T"] - case["n"] + 1) * case["window"], name
        seen += 1
    for name, case in NC.bulk_cases():
        if bulk_names is not None and name not in bulk_names:
            continue
        src = NC.bulk_source(case)
        ring, pushed, _ = _run(exe, tmp_path, 1, case, [src])
        want, want_pushed = NC.bulk_twin(case, src)
        assert NC.ring_bytes(ring) == NC.ring_bytes(want) and pushed == want_pushed, name
        seen += 1
    return seen


def test_core_header_on_the_host_equals_the_twin_bit_for_bit(tmp_path):
    """tests/hostcheck/nstep_hostcheck.cpp, g++ -ffp-contract=off, on EVERY case the GPU test runs.  The cases' coverage is asserted
    first: every n and window of the issue, a push that wraps mid-window, T = n, untouched slots, the bulk skip rule."""
    cases = dict(NC.fold_cases())
    assert {c["n"] for c in cases.values()} == {1, 2, 3, 5, 16} and {c["window"] for c in cases.values()} == {1, 33, 64}
    assert all(c["capacity"] == 100 and c["pos0"] == 90 and c["episodes"] == 2 for c in cases.values())
    assert 90 + 33 > 100                                                        # window 33 from position 90 wraps mid-window
    assert {n for n in (1, 2, 3, 5, 16) if any(c["n"] == n and c["T"] == n for c in cases.values())} == {1, 2, 3, 5, 16}
    ring, _ = NC.fold_twin(cases["n5-w33-T5"], NC.staging(cases["n5-w33-T5"]))
    assert (ring["r"] == NR.SENT_F).sum() == 100 - 66 and (ring["done"] == NR.SENT_B).sum() >= 100 - 66      # untouched slots keep the sentinel
    bulk = dict(NC.bulk_cases())
    assert {c["n"] for c in bulk.values()} == {1, 3, 6} and {c["skips"] for c in bulk.values() if c["n"] == 6} == {False, True}
    assert all({c["skips"] for c in bulk.values() if c["n"] == n} == {False, True} for n in (1, 3, 6))
    assert _check_all(_hostcheck(tmp_path), tmp_path) == len(cases) + len(bulk)


def test_core_header_on_the_host_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: clean, and the same bits."""
    n = _check_all(_hostcheck(tmp_path, sanitize=True), tmp_path, fold_names=("n1-w33-T6", "n3-w33-T6", "n5-w64-T5", "n16-w1-T16", "n16-w64-T16"),
                   bulk_names=("n1-e40", "n3-e5", "n6-e120"))
    assert n == 8


def test_history_does_not_cross_a_reset(tmp_path):
    """The core header's fold (the host build's output, not the twin's) on two episodes back to back: every transition of the second
    episode carries the second episode's states and rewards only, s' and done are the newest hour's, hours 0 and 1 of an episode emit
    nothing.  The expectations are read off the staged data directly."""
    case = dict(NC.fold_cases())["n3-w1-T6"]
    stages = NC.staging(case)
    ring, pushed, _ = _run(_hostcheck(tmp_path), tmp_path, 0, case, stages)
    assert pushed == case["pos0"] + 8 and (ring["r"] == NR.SENT_F).sum() == 100 - 8
    d = [(case["pos0"] + q) % 100 for q in range(8)]                            # 4 pushes per episode, window 1
    assert list(ring["s"][d, 0]) == [0, 0, 0, 0, 1, 1, 1, 1] and list(ring["s"][d, 1]) == [0, 1, 2, 3, 0, 1, 2, 3]
    assert list(ring["s2"][d, 1] - f32(0.5)) == [2, 3, 4, 5, 2, 3, 4, 5]          # s2 is the newest hour's
    for q, slot in enumerate(d):
        e, t = divmod(q, 4)
        assert ring["r"][slot] == NR.horner(np.array([stages[e * 6 + t + k]["r"][0] for k in range(3)]), case["gamma"])
        assert ring["done"][slot] == stages[e * 6 + t + 2]["done"][0]


def test_return_is_within_one_ulp_of_the_direct_sum():
    """G against sum_k gamma64^k r_k by math.fsum over float64 products.  Bound: Horner makes at most 2 (n - 1) <= 30 roundings of
    2^-53 relative to partial sums bounded by sum |r_k|, so |acc - exact| <= 30 * 2^-53 * sum |r_k| -- far below float32's spacing
    -- and the final rounding to float32 adds half an ulp: one float32 ulp of the result, plus that float64 slack, holds."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in range(1, 17):
        for gamma in (0.99, 0.9, 0.5, 1.0, 0.0):
            r = (rng.normal(0, 1, (n, 200)) * 10.0 ** rng.integers(-3, 4, (n, 200))).astype(f32)
            G = NR.horner(r, gamma)
            for j in range(200):
                exact = NR.direct_sum(r[:, j], gamma)
                ulp = float(np.spacing(np.abs(f32(exact)))) if exact != 0 else float(np.spacing(f32(0)))
                slack = 30 * 2.0 ** -53 * float(np.abs(r[:, j].astype(f64)).sum())
                err = abs(float(G[j]) - exact)
                assert err <= ulp + slack, (n, gamma, j, err, ulp)
                worst = max(worst, err / ulp)
    assert worst <= 1.0


def test_known_answer():
    """gamma = 0.5 and r_h = h + 1: G = sum (k + 1) / 2^k is exact in binary."""
    for n in range(1, 17):
        r = np.arange(1, n + 1, dtype=f32)
        want = sum((k + 1) / 2.0 ** k for k in range(n))
        assert NR.horner(r, 0.5) == f32(want) and float(f32(want)) == want
    R = importlib.import_module(U.PKG_NAME + ".replay")
    assert R.nstep_gamma(0.5, 4) == 0.0625


def test_discount():
    R = importlib.import_module(U.PKG_NAME + ".replay")
    for g in (0.99, 0.9, 0.95, 1.0, 0.0, 0.999):
        assert R.nstep_gamma(g, 1) == float(f32(g)) == float(NR.nstep_gamma(g, 1))
        for n in (2, 3, 5, 16):
            p = f64(f32(g))
            for _ in range(n - 1):
                p = p * f64(f32(g))
            assert R.nstep_gamma(g, n) == float(f32(p)) == float(NR.nstep_gamma(g, n))
    assert R.nstep_gamma(0.99, 3) == float(f32(0.9702990126609802))           # float32(0.99)^3 in float64, rounded once
    for bad in (0, 17, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="1 .. 16"):
            R.nstep_gamma(0.99, bad)


def test_slab_layouts(built_lib):
    """An n_step = 1 group carves nothing: the DDPG, TD3 and prioritized groups' layouts are today's, tiled on and off.  n_step = 3:
    every earlier offset is unchanged and the new blocks come last."""
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    T = importlib.import_module(U.PKG_NAME + ".td3")
    ws = C.c_int64()
    assert D._declare().shems_ddpg_workspace_floats(C.byref(ws)) == 0
    assert G.nstep_extra_blocks(1, 64) == ()
    E, cap = 64, 24000
    for tiled, floats in ((False, 3702636), (True, 4751212)):
        assert G.slab_layout(D.N_ACTOR, D.N_CRITIC, ws.value, cap, tiled)[1] == floats          # (the figures tests/test_per_host.py holds)
        for extra in ((), tuple(T.group_extra_blocks(D.N_CRITIC, tiled, ws.value)), tuple(G.per_extra_blocks(cap))):
            base, n0 = G.slab_layout(D.N_ACTOR, D.N_CRITIC, ws.value, cap, tiled, extra)
            one, n1 = G.slab_layout(D.N_ACTOR, D.N_CRITIC, ws.value, cap, tiled, (*extra, *G.nstep_extra_blocks(1, E)))
            assert (one, n1) == (base, n0) and list(one) == list(base)
            lay, n3 = G.slab_layout(D.N_ACTOR, D.N_CRITIC, ws.value, cap, tiled, (*extra, *G.nstep_extra_blocks(3, E)))
            assert all(lay[k] == v for k, v in base.items()) and list(lay)[:len(base)] == list(base)
            new = list(lay)[len(base):]
            assert new == ["ns_stage_s", "ns_stage_a", "ns_stage_r", "ns_stage_s2", "ns_stage_done", "ns_hist_s", "ns_hist_a", "ns_hist_r"]
            assert lay["ns_stage_s"][0] == n0 and all(lay[k][0] % 4 == 0 for k in new)
            assert [lay[k][1] for k in new] == [E * 9, E * 2, E, E * 9, E // 4, 3 * E * 9, 3 * E * 2, 3 * E]
            assert n3 == lay["ns_hist_r"][0] + 3 * E


_C_TO_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double,
                "float": C.c_float}


def test_prototypes_struct_and_exports(built_lib, tmp_path):
    S = U.pkg()
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    sigs = S._capi._nstep_sigs()
    assert set(sigs) == {"shems_nstep_fold_dev", "shems_nstep_group_fold_dev", "shems_nstep_from_episodes_dev"}
    for name, args in sigs.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        decl = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(decl) == len(args), (name, decl)
        for d, a in zip(decl, args):
            if "*" in d:
                base = d.replace("const", "").split("*")[0].strip()
                want = {"shems_nstep": (C.POINTER(S._capi.NStepArgs),), "shems_replay": (C.POINTER(S._capi.Replay),)}.get(base, (C.c_void_p,))
                assert a in want, (name, d, a)
            else:
                assert a is _C_TO_CTYPES[d.split()[0]], (name, d, a)
    names = [f[0] for f in S._capi.NStepArgs._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shems_hip.h"\nint main(void){printf("%zu %d", sizeof(shems_nstep), '
                   "SHEMS_NSTEP_MAX);" + "".join(f'printf(" %zu", offsetof(shems_nstep, {n}));' for n in names) + "return 0;}\n")
    exe = tmp_path / "o"
    subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(S._capi.NStepArgs) == 48 and vals[1] == S._capi.NSTEP_MAX == NR.NSTEP_MAX == 16
    assert vals[2:] == [getattr(S._capi.NStepArgs, n).offset for n in names]
    core = open(os.path.join(U.ROOT, U.PKG_NAME, "csrc", "shems_nstep_core.h")).read()
    assert "kNstepMax = 16" in core
    assert set(sigs) <= set(S._capi.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib]).decode()
    assert set(sigs) <= set(re.findall(r" T (shems_[a-z0-9_]+)", out))
    L = S._capi.declare_nstep()
    assert all(getattr(L, n).argtypes == a for n, a in sigs.items())
    B = importlib.import_module(U.PKG_NAME + "._build")
    assert ("shems_nstep.hip", ["-ffp-contract=off"]) in B.UNITS


def test_native_argument_checks(built_lib):
    """Bad n, window, hour or capacities return SHEMS_ERR_ARG by name and launch nothing (no device is needed to be refused)."""
    S = U.pkg()
    L = S._capi.declare_nstep()
    NS, RP = S._capi.NStepArgs, S._capi.Replay
    ok_ring = lambda cap: RP(cap, 8, 8, 8, 8, 8)
    good = dict(ns=NS(3, 0, 33, 0.99, 0, 8, 8, 8), stage=ok_ring(33), ring=ok_ring(100), pos=90, hour=2)

    def fold(**kw):
        a = dict(good, **kw)
        rc = L.shems_nstep_fold_dev(C.byref(a["ns"]), C.byref(a["stage"]), C.byref(a["ring"]), a["pos"], a["hour"], None)
        return rc, L.shems_last_error().decode()
    for kw, word in ((dict(ns=NS(0, 0, 33, 0.99, 0, 8, 8, 8)), "n = 0"), (dict(ns=NS(17, 0, 33, 0.99, 0, 8, 8, 8)), "n = 17"),
                     (dict(ns=NS(3, 0, 0, 0.99, 0, 8, 8, 8)), "window = 0"), (dict(ns=NS(3, 0, 33, 0.99, 0, 0, 8, 8)), "history"),
                     (dict(hour=-1), "hour = -1"), (dict(stage=ok_ring(32)), "staging capacity 32"), (dict(ring=ok_ring(32)), "ring capacity 32"),
                     (dict(ring=RP(100, 8, 8, 0, 8, 8)), "incomplete replay ring"), (dict(pos=-1), "ring_pos = -1")):
        rc, msg = fold(**kw)
        assert rc == S._capi.ERR_ARG and "shems_nstep_fold_dev" in msg and word in msg, (kw, msg)
    grp = C.create_string_buffer(24)                                            # a zeroed shems_group: count 0
    rc = L.shems_nstep_group_fold_dev(C.byref(good["ns"]), C.byref(good["stage"]), C.byref(good["ring"]), grp, None, 90, 2, None)
    assert rc == S._capi.ERR_ARG and "shems_nstep_group_fold_dev: bad group" in L.shems_last_error().decode()
    rc = L.shems_nstep_group_fold_dev(C.byref(NS(17, 0, 33, 0.99, 0, 8, 8, 8)), C.byref(good["stage"]), C.byref(good["ring"]), grp, None, 90, 2, None)
    assert rc == S._capi.ERR_ARG and "shems_nstep_group_fold_dev: n = 17" in L.shems_last_error().decode()
    src, ring = ok_ring(30), RP(100, 16, 16, 16, 16, 16)
    for args, word in (((5, 6, 0, 0.99), "n = 0"), ((5, 6, 17, 0.99), "n = 17"), ((5, 2, 3, 0.99), "steps = 2 below n = 3"),
                       ((0, 6, 3, 0.99), "episodes = 0"), ((6, 6, 3, 0.99), "source capacity 30")):
        rc = L.shems_nstep_from_episodes_dev(C.byref(src), args[0], args[1], args[2], args[3], C.byref(ring), 0, None)
        msg = L.shems_last_error().decode()
        assert rc == S._capi.ERR_ARG and "shems_nstep_from_episodes_dev" in msg and word in msg, (args, msg)
    rc = L.shems_nstep_from_episodes_dev(C.byref(src), 5, 6, 3, 0.99, C.byref(src), 0, None)
    assert rc == S._capi.ERR_ARG and "same ring" in L.shems_last_error().decode()


class _Sync:
    def __init__(self, world):
        self.world, self.native = world, None


class _Dist:                                           # what GradSync reads of torch.distributed
    def __init__(self, world):
        self.world = world

    def is_initialized(self):
        return True

    def get_world_size(self):
        return self.world

    def get_rank(self):
        return 0


def test_python_level_refusals(built_lib):
    """Everything an n-step learner does not cover is refused by name before any device work."""
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    T = importlib.import_module(U.PKG_NAME + ".td3")
    R = importlib.import_module(U.PKG_NAME + ".replay")
    M = importlib.import_module(U.PKG_NAME + ".main")
    for cls in (D.Agent, T.TD3Agent):
        for bad in (0, 17, 2.5, None):
            with pytest.raises(ValueError, match="n_step.*1 .. 16"):
                cls(n_step=bad)
    ag = object.__new__(D.Agent)
    ag.__dict__.update(n_step=3, sync=_Sync(2), gamma=0.99)
    for what in ("episode_", "populate_memory"):
        with pytest.raises(NotImplementedError, match=what + ".*n_step = 3.*data-parallel.*sync.world = 2"):
            ag._nstep_refusals(what, 72)
    ag.sync = _Sync(1)
    with pytest.raises(ValueError, match="num_steps = 2 < n_step = 3"):
        ag._nstep_refusals("episode_", 2)
    ag._nstep_refusals("episode_", 3)
    assert ag.gamma_n == R.nstep_gamma(0.99, 3) and ag.gamma == 0.99
    ag.n_step = 1
    assert ag.gamma_n is ag.gamma                                               # n_step = 1: today's value, untouched
    env = types.SimpleNamespace(n=4, maxsteps=2)
    ag.n_step, ag._same_device = 3, lambda *a: None
    with pytest.raises(ValueError, match="populate_memory: num_steps = 2 < n_step = 3"):
        ag.populate_memory(env, types.SimpleNamespace(capacity=10, pushed=0))
    with pytest.raises(NotImplementedError, match="n_step = 3.*native loop.*shems_train_steps"):
        D.TrainWorkload(S, None, 64, 0, loop="native", n_step=3)
    with pytest.raises(NotImplementedError, match="n_step = 3: TrainWorkload.*no n-step mode"):
        D.TrainWorkload(S, None, 64, 0, n_step=3)
    before = ag.sync                                                            # a refused enable_data_parallel leaves the agent's sync alone
    with pytest.raises(NotImplementedError, match="enable_data_parallel: n_step = 3.*data-parallel.*sync.world = 2"):
        ag.enable_data_parallel(_Dist(2))
    assert ag.sync is before and ag.sync.world == 1
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    with pytest.raises(NotImplementedError, match="warm_start: n_step = 3.*one-step.*nothing was trained"):
        I.warm_start(ag, None, None, None, None, 1, 1, 1)
    with pytest.raises(NotImplementedError, match="warm_start_group: n_step = 5.*one-step"):
        I.warm_start_group(types.SimpleNamespace(n_step=5, has_evaluate=True), None, None, None, None, 1, 1, 1)
    for kw, word in ((dict(form="wide"), "form='wide'"), (dict(noise_type="ou"), "Ornstein-Uhlenbeck"),
                     (dict(hparams=[{"mem_size": 500}, {}, {}]), "per-learner mem_size")):
        with pytest.raises(NotImplementedError) as ei:
            G.LearnerGroup(3, 32, n_step=3, **kw)
        assert "n-step learner group" in str(ei.value) and word in str(ei.value), (kw, str(ei.value))
        G_ok = G.nstep_group_refusals(None, "gn", False)                        # (what the subclasses' groups pass: nothing refused)
        assert G_ok is None
    for cls in (G.LearnerGroup, T.TD3LearnerGroup, G.PrioritizedLearnerGroup):
        with pytest.raises(ValueError, match="n_step.*1 .. 16"):
            cls(3, 32, n_step=17)
    with pytest.raises(ValueError, match="n = 0"):
        R.NStepWindow(0, 4, 0.99)
    with pytest.raises(ValueError, match="window_count = 0"):
        R.NStepWindow(3, 0, 0.99)
    ns = types.SimpleNamespace(envs_per_learner=64, capacity=24000, tick=5, n_step=3)
    assert G.LearnerGroup.ring_window(ns, 72, None) == (64, 0) and G.LearnerGroup.ring_window(ns, 72, 7) == (7, 0)
    ns.n_step = 1
    assert G.LearnerGroup.ring_window(ns, 72, 7) == (7, 35)
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NSTEP": "3", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_IMITATE": "1x1",
           "SHEMS_FORESIGHT_WARMSTART": "4"}
    with pytest.raises(NotImplementedError, match="SHEMS_NSTEP = 3 with SHEMS_FORESIGHT_WARMSTART.*one-step"):
        M.main(env)


def test_hparam_records_carry_the_n_step_discount(built_lib):
    G = importlib.import_module(U.PKG_NAME + ".group")
    R = importlib.import_module(U.PKG_NAME + ".replay")
    hp = [{"gamma": 0.99}, {"gamma": 0.9}, {}]
    full1, arr1 = G._hparams_records(3, hp, 0.1, 1000)
    full3, arr3 = G._hparams_records(3, hp, 0.1, 1000, n_step=3)
    assert full1 == full3 and [r["gamma"] for r in full3] == [float(f32(0.99)), float(f32(0.9)), float(f32(0.99))]
    assert [arr1[l].gamma for l in range(3)] == [r["gamma"] for r in full1]                   # n_step = 1: today's records
    assert [arr3[l].gamma for l in range(3)] == [R.nstep_gamma(r["gamma"], 3) for r in full3]
    assert bytes(arr1) == bytes(G._hparams_records(3, hp, 0.1, 1000, n_step=1)[1])


def test_shems_nstep_parser():
    M = importlib.import_module(U.PKG_NAME + ".main")
    assert M.parse_nstep(None) == 1 and M.parse_nstep("1") == 1 and M.nstep_from_env({}) == 1
    assert M.parse_nstep("3") == 3 and M.nstep_from_env({"SHEMS_NSTEP": "16"}) == 16
    for bad in ("0", "17", "-1", "3.0", "three", "", "1e1", "2:3", "\u00b3", "\u0663"):
        with pytest.raises(ValueError) as ei:
            M.parse_nstep(bad)
        assert "SHEMS_NSTEP" in str(ei.value) and repr(bad) in str(ei.value)
    assert M.nstep_case_suffix(1) == "" and M.nstep_case_suffix(3) == "_n3"
    c = M.config_from_env({"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0"})
    base = c.case
    c.algo_suffix += M.nstep_case_suffix(1)
    assert c.case == base
    T = importlib.import_module(U.PKG_NAME + ".td3")
    c.algo_suffix = T.case_suffix(policy_delay=2, sigma_trg=0.2, clip_trg=0.5) + M.nstep_case_suffix(5)
    assert c.case.startswith(base + "_td3-") and c.case.endswith("_n5")
    c.algo_suffix = M.replay_case_suffix(alpha=0.6, beta0=0.4) + M.nstep_case_suffix(3)
    assert c.case == base + "_per-a0.6-b0.4_n3"

"""TD3 without a GPU: the NumPy twin against the DDPG oracle, the target-noise stream, a host build of csrc/shems_td3_core.h against
the twin bit for bit, the C struct, the exports, the schedule and the SHEMS_ALGO parser."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ddpg_oracle as DO
import td3_ref as TR
import util as U

f32 = np.float32


def _case(seed=11, n=1000, batch=24):
    rng = np.random.default_rng(seed)
    pa, pc = DO.init_params(seed, 9, 2, 0), DO.init_params(seed, 11, 1, 1)
    pc2 = DO.init_params(seed + 1000, 11, 1, 1)
    for p in (pc, pc2):
        p[128250:128750] *= 30.0
    pa[128000:129000] *= 30.0
    s = rng.random((n, 9)).astype(f32) * 5
    s2 = rng.random((n, 9)).astype(f32) * 5
    a = (rng.random((n, 2)) * 2 - 1).astype(f32)
    r = rng.normal(-1, 2, n).astype(f32)
    done = rng.random(n) < 0.05
    return dict(pa=pa, pc=pc, pc2=pc2, s=s, s2=s2, a=a, r=r, done=done, s_min=s.min(0), s_max=s.max(0), batch=batch)


def test_twin_degenerates_to_the_ddpg_oracle():
    """sigma_trg = 0, critic 2 a copy of critic 1, every update a policy step: the twin's update IS DO.Learner.replay -- every array
    equal (0 * z = 0, the clamp is the identity on tanh's range, min(q, q) = q)."""
    h = _case()
    tw = TR.Twin(h["pa"], h["pc"], h["pc"], h["s_min"], h["s_max"], sigma_trg=0.0, clip_trg=0.5)
    L = DO.Learner(h["pa"], h["pc"], h["s_min"], h["s_max"])
    for tick in range(3):
        idx = DO.sample_indices(11, tick, h["batch"], len(h["s"]))
        b = [h[k][idx] for k in ("s", "a", "r", "s2", "done")]
        lc, la = L.replay(*b)
        l1, l2, la2 = tw.replay(*b, seed=11, tick=tick, update_policy=True)
        assert (l1, la2) == (lc, la) and l2 == l1
        for name, ref in (("actor", L.actor), ("actor_t", L.actor_t), ("critic", L.critic), ("critic_t", L.critic_t)):
            assert np.array_equal(getattr(tw, name), ref), (tick, name)
        assert np.array_equal(tw.critic2, L.critic) and np.array_equal(tw.critic2_t, L.critic_t)
        for o, ro in ((tw.L.opt_a, L.opt_a), (tw.L.opt_c, L.opt_c), (tw.L2.opt_c, L.opt_c)):
            assert np.array_equal(o.m, ro.m) and np.array_equal(o.v, ro.v) and o.bp == ro.bp


def test_twin_leaves_the_actor_and_the_targets_alone_off_a_policy_step():
    h = _case()
    tw = TR.Twin(h["pa"], h["pc"], h["pc2"], h["s_min"], h["s_max"], sigma_trg=0.5, clip_trg=0.5)
    idx = DO.sample_indices(11, 3, h["batch"], len(h["s"]))
    b = [h[k][idx] for k in ("s", "a", "r", "s2", "done")]
    _, _, la = tw.replay(*b, seed=11, tick=3, update_policy=False)
    assert la is None
    assert np.array_equal(tw.actor, h["pa"]) and np.array_equal(tw.actor_t, h["pa"])
    assert np.array_equal(tw.critic_t, h["pc"]) and np.array_equal(tw.critic2_t, h["pc2"])
    assert not np.array_equal(tw.critic, h["pc"]) and not np.array_equal(tw.critic2, h["pc2"])
    assert tw.L.opt_a.bp == [0.9, 0.999] and tw.L.opt_c.bp == tw.L2.opt_c.bp == [0.9 * 0.9, 0.999 * 0.999]


def test_target_noise_stream():
    """Seed 11, tick 3: the words are DO.philox at counter (m, 0, tick, 0x5452474E); the draw is not the act noise's; eps and a~' stay
    inside their clamps."""
    n = 128
    ctr, (x, y, z, w) = TR.target_words(11, 3, n)
    assert (ctr[:, 0] == np.arange(n)).all() and (ctr[:, 1] == 0).all() and (ctr[:, 2] == 3).all() and (ctr[:, 3] == 0x5452474E).all()
    assert (ctr[:, 4] == 11).all() and (ctr[:, 5] == 0).all()
    for m in (0, 1, 77, 127):
        ref = DO.philox(m, 0, 3, 0x5452474E, 11, 0)
        assert (int(x[m]), int(y[m]), int(z[m]), int(w[m])) == tuple(int(v) for v in ref)
    assert TR.STREAM_TARGET not in (DO.STREAM_NOISE, DO.STREAM_SAMPLE, DO.STREAM_INIT, DO.STREAM_PERTURB)
    zn = TR.target_noise(11, 3, n)
    act = DO.gauss_noise(11, 3, n)
    assert zn.shape == act.shape == (n, 2) and zn.dtype == np.float32 and not (zn == act).any()
    assert abs(float(zn.mean())) < 0.25 and 0.8 < float(zn.std()) < 1.2
    seed_hi = (5 << 32) | 11
    assert (TR.target_words(seed_hi, 3, 4)[0][:, 5] == 5).all() and not (TR.target_noise(seed_hi, 3, n) == zn).any()
    rng = np.random.default_rng(0)
    a_t = np.tanh(rng.normal(0, 2, (n, 2))).astype(f32)
    for sigma, clip in ((0.2, 0.5), (0.5, 0.5), (2.0, 0.1), (0.0, 0.5), (0.3, 0.0)):
        eps = TR.noise_eps(zn, sigma, clip)
        a_sm = TR.smoothed_action(a_t, zn, sigma, clip)
        assert (np.abs(eps) <= f32(clip)).all() and (np.abs(a_sm) <= 1).all()
        if sigma == 0.0 or clip == 0.0:
            assert not eps.any() and np.array_equal(a_sm, a_t)
    assert (np.abs(TR.noise_eps(zn, 0.5, 0.5)) == f32(0.5)).any()


def _hostcheck(tmp_path, sanitize=False):
    exe = str(tmp_path / ("td3_hostcheck_san" if sanitize else "td3_hostcheck"))
    src = os.path.join(U.ROOT, "tests", "hostcheck", "td3_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] +
                          (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + ["-o", exe, src])
    return exe


def _hostcheck_inputs(n=300, seed=11, tick=3, sigma=0.5, clip=0.5):
    rng = np.random.default_rng(4)
    a_t = np.tanh(rng.normal(0, 2, (n, 2))).astype(f32)
    a_t[:4] = [[1.0, -1.0], [0.0, -0.0], [0.999999, -0.999999], [0.5, 0.5]]
    z = TR.target_noise(seed, tick, n)
    if sigma > 0:
        z[4] = [np.inf, -np.inf]                           # (0 * inf is a NaN: not a draw Box-Muller can make)
    z[5] = [0.0, -0.0]
    q1 = rng.normal(0, 3, n).astype(f32)
    q2 = (q1 + rng.normal(0, 1e-3, n)).astype(f32)
    q2[:8] = q1[:8]                                        # ties
    r = rng.normal(-1, 2, n).astype(f32)
    done = (rng.random(n) < 0.2).astype(f32)
    return dict(n=n, seed=seed, tick=tick, sigma=sigma, clip=clip, a_t=a_t, z=z, q1=q1, q2=q2, r=r, done=done)


def _run_hostcheck(exe, tmp_path, h):
    path = str(tmp_path / "td3_in.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<iIQ4f", h["n"], h["tick"], h["seed"], h["sigma"], h["clip"], float(DO.GAMMA), 0.0))
        for k in ("a_t", "z", "q1", "q2", "r", "done"):
            f.write(np.ascontiguousarray(h[k], f32).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = np.array([[int(w, 16) for w in line.split()[1:]] for line in out.stdout.strip().split("\n")], np.uint64).astype(np.uint32)
    assert rows.shape == (h["n"], 17)
    return rows


def _assert_hostcheck_equals_the_twin(rows, h):
    n = h["n"]
    ctr, words = TR.target_words(h["seed"], h["tick"], n)
    assert np.array_equal(rows[:, 0:6], ctr)
    assert np.array_equal(rows[:, 6:10], np.stack(words, 1))
    x, y = words[0], words[1]
    u1 = ((x >> np.uint32(8)).astype(f32) + f32(1)) * f32(1.0 / 16777216.0)
    u2 = (y >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)
    assert np.array_equal(rows[:, 10], U.bits32(u1)) and np.array_equal(rows[:, 11], U.bits32(u2))
    eps = TR.noise_eps(h["z"], h["sigma"], h["clip"])
    a_sm = TR.smoothed_action(h["a_t"], h["z"], h["sigma"], h["clip"])
    yv = TR.target_y(h["r"], h["done"], h["q1"], h["q2"])
    assert np.array_equal(rows[:, 12:14], U.bits32(eps)), "eps"
    assert np.array_equal(rows[:, 14:16], U.bits32(a_sm)), "smoothed action"
    assert np.array_equal(rows[:, 16], U.bits32(yv)), "y"
    assert (np.abs(a_sm) == 1).any() and (h["q2"] < h["q1"]).any() and (h["q1"] < h["q2"]).any()
    if h["sigma"] > 0:
        assert (np.abs(eps) == f32(h["clip"])).any()


def test_core_header_on_the_host_equals_the_twin_bit_for_bit(tmp_path):
    """tests/hostcheck/td3_hostcheck.cpp, g++ -ffp-contract=off: counter words, block words, the two uniforms, eps, a~' and y."""
    exe = _hostcheck(tmp_path)
    for kw in (dict(), dict(sigma=0.0), dict(sigma=0.2, clip=0.05, seed=(7 << 32) | 3, tick=0xFFFFFFFF)):
        h = _hostcheck_inputs(**kw)
        _assert_hostcheck_equals_the_twin(_run_hostcheck(exe, tmp_path, h), h)


def test_core_header_on_the_host_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: clean, and the same bits."""
    exe = _hostcheck(tmp_path, sanitize=True)
    h = _hostcheck_inputs(n=64)
    _assert_hostcheck_equals_the_twin(_run_hostcheck(exe, tmp_path, h), h)


def test_td3_record_matches_the_c_struct(tmp_path):
    T = importlib.import_module(U.PKG_NAME + ".td3")
    names = [f[0] for f in T.Td3Args._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shems_hip.h"\nint main(void){printf("%zu", sizeof(shems_td3));' +
                   "".join(f'printf(" %zu", offsetof(shems_td3, {n}));' for n in names) + 'return 0;}\n')
    exe = tmp_path / "o"
    subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(T.Td3Args)
    assert vals[1:] == [getattr(T.Td3Args, n).offset for n in names]
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    assert T.Td3Args.d.offset == 0 and T.Td3Args.critic2.offset == C.sizeof(D.DdpgArgs)


def test_td3_entry_points_are_exported(built_lib):
    S = U.pkg()
    names = S._capi.exported_symbols()
    assert "shems_td3_update" in names and "shems_td3_workspace_floats" in names
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib]).decode()
    exported = set(re.findall(r" T (shems_[a-z0-9_]+)", out))
    assert {"shems_td3_update", "shems_td3_workspace_floats"} <= exported


def test_policy_schedule():
    T = importlib.import_module(U.PKG_NAME + ".td3")
    got = {d: [T.is_policy_step(u, d) for u in range(10)] for d in (1, 2, 3)}
    assert got[1] == [True] * 10
    assert got[2] == [False, True] * 5
    assert got[3] == [False, False, True, False, False, True, False, False, True, False]
    with pytest.raises(ValueError):
        T.is_policy_step(0, 0)


def test_shems_algo_parser():
    T = importlib.import_module(U.PKG_NAME + ".td3")
    M = importlib.import_module(U.PKG_NAME + ".main")
    dflt = dict(policy_delay=2, sigma_trg=0.2, clip_trg=0.5)
    assert T.parse_algo(None) == ("ddpg", None) and T.parse_algo("ddpg") == ("ddpg", None)
    assert M.algo_from_env({}) == ("ddpg", None)
    assert T.parse_algo("td3") == ("td3", dflt)
    assert T.parse_algo("td3:3") == ("td3", dict(dflt, policy_delay=3))
    assert T.parse_algo("td3:1:0.1") == ("td3", dict(dflt, policy_delay=1, sigma_trg=0.1))
    assert T.parse_algo("td3:4:0:0.25") == ("td3", dict(policy_delay=4, sigma_trg=0.0, clip_trg=0.25))
    assert M.algo_from_env({"SHEMS_ALGO": "td3:2:0.2:0.5"}) == ("td3", dflt)
    for bad in ("sac", "TD3", "td3:0", "td3:two", "td3:2:-0.1", "td3:2:0.2:nan", "td3:2:0.2:0.5:1", "td3:2:inf", "td3::0.3", "td3:", ""):
        with pytest.raises(ValueError) as ei:
            T.parse_algo(bad)
        assert "SHEMS_ALGO" in str(ei.value) and repr(bad) in str(ei.value)
    # the case string: nothing for DDPG, a suffix of its own for TD3
    c = M.config_from_env({"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0"})
    base = c.case
    assert base.endswith("_ntrg0.2")
    c.algo_suffix = T.case_suffix(**dflt)
    assert c.case == base + "_td3-d2-s0.2-c0.5"

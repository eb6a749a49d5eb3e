"""Shared helpers for the test-suite: paths, case generators, oracle wrappers."""
from __future__ import annotations

import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

PKG_NAME = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"


def pkg():
    return importlib.import_module(PKG_NAME)


def tables_mod():
    return importlib.import_module(PKG_NAME + ".tables")


import oracle_c  # noqa: E402  (test infrastructure)
import shems_oracle_np as onp  # noqa: E402

CHARGER_IDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 98]


# ------------------------------------------------------------------ cases --
def single_step_cases(seed, n, rule_fraction=0.25):
    """Random + adversarial single-step cases.  Each case is an env sitting on row 1 of its own
    2-row table.  Returns dict of arrays."""
    rng = np.random.default_rng(seed)
    soc_max = np.float32(6.75)
    soc_b = (rng.random(n) * 7.0).astype(np.float32)
    soc_b[rng.random(n) < 0.15] = 0.0
    tiny = rng.random(n) < 0.1
    soc_b[tiny] = (rng.random(tiny.sum()) * 2e-2).astype(np.float32)
    full = rng.random(n) < 0.1
    soc_b[full] = soc_max
    soc_ev = rng.random(n).astype(np.float32)
    soc_ev[rng.random(n) < 0.2] = 1.0
    c_ev = rng.integers(-1, 30, n).astype(np.float32)
    c_ev[rng.random(n) < 0.35] = -1.0
    c_ev[rng.random(n) < 0.15] = 0.0
    d_e = np.round(0.195 + rng.random(n) * 6.0, 3).astype(np.float32)
    g_e = np.round(rng.random(n) * 20.0, 3).astype(np.float32)
    g_e[rng.random(n) < 0.45] = 0.0
    eq = rng.random(n) < 0.05
    g_e[eq] = d_e[eq]                                     # g_e == d_e edge
    p_buy = np.full(n, 0.4, np.float32)
    p_buy[rng.random(n) < 0.2] = np.float32(0.2963)
    hour = rng.integers(0, 24, n)
    h_cos = np.cos(2 * np.pi * hour / 23.0).astype(np.float32)
    h_sin = np.sin(2 * np.pi * hour / 23.0).astype(np.float32)
    season = rng.integers(1, 5, n).astype(np.float32)
    obs = np.stack([soc_b, soc_ev, c_ev, d_e, g_e, p_buy, h_cos, h_sin, season], 1).astype(np.float32)

    # next row
    n_c = np.where(c_ev > 0, c_ev - 1, -1.0).astype(np.float32)
    arrive = (c_ev == -1) & (rng.random(n) < 0.4)
    n_c[arrive] = rng.integers(0, 72, arrive.sum()).astype(np.float32)
    n_soc = np.ones(n, np.float32)
    n_soc[arrive] = rng.random(arrive.sum()).astype(np.float32)
    mid = (n_c >= 0) & ~arrive
    n_soc[mid] = rng.random(mid.sum()).astype(np.float32)  # must be ignored by next_state! (not newly connected)
    n_de = np.round(0.195 + rng.random(n) * 6.0, 3).astype(np.float32)
    n_ge = np.round(rng.random(n) * 20.0, 3).astype(np.float32)
    row_cur = np.stack([c_ev, soc_ev, d_e, g_e, p_buy, h_cos, h_sin, season], 1).astype(np.float32)
    row_next = np.stack([n_c, n_soc, n_de, n_ge, p_buy, h_cos, h_sin, season], 1).astype(np.float32)

    mode = np.where(rng.random(n) < rule_fraction, -1, 0).astype(np.int32)
    act = rng.random((n, 2)).astype(np.float32)
    edge = rng.random(n) < 0.1
    act[edge] = rng.choice(np.array([0.0, 1.0, 0.99, 0.98999], np.float32), (edge.sum(), 2))
    # rule mode: kWh set-points, some from the rule controller range, some arbitrary
    r = mode < 0
    act[r, 0] = ((rng.random(r.sum()) * 2 - 1) * 4.0).astype(np.float32)
    small = r & (rng.random(n) < 0.2)
    act[small, 0] = ((rng.random(small.sum()) * 2 - 1) * 0.02).astype(np.float32)
    act[r, 1] = (rng.random(r.sum()) * 11.0).astype(np.float32)
    act[r & (rng.random(n) < 0.3), 1] = 0.0
    return dict(obs=obs, row_cur=row_cur, row_next=row_next, act=act, mode=mode)


def oracle_profile(charger_id=98, w=None, pot=None, pen=None):
    return oracle_c.profile(charger_id, w, pot, pen)


def run_oracle_c(cases, prof):
    """Step every case with the C oracle.  Returns rewards, obs', results[23], B/EV."""
    n = len(cases["obs"])
    L = oracle_c.lib()
    rewards = np.zeros(n)
    obs2 = np.zeros((n, 9), np.float32)
    res = np.zeros((n, 23))
    env = oracle_c.Batch(1, 72, np.zeros((2, 8), np.float32), prof)
    for i in range(n):
        tab = np.ascontiguousarray(np.stack([cases["row_cur"][i], cases["row_next"][i]]), dtype=np.float32)
        L.orc_env_init(env.at(0), 72, tab.ctypes.data, 2, C.byref(prof))
        L.orc_env_set_state(env.at(0), np.ascontiguousarray(cases["obs"][i]).ctypes.data, 1, 0)
        r = C.c_double(0)
        a = np.ascontiguousarray(cases["act"][i], dtype=np.float32)
        rc = L.orc_step(env.at(0), a.ctypes.data_as(C.POINTER(C.c_float)), int(cases["mode"][i]), C.byref(r),
                        res[i].ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0
        rewards[i] = r.value
        L.orc_env_get_state(env.at(0), obs2[i].ctypes.data)
    return rewards, obs2, res


def run_oracle_np(cases, charger_id=98, w=0.01, pot=2.0, pen=0.1):
    n = len(cases["obs"])
    P = onp.Profile(charger_id, np.float32(w), np.float32(pot), np.float32(pen))
    rewards = np.zeros(n)
    obs2 = np.zeros((n, 9), np.float32)
    res = np.zeros((n, 23))
    for i in range(n):
        tab = np.stack([cases["row_cur"][i], cases["row_next"][i]])
        e = onp.Env(72, tab, P)
        e.state[:] = cases["obs"][i]
        e.idx = 1
        m = int(cases["mode"][i])
        r, s, rr = e.step_(cases["act"][i], track=(m if m < 0 else 1))
        rewards[i], obs2[i], res[i] = r, s, rr
    return rewards, obs2, res


# ------------------------------------------------------------- hostcheck --
class HCConfig(C.Structure):   # mirrors shems_config (include/shems_hip.h)
    _fields_ = [("cap_ev", C.c_float), ("soc_max", C.c_float), ("rate_max", C.c_double),
                ("disc_weight", C.c_double), ("disc_pot", C.c_double), ("penalty_weight", C.c_float),
                ("table_row0", C.c_int32), ("nrow", C.c_int32), ("reserved", C.c_int32)]


def hostcheck_lib():
    d = os.path.join(ROOT, "tests", "hostcheck")
    so = os.path.join(d, "libhostcheck.so")
    src = os.path.join(d, "hostcheck.cpp")
    core = os.path.join(ROOT, PKG_NAME, "csrc", "shems_core.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(core)) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-o", so, src])
    return C.CDLL(so)


def cfg_from_profile(prof, row0=0, nrow=2):
    return HCConfig(prof.cap_ev, prof.soc_max, prof.rate_max, prof.disc_weight, prof.disc_pot,
                    prof.penalty_weight, row0, nrow, 0)


def run_hostcheck(cases, prof):
    L = hostcheck_lib()
    n = len(cases["obs"])
    cfg = cfg_from_profile(prof)
    rewards = np.zeros(n)
    obs2 = np.zeros((n, 9), np.float32)
    flows = np.zeros((n, 12))
    bev = np.zeros((n, 2), np.float32)
    fp = C.POINTER(C.c_float)
    for i in range(n):
        r = C.c_double(0)
        L.hc_step(C.byref(cfg), cases["obs"][i].ctypes.data_as(fp), cases["row_cur"][i].ctypes.data_as(fp),
                  cases["row_next"][i].ctypes.data_as(fp), cases["act"][i].ctypes.data_as(fp), int(cases["mode"][i]),
                  obs2[i].ctypes.data_as(fp), C.byref(r), flows[i].ctypes.data_as(C.POINTER(C.c_double)),
                  bev[i].ctypes.data_as(fp))
        rewards[i] = r.value
    return rewards, obs2, flows, bev


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------ per-env configs --
SWEEP = ((0.01, 2.0), (0.04, 2.0), (0.1, 2.0), (0.01, 1.0), (0.04, 1.0), (0.1, 1.0))     # env.mixed_profile_setup's default


def mixed_batches(n, co=None, maxsteps=72):
    """BASELINE config 5 on the device and in the C oracle: the tables of env.mixed_profile_setup (real series of 4 319 / 4 320 rows
    where the reference holds one), one config per (charger profile, sweep point), config co[i] for env i (default i mod 60).
    Returns (ShemsBatch, oracle_c.Batch, tables, configs, co, table_of_env)."""
    S = pkg()
    tabs, cfgs, co0 = S.mixed_profile_setup(n)
    co = co0 if co is None else np.ascontiguousarray(co, dtype=np.uint16)
    assert co.shape == (n,) and int(co.max()) < len(cfgs)
    profs = [oracle_c.profile(c, w, pot) for c in CHARGER_IDS for (w, pot) in SWEEP]
    tab_of = np.repeat(np.arange(len(CHARGER_IDS)), len(SWEEP))[co]
    env = S.ShemsBatch(n, maxsteps, tabs, cfgs, co)
    ref = oracle_c.Batch(n, maxsteps, tabs, profs, tab_of, co)
    return env, ref, tabs, cfgs, co, tab_of


def learner_grid_cfgs(count, envs_per_learner):
    """The thesis grid of a learner group on the mixed_profile_setup configs: every env of learner l on charger profile l mod 10, the
    weight point l mod 6 (one learner: env i on config i mod 60)."""
    n = count * envs_per_learner
    if count == 1:
        return (np.arange(n) % (len(CHARGER_IDS) * len(SWEEP))).astype(np.uint16)
    l = np.arange(n) // envs_per_learner
    return (len(SWEEP) * (l % len(CHARGER_IDS)) + l % len(SWEEP)).astype(np.uint16)


def obs_of_rows(tab, idx, soc_b):
    """The observation of envs sitting on 1-based rows `idx` of `tab` (the layout reset! leaves: soc_b, soc_ev, h, d_e, g_e, p_buy,
    h_cos, h_sin, season)."""
    rows = tab[np.asarray(idx) - 1]
    return np.concatenate([np.asarray(soc_b, np.float32)[:, None], rows[:, [1, 0]], rows[:, 2:]], 1).astype(np.float32)


# ------------------------------------------ the throughput group's variants --
def group_variant_refusal_rows(name, update, head, entry, mem_tail, batch_words):
    """The rows the two variants of the throughput group share (td3.group_refusals, group.per_group_refusals), every message in full: one
    per fault, then pairs of faults adjacent in the walk's order, the earlier one reported."""
    form = f"{name}: form={{!r}} has no {head}; the group runs the throughput form ({entry}) whatever its count"
    ou = f"{name}: Ornstein-Uhlenbeck noise runs on the *_x entry points, which have no {update}"
    hid = f"{name}: hidden= belongs to form='wide', which has no {update}"
    mem = f"{name}: hparams[{{}}]: per-learner mem_size runs on the *_x entry points, which have no {update}{mem_tail}"
    bat = f"{name}: hparams[{{}}]: batch 129 > 128: {batch_words}"
    wid = f"{name}: hparams[{{}}]: hidden (300, 600) is wider than (250, 500): the wide form has no {update}"
    NI = NotImplementedError
    return [(dict(form="latency"), NI, form.format("latency")), (dict(form="wide"), NI, form.format("wide")),
            (dict(form="fast"), ValueError, "form must be 'throughput'"), (dict(noise_type="ou"), NI, ou), (dict(hidden=(300, 600)), NI, hid),
            (dict(hparams=[{"mem_size": 64}, {}]), NI, mem.format(0)), (dict(hparams=[{}, {"batch": 129}]), NI, bat.format(1)),
            (dict(hparams=[{"hidden": (300, 600)}, {}]), NI, wid.format(0)),
            (dict(form="wide", noise_type="ou"), NI, form.format("wide")), (dict(form="fast", noise_type="ou"), ValueError, "form must be 'throughput'"),
            (dict(noise_type="ou", hidden=(300, 600)), NI, ou), (dict(hidden=(300, 600), hparams=[{"mem_size": 64}]), NI, hid),
            (dict(hparams=[{"mem_size": 64, "batch": 129}]), NI, mem.format(0)), (dict(hparams=[{"batch": 129, "hidden": (300, 600)}]), NI, bat.format(0)),
            (dict(hparams=[{"hidden": (300, 600)}, {"mem_size": 64}]), NI, wid.format(0)),       # (record by record: learner 0's last check first)
            (dict(hparams=[(), {"batch": 129}]), NI, bat.format(1))]                                # (a record that is no mapping is passed over)

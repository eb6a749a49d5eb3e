"""Shared by the regret tests: the audit of a tracked pass restated on the C oracle, and oracle-made trajectories to audit.

The twin follows the definition at the end of csrc/shems_foresight_core.h, NOT the package: for hour t of a pass the state is read
back from the 23-column row (Soc_b column 22, Soc_ev column 4, c_ev column 1; load, PV and price from the table row the row index
names), one oracle env per action is put into that state (oracle_c.Batch.set_state) and stepped with the DRL step, V_{t+1} is read
at the state each leaves with foresight_twin.interp, and the FIRST maximum is taken.  achieved_q is the row's reward plus V_{t+1} at
the state of the NEXT row (plus 0.0 in the last hour), v_state is V_t at the row's state.  Nothing is imported from foresight.py.
Every trajectory is computed once per process and shared (functools.lru_cache); callers must not modify what they get.
"""
from __future__ import annotations

import functools

import numpy as np

import foresight_twin as FT
import util as U
from util import oracle_c


def twin_audit(V, results, tab, prof, idx0, nb, ne, nab, nae):
    """V [T + 1][nb * ne] float64, results [T][23] float64 of a pass that starts on 1-based row idx0 of `tab`.  Returns
    (out [T][3] float64 = best_q, achieved_q, v_state; best_action [T] int32)."""
    V, res = np.asarray(V, np.float64), np.asarray(results, np.float64)
    T = res.shape[0]
    assert V.shape == (T + 1, nb * ne) and res.shape == (T, 23)
    acts = FT.action_grid(nab, nae)
    A = len(acts)
    idx = res[:, 0].astype(np.int64) - 1                                    # column 0 holds the row index after the step
    assert (idx == idx0 + np.arange(T)).all(), "the pass does not sit on rows idx0 .. idx0 + T - 1"
    soc_b, soc_ev, c_ev = res[:, 22].astype(np.float32), res[:, 4].astype(np.float32), res[:, 1].astype(np.float32)
    assert (soc_b.astype(np.float64) == res[:, 22]).all() and (soc_ev.astype(np.float64) == res[:, 4]).all()   # stored floats: exact
    obs = U.obs_of_rows(tab, idx, soc_b)                                    # d_e, g_e, p_buy (and the rest) of table row idx
    obs[:, 1], obs[:, 2] = soc_ev, c_ev
    ref = oracle_c.Batch(T * A, 1, tab, prof)
    ref.set_state(np.repeat(obs, A, axis=0), np.repeat(idx, A))
    rc, r, o2, _ = ref.step(np.ascontiguousarray(np.tile(acts, (T, 1))), 0)
    assert rc == 0
    r, sb2, se2 = r.reshape(T, A), o2[:, 0].reshape(T, A), o2[:, 1].reshape(T, A)
    out = np.zeros((T, 3), np.float64)
    best = np.zeros(T, np.int32)
    for t in range(T):
        q = r[t] + FT.interp(V[t + 1], nb, ne, prof.soc_max, sb2[t], se2[t])
        best[t] = int(np.argmax(q))                                          # the first maximum
        out[t, 0] = q[best[t]]
        nxt = FT.interp(V[t + 1], nb, ne, prof.soc_max, soc_b[t + 1], soc_ev[t + 1]) if t < T - 1 else 0.0
        out[t, 1] = res[t, 5] + nxt
        out[t, 2] = FT.interp(V[t], nb, ne, prof.soc_max, soc_b[t], soc_ev[t])
    return out, best


# ------------------------------------------------------------ trajectories --
def _start(tab, prof, idx0, T, soc_b0):
    ref = oracle_c.Batch(1, T, tab, prof)
    s0 = np.float32(0.5 * float(prof.soc_max)) if soc_b0 is None else np.float32(soc_b0)
    ref.set_state(U.obs_of_rows(tab, np.array([idx0]), np.array([s0], np.float32)), np.array([idx0], np.int64), np.zeros(1, np.int64))
    return ref


def rule_pass(tab, prof, idx0, T, soc_b0=None):
    """The rule-based controller (action(env, track), step! with track < 0) from row idx0: [T][23]."""
    ref, res = _start(tab, prof, idx0, T, soc_b0), np.zeros((T, 23))
    for t in range(T):
        rc, _, _, rr = ref.step(ref.action_rule(), -1, want_results=True)
        assert rc == 0
        res[t] = rr[0]
    return res


def random_pass(tab, prof, idx0, T, seed=5, soc_b0=None):
    """Random DRL targets, np.random.default_rng(seed).random((1, 2)).astype(float32) per hour, stepped with track_mode 0: [T][23]."""
    ref, res, rng = _start(tab, prof, idx0, T, soc_b0), np.zeros((T, 23)), np.random.default_rng(seed)
    for t in range(T):
        rc, _, _, rr = ref.step(rng.random((1, 2)).astype(np.float32), 0, want_results=True)
        assert rc == 0
        res[t] = rr[0]
    return res


def greedy_pass(V, tab, prof, idx0, nb, ne, nab, nae, soc_b0=None):
    """The greedy pass on the planes V [T + 1][N]: at every hour the first maximum of the twin's Q from the oracle env's own state.
    Returns ([T][23], actions [T] int32)."""
    T = V.shape[0] - 1
    ref, res, took = _start(tab, prof, idx0, T, soc_b0), np.zeros((T, 23)), np.zeros(T, np.int32)
    acts = FT.action_grid(nab, nae)
    A = len(acts)
    probe = oracle_c.Batch(A, 1, tab, prof)
    for t in range(T):
        probe.set_state(np.repeat(ref.state(), A, axis=0), np.full(A, idx0 + t, np.int64))
        rc, r, o2, _ = probe.step(acts, 0)
        assert rc == 0
        took[t] = int(np.argmax(r + FT.interp(V[t + 1], nb, ne, prof.soc_max, o2[:, 0], o2[:, 1])))
        rc, _, _, rr = ref.step(acts[took[t]:took[t] + 1], 0, want_results=True)
        assert rc == 0
        res[t] = rr[0]
    return res, took


@functools.lru_cache(maxsize=None)
def s1_passes():
    """S1's three trajectories from Soc_b = 0.5 soc_max: rule, greedy on the twin's V, random.  (results [3][30][23], greedy actions)."""
    d = FT.s1()
    T = FT.S1["T"]
    g = {k: FT.S1[k] for k in ("nb", "ne", "nab", "nae")}
    greedy, took = greedy_pass(d["V"], d["tab"], d["prof"], d["idx0"], **g)
    return np.stack([rule_pass(d["tab"], d["prof"], d["idx0"], T), greedy, random_pass(d["tab"], d["prof"], d["idx0"], T)]), took


@functools.lru_cache(maxsize=None)
def s1_twin():
    """The twin's audit of s1_passes(): (out [3][30][3], best_action [3][30])."""
    d = FT.s1()
    res, _ = s1_passes()
    g = {k: FT.S1[k] for k in ("nb", "ne", "nab", "nae")}
    both = [twin_audit(d["V"], r, d["tab"], d["prof"], d["idx0"], **g) for r in res]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


S2_PASSES = (3, 0, 2, 1, 0)                                                  # problem_of_pass of the S2 case


@functools.lru_cache(maxsize=None)
def s2_passes():
    """Five random-target passes on S2's four problems, each from its problem's start row (seeds 5 .. 9): results [5][8][23]."""
    d = FT.s2()
    return np.stack([random_pass(d["tabs"][p], d["profs"][p], d["idx0"][p], FT.S2["T"], seed=5 + k) for k, p in enumerate(S2_PASSES)])


@functools.lru_cache(maxsize=None)
def s2_twin():
    d = FT.s2()
    g = {k: FT.S2[k] for k in ("nb", "ne", "nab", "nae")}
    both = [twin_audit(d["V"][p], r, d["tabs"][p], d["profs"][p], d["idx0"][p], **g) for r, p in zip(s2_passes(), S2_PASSES)]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def phase_of(c_ev, h_next):
    """The EV phase of an hour: 0 absent, 1 arrival (takes precedence over absent), 2 connected, 3 departure."""
    if c_ev == -1:
        return 1 if h_next >= 0 else 0
    return 3 if c_ev == 0 else 2

"""Shared by the warm-start tests: a NumPy twin of the transitions call and of the critic-only update.

Part 1 follows the definition in csrc/shems_foresight_core.h (fs_transition_hour, fs_returns), NOT the package: for hour t of a pass
with a successor, s and s2 are the observations of imitation_ref for rows t and t + 1, a is the label of the targets the row records
(columns 21 and 2), r is float32(column 5); the return-to-go is G[T - 1] = r[T - 1], G[t] = r[t] + float64(float32(gamma)) * G[t + 1],
the product rounded, then the sum.  TD slots hold (s, a, r, s2, 0), MC slots (s, a, float32(G[t]), s2, 1); (pass e, hour t) goes to
slot (pos + e * (T - tail) + t) mod capacity.  Part 2 is the critic step of oracle/ddpg_oracle.py on one minibatch.
Results that are cached (functools.lru_cache) are shared: callers must not modify what they get.
"""
from __future__ import annotations

import functools

import numpy as np

import ddpg_oracle as DO
import imitation_ref as IR

TD, MC = 0, 1
TRANSITION_MODE = {"td": TD, "mc": MC}
ERR_INDEX = IR.ERR_INDEX
f32 = np.float32


# ------------------------------------------------------------------ transitions --
def returns(rewards, gamma):
    """G of one pass, float64, sequentially from the end."""
    r = np.asarray(rewards, np.float64)
    g = np.float64(f32(gamma))
    G = np.empty_like(r)
    G[-1] = r[-1]
    for t in range(len(r) - 2, -1, -1):
        carried = g * G[t + 1]
        G[t] = r[t] + carried
    return G


def obs(r, tab, idx0, t):
    row = tab[idx0 + t - 1]
    return np.array([f32(r[22]), f32(r[4]), f32(r[1]), row[2], row[3], row[4], row[5], row[6], row[7]], f32)


def twin_transitions(results, tabs, idx0s, mode, gamma, tail, pos=0, capacity=None):
    """results [n][T][23] float64; tabs / idx0s: per pass, the table and the 1-based start row of its problem (None: the pass names no
    problem).  Returns dict(slot [n][T - tail] int64, -1 where the hour gives no transition; s, s2 [n][T - tail][9], a [..][2],
    r [..] float32, done [..] uint8; status [n] int32; G [n][T] float64, NaN in a pass the returns refuse)."""
    res = np.asarray(results, np.float64)
    n, T, _ = res.shape
    keep = T - tail
    assert 1 <= tail < T
    capacity = n * keep if capacity is None else int(capacity)
    assert n * keep <= capacity and 0 <= pos < capacity
    out = dict(slot=np.full((n, keep), -1, np.int64), s=np.zeros((n, keep, 9), f32), s2=np.zeros((n, keep, 9), f32),
               a=np.zeros((n, keep, 2), f32), r=np.zeros((n, keep), f32), done=np.zeros((n, keep), np.uint8),
               status=np.zeros(n, np.int32), G=np.full((n, T), np.nan))
    for e in range(n):
        tab, idx0 = tabs[e], idx0s[e]
        hour_ok = [tab is not None and IR.row_ok(res[e, t, 0], t, idx0, tab.shape[0]) for t in range(T)]
        finite = np.isfinite(res[e, :, 5])
        pass_ok = all(hour_ok) and bool(finite.all())
        if pass_ok:
            out["G"][e] = returns(res[e, :, 5], gamma)
        if mode == MC and not pass_ok:
            out["status"][e] = ERR_INDEX
            continue
        for t in range(keep):
            r = res[e, t]
            if not (hour_ok[t] and hour_ok[t + 1] and finite[t]):
                out["status"][e] = ERR_INDEX
                continue
            out["s"][e, t], out["s2"][e, t] = obs(r, tab, idx0, t), obs(res[e, t + 1], tab, idx0, t + 1)
            out["a"][e, t] = IR.label(np.array([r[21], r[2]]).astype(f32))
            out["r"][e, t] = f32(out["G"][e, t]) if mode == MC else f32(r[5])
            out["done"][e, t] = 1 if mode == MC else 0
            out["slot"][e, t] = (pos + e * keep + t) % capacity
    return out


RING_ARRAYS = (("s", (9,), f32), ("a", (2,), f32), ("r", (), f32), ("s2", (9,), f32), ("done", (), np.uint8))


def sentinel_arrays(capacity, byte):
    """The five ring arrays with every byte set to `byte`."""
    return {k: np.frombuffer(bytes([byte]) * (capacity * int(np.prod(sh, dtype=np.int64)) * np.dtype(dt).itemsize), dt)
            .reshape((capacity,) + sh).copy() for k, sh, dt in RING_ARRAYS}


def fill(tw, capacity, sentinel=None):
    """The five ring arrays a transitions call leaves, from `sentinel` (sentinel_arrays) or zeros."""
    ring = {k: np.zeros((capacity,) + sh, dt) for k, sh, dt in RING_ARRAYS} if sentinel is None else {k: v.copy() for k, v in sentinel.items()}
    ok = tw["slot"] >= 0
    for k, _, _ in RING_ARRAYS:
        ring[k][tw["slot"][ok]] = tw[k][ok]
    return ring


# ------------------------------------------------------------------ critic step --
CRITIC_SEED, CRITIC_TICK = IR.CLONE_SEED, IR.CLONE_TICK
CRITIC_CASES = IR.CLONE_CASES                                                 # (batch, ring length), ring capacity IR.CLONE_CAP


def learner(d):
    """The oracle's learner on critic_data: live networks and the (different) targets."""
    L = DO.Learner(d["pa"], d["pc"], d["s_min"], d["s_max"])
    L.actor_t, L.critic_t = d["pa_t"].copy(), d["pc_t"].copy()
    return L


def critic_reference(batch, ring_len, reward="r", done=None, dtype=np.float64, critic=None, seed=CRITIC_SEED, tick=CRITIC_TICK):
    """(gradient in `dtype`, loss, targets y (float32, the oracle's), minibatch slots) of the critic step of one case on critic_data.
    reward: "r" (hourly rewards) or "G" (returns: the MC ring); done: None = the data's own, or one value for every slot."""
    d = critic_data()
    idx = DO.sample_indices(seed, tick, batch, ring_len)
    L = learner(d)
    if critic is not None:
        L.critic = np.asarray(critic)
    dn = d["done"][idx] if done is None else np.full(batch, done, np.uint8)
    y = L.targets(d[reward][idx], d["s2"][idx], dn.astype(bool))
    g, loss = L.critic_grad(d["s"][idx], d["a"][idx], y, dtype=dtype)
    return g, loss, y, idx


@functools.lru_cache(maxsize=None)
def critic_data(seed=IR.CLONE_SEED, cap=IR.CLONE_CAP):
    """clone_data's ring completed to full transitions: s2 spread like s, rewards of the env's hourly magnitude, done with both values
    present, a critic whose 3e-3 head is lifted as the actor's is, and targets that differ from the live networks."""
    d = IR.clone_data(seed, cap)
    rng = np.random.default_rng(seed + 1)
    s2 = d["s"][rng.permutation(cap)].copy()
    s2[:, 0] = rng.random(cap) * 6.75
    r = (-rng.random(cap) * 2.5).astype(f32)
    done = (rng.random(cap) < 0.3).astype(np.uint8)
    done[0], done[1] = 0, 1
    pc = d["pc"].copy()
    n = len(pc)
    pc[n - 501:n - 1] *= 30.0
    pc[11 * 250:11 * 250 + 250] = rng.normal(0, 0.05, 250)
    pa_t = (d["pa"] + rng.normal(0, 1e-3, len(d["pa"]))).astype(f32)
    pc_t = (pc + rng.normal(0, 1e-3, n)).astype(f32)
    # returns of the magnitude of real ones (a pass of Charger98 sums to a few hundred), for the MC ring
    G = (-rng.random(cap) * 400.0).astype(f32)
    return dict(d, s2=s2, r=r, done=done, pc=pc, pa_t=pa_t, pc_t=pc_t, G=G)

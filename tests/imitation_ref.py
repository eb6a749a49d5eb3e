"""Shared by the imitation tests: a NumPy twin of the demo conversion and of the supervised (cloning) update.

Part 1 follows the definition in csrc/shems_foresight_core.h (fs_demo_hour), NOT the package: for hour t of a pass the row check of
the audit is restated, the observation is (Soc_b column 22, Soc_ev column 4, c_ev column 1 of the 23-column row, as float32; columns
2 .. 7 of the table row the row index names), the label is float32(2.0 * float64(target) - 1.0), and (pass e, hour t) goes to slot
(pos + e * T + t) mod capacity.  Part 2 is the clone step -- loss = Flux.mse(actor(normalize(s)), a_demo) -- built from
oracle/ddpg_oracle.py (mlp_forward, mlp_backward, Adam, soft_update, sample_indices) in float32 and float64.
Results that are cached (functools.lru_cache) are shared: callers must not modify what they get.
"""
from __future__ import annotations

import functools

import numpy as np

import ddpg_oracle as DO
import foresight_twin as FT

ERR_INDEX = -3
f32 = np.float32


# --------------------------------------------------------------- demo conversion --
def label(target):
    """a = (float)(2.0 * (double)target - 1.0), element-wise."""
    return (2.0 * np.asarray(target, f32).astype(np.float64) - 1.0).astype(f32)


def scale_action(a):
    """DDPG.jl:178-184 with bounds (0, 1): Float32((a + 1.0) * 0.5), in float64."""
    return ((np.asarray(a, f32).astype(np.float64) + 1.0) * 0.5).astype(f32)


def row_ok(x, t, idx0, nrow):
    """The audit's row check on column 0 of a results row (the row index AFTER the step)."""
    if not (x >= 1.0 and x <= 2147483647.0):
        return False
    idx = int(x) - 1
    return idx >= 1 and idx == idx0 + t and idx + 1 <= nrow


def twin_demos(results, tab, idx0, nab, nae, targets=None, best_action=None, pos=0, capacity=None):
    """results [n][T][23] float64 of passes that start on 1-based row idx0 of `tab`; exactly one of targets [n][T][2] float32 and
    best_action [n][T] int.  Returns (slot [n][T] int64, -1 where the hour gives no pair; s [n][T][9] float32; a [n][T][2] float32;
    status [n] int32)."""
    assert (targets is None) != (best_action is None)
    res = np.asarray(results, np.float64)
    n, T, _ = res.shape
    capacity = n * T if capacity is None else int(capacity)
    assert n * T <= capacity and 0 <= pos < capacity
    tb, te = FT.targets(nab), FT.targets(nae)
    slot = np.full((n, T), -1, np.int64)
    s, a, status = np.zeros((n, T, 9), f32), np.zeros((n, T, 2), f32), np.zeros(n, np.int32)
    for e in range(n):
        for t in range(T):
            r = res[e, t]
            ok = row_ok(r[0], t, idx0, tab.shape[0])
            if ok and best_action is not None:
                k = int(best_action[e][t])
                ok = 0 <= k < nab * nae
            if not ok:
                status[e] = ERR_INDEX
                continue
            row = tab[idx0 + t - 1]
            s[e, t] = [f32(r[22]), f32(r[4]), f32(r[1]), row[2], row[3], row[4], row[5], row[6], row[7]]
            tgt = np.asarray(targets[e][t], f32) if targets is not None else np.array([tb[k // nae], te[k % nae]], f32)
            a[e, t] = label(tgt)
            slot[e, t] = (pos + e * T + t) % capacity
    return slot, s, a, status


def fill(slot, s, a, capacity, sentinel=None):
    """The ring arrays (s [capacity][9], a [capacity][2]) a demos call leaves, from `sentinel` (s0, a0) or zeros."""
    S = np.zeros((capacity, 9), f32) if sentinel is None else sentinel[0].copy()
    A = np.zeros((capacity, 2), f32) if sentinel is None else sentinel[1].copy()
    ok = slot >= 0
    S[slot[ok]], A[slot[ok]] = s[ok], a[ok]
    return S, A


# ------------------------------------------------------------------ clone step --
def clone_grad(actor, s, a_demo, s_min, s_max, dtype=np.float32):
    """d Flux.mse(actor(normalize(s)), a_demo) / d actor (flat, Flux.params order) and the loss, arithmetic in `dtype`; the network
    input is the float32 normalize(s) in both (what the kernels read)."""
    sn = DO.normalize(s, s_min, s_max)
    y, cache = DO.mlp_forward(actor, sn, DO.STATE, DO.ACTION, True, keep=True, dtype=dtype)
    B = len(s)
    diff = (y - np.asarray(a_demo, f32).astype(dtype)).astype(dtype)
    dy = (diff / dtype(B)).astype(dtype)                       # d mean(diff^2 over 2 B elements) / d y = 2 diff / (2 B)
    g, _ = DO.mlp_backward(actor, cache, dy, DO.STATE, DO.ACTION, True, dtype=dtype)
    return g, float(np.mean(diff * diff))


class CloneLearner:
    """actor, actor_t and one ADAM: clone() = one supervised update on the minibatch sample_indices names."""

    def __init__(self, actor, s_min, s_max, eta=DO.ETA_ACT, actor_t=None):
        self.actor = np.asarray(actor, f32).copy()
        self.actor_t = self.actor.copy() if actor_t is None else np.asarray(actor_t, f32).copy()
        self.opt = DO.Adam(len(self.actor), eta)
        self.s_min, self.s_max = np.asarray(s_min, f32), np.asarray(s_max, f32)

    def clone(self, s_ring, a_ring, ring_len, seed, tick, batch, tau=1.0, dtype=np.float32):
        idx = DO.sample_indices(seed, tick, batch, ring_len)
        g, loss = clone_grad(self.actor, s_ring[idx], a_ring[idx], self.s_min, self.s_max, dtype)
        self.actor = self.opt.step(self.actor, g.astype(f32))
        self.actor_t = DO.soft_update(self.actor_t, self.actor, f32(tau))
        return g, loss


# ------------------------------------------------- the clone cases of the GPU test --
CLONE_CAP = 128                                                              # a full ring: length == capacity
CLONE_CASES = [(B, n) for B in (1, 7, 120, 128) for n in (1, 90, CLONE_CAP)]   # (batch, ring length)
CLONE_SEED, CLONE_TICK = 11, 3


@functools.lru_cache(maxsize=None)
def clone_data(seed=CLONE_SEED, cap=CLONE_CAP):
    """A ring of `cap` synthetic demonstrations (states spread like the env's, labels in [-1, 1] with a fifth of them exactly at the
    ends) and an actor whose 3e-3 head is lifted so that every gradient path is exercised."""
    rng = np.random.default_rng(seed)
    s = np.empty((cap, 9), f32)
    s[:, 0] = rng.random(cap) * 6.75
    s[:, 1] = rng.random(cap)
    s[:, 2] = rng.integers(-1, 30, cap)
    s[:, 3:5] = rng.random((cap, 2)) * 5
    s[:, 5] = np.where(rng.random(cap) < 0.2, 0.2963, 0.4)
    hour = rng.integers(0, 24, cap)
    s[:, 6], s[:, 7], s[:, 8] = np.cos(2 * np.pi * hour / 23.0), np.sin(2 * np.pi * hour / 23.0), rng.integers(1, 5, cap)
    a = (rng.random((cap, 2)) * 2 - 1).astype(f32)
    ends = rng.random((cap, 2)) < 0.2
    a[ends] = np.where(rng.random(int(ends.sum())) < 0.5, f32(-1), f32(1))
    pa, pc = DO.init_params(seed, 9, 2, 0), DO.init_params(seed, 11, 1, 1)
    pa[128000:129000] *= 30.0
    pa[2250:2500] = rng.normal(0, 0.05, 250)
    return dict(s=s, a=a, s_min=s.min(0), s_max=s.max(0), pa=pa, pc=pc)


def clone_reference(batch, ring_len, dtype, seed=CLONE_SEED, tick=CLONE_TICK, actor=None):
    """(gradient, loss, minibatch slots) of the clone step of one case on clone_data, in `dtype`."""
    d = clone_data()
    idx = DO.sample_indices(seed, tick, batch, ring_len)
    g, loss = clone_grad(d["pa"] if actor is None else actor, d["s"][idx], d["a"][idx], d["s_min"], d["s_max"], dtype)
    return g, loss, idx


def twin_loss_distance():
    """The float32 twin's distance from float64 in the loss over CLONE_CASES, as a fraction of max(1, |loss|): {case: distance}."""
    out = {}
    for B, n in CLONE_CASES:
        l32, l64 = clone_reference(B, n, np.float32)[1], clone_reference(B, n, np.float64)[1]
        out[B, n] = abs(l32 - l64) / max(1.0, abs(l64))
    return out

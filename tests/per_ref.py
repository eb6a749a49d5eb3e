"""NumPy twin of prioritized replay (include/shems_hip.h: shems_ddpg_update_per; csrc/shems_per_core.h).  TEST INFRASTRUCTURE ONLY.

The sampler (fresh slots, the block sums in the definition's order, the stratified draw, the importance weights), the priority
write-back, and the weighted critic head on top of oracle/ddpg_oracle.py.  Float32 throughout, one rounding per operation; the two
powers are evaluated in float64 as well (the arbiter the tolerance-class outputs are held to).
"""
from __future__ import annotations

import numpy as np

import ddpg_oracle as DO

f32 = np.float32
STREAM_PER = 0x50455253                      # kStreamPer of csrc/philox.h
BLOCK, CHUNK, COLS = 256, 64, 128
ALPHA, BETA, EPS_P = 0.6, 0.4, 1e-6
PW_T, PW_IDX, PW_W, PW_U, PW_TM, PW_S = 0, 4, 132, 260, 388, 516     # the workspace carve (floats)


def n_blocks(slots):
    return (int(slots) + BLOCK - 1) // BLOCK


def ws_floats(capacity):
    return (PW_S + 2 * n_blocks(capacity) + 3) // 4 * 4


def fresh_mask(n, fresh_pos, fresh_count, capacity):
    """Which of the slots [0, n) are fresh: fresh_count >= capacity = all, else ((i - fresh_pos) mod capacity) < fresh_count."""
    i = np.arange(n, dtype=np.int64)
    if fresh_count >= capacity:
        return np.ones(n, bool)
    return ((i - int(fresh_pos)) % int(capacity)) < int(fresh_count)


def chunk_sums(x):
    """x [k][64] float32 -> [k]: the balanced pairwise tree, six levels (wave_sum's association; IEEE addition commutes)."""
    v = np.asarray(x, f32)
    while v.shape[1] > 1:
        v = (v[:, 0::2] + v[:, 1::2]).astype(f32)
    return v[:, 0]


def block_sums(prio, ring_len):
    """(S [nb], C [nb], T) over the slots [0, ring_len), zero-padded to blocks of 256: S_b = ((s0 + s1) + s2) + s3, C_b running."""
    nb = n_blocks(ring_len)
    p = np.zeros(nb * BLOCK, f32)
    p[:ring_len] = np.asarray(prio, f32)[:ring_len]
    s = chunk_sums(p.reshape(nb * 4, CHUNK)).reshape(nb, 4)
    S = (((s[:, 0] + s[:, 1]).astype(f32) + s[:, 2]).astype(f32) + s[:, 3]).astype(f32)
    C = np.empty(nb, f32)
    run = f32(0)
    for b in range(nb):
        run = S[b] if b == 0 else f32(run + S[b])
        C[b] = run
    return S, C, C[-1]


def uniforms(seed, tick, n=COLS):
    """u_m = (w >> 8) 2^-24, w = word m & 3 of the Philox block at counter (m >> 2, 0, tick, STREAM_PER), key seed."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    xs = DO.philox(q, 0, tick, STREAM_PER, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = np.stack(xs, 1).reshape(-1)[:n]
    return ((w >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)


def targets(u, T, batch):
    """t_m = (m + u_m) * (T / batch): three roundings."""
    m = np.arange(len(u)).astype(f32)
    a = (m + u).astype(f32)
    seg = f32(f32(T) / f32(batch))
    return (a * seg).astype(f32)


def search(prio, S, C, t, ring_len):
    """The slot of one target t (step 3)."""
    nb = len(C)
    hit = np.nonzero(C > t)[0]
    if len(hit):
        b = int(hit[0])
    else:
        pos = np.nonzero(S > 0)[0]
        b = int(pos[-1]) if len(pos) else 0
    j0 = b * BLOCK
    p = np.zeros(BLOCK, f32)
    n = max(0, min(BLOCK, ring_len - j0))
    p[:n] = prio[j0:j0 + n]
    r = C[b - 1] if b > 0 else f32(0)
    run = np.add.accumulate(np.concatenate(([r], p)).astype(f32))[1:]      # sequential, one float32 rounding per slot
    assert run.dtype == f32
    over = np.nonzero(run > t)[0]
    if len(over):
        j = j0 + int(over[0])
    else:
        pos = np.nonzero(p > 0)[0]
        j = j0 + (int(pos[-1]) if len(pos) else BLOCK - 1)
    return min(j, ring_len - 1)


def raw_weights(ring_len, pi, T, beta, dtype=np.float32):
    """(ring_len pi / T)^(-beta); 1 where beta = 0, T = 0 or pi = 0.  dtype float64: x in float32 as the device forms it, the power
    in float64."""
    pi = np.asarray(pi, f32)
    if beta == 0.0 or not T > 0:
        return np.ones(len(pi), dtype)
    with np.errstate(divide="ignore"):
        x = ((f32(ring_len) * pi).astype(f32) / f32(T)).astype(f32)
        if dtype == np.float32:
            raw = np.power(x, f32(-beta)).astype(f32)
        else:
            raw = np.power(x.astype(np.float64), -float(f32(beta)))
    return np.where(pi > 0, raw, dtype(1)).astype(dtype)


def weights(ring_len, pi, T, beta, batch, dtype=np.float32):
    raw = raw_weights(ring_len, pi, T, beta, dtype)
    out = np.zeros(len(raw), dtype)
    out[:batch] = raw[:batch] / raw[:batch].max()
    return out


def new_priority(diff, eps_p, alpha, dtype=np.float32):
    """(|diff| + eps_p)^alpha; dtype float64: the sum in float32 as the device forms it, the power in float64."""
    base = (np.abs(np.asarray(diff, f32)) + f32(eps_p)).astype(f32)
    if dtype == np.float32:
        return np.power(base, f32(alpha)).astype(f32)
    return np.power(base.astype(np.float64), float(f32(alpha)))


def sample(prio, pmax, capacity, ring_len, fresh_pos, fresh_count, seed, tick, batch, beta):
    """Steps 1-4.  prio [capacity] is updated in place.  Returns a dict with S, C, T, u, t, idx [128] (-1 in the pad columns),
    slots [128] (the pad columns' too), w [128]."""
    fm = fresh_mask(ring_len, fresh_pos, fresh_count, capacity)
    prio[:ring_len][fm] = f32(pmax)
    S, C, T = block_sums(prio, ring_len)
    u = uniforms(seed, tick)
    t = targets(u, T, batch)
    slots = np.array([search(prio, S, C, t[m], ring_len) for m in range(COLS)], np.int64)
    idx = np.where(np.arange(COLS) < batch, slots, -1).astype(np.int32)
    w = weights(ring_len, prio[slots], T, beta, batch)
    return dict(S=S, C=C, T=T, u=u, t=t, idx=idx, slots=slots, w=w, fresh=fm)


def write_back(prio, pmax, slots, diff, eps_p, alpha):
    """Step 6 on the live columns: the highest column wins a slot drawn twice.  Returns the new pmax."""
    pn = new_priority(diff, eps_p, alpha)
    for m in range(len(slots)):                       # ascending: a later column overwrites
        prio[slots[m]] = pn[m]
    return f32(max(f32(pmax), pn.max()))


class PerLearner(DO.Learner):
    """DO.Learner with the weighted critic head: dq = 2 w diff / B, loss = sum w diff^2 / B."""

    def critic_grad_w(self, s, a, y, w, dtype=np.float32):
        sn = DO.normalize(s, self.s_min, self.s_max)
        q, cache = DO.mlp_forward(self.critic, np.concatenate([sn, a], 1), 11, 1, False, keep=True, dtype=dtype)
        B = len(y)
        diff = (q[:, 0] - y).astype(dtype)
        dq = (dtype(2) * np.asarray(w, dtype) * diff / dtype(B)).astype(dtype)[:, None]
        g, _ = DO.mlp_backward(self.critic, cache, dq, 11, 1, False, dtype=dtype)
        return g, float(np.sum(np.asarray(w, np.float64) * diff.astype(np.float64) ** 2) / B), diff

    def replay_w(self, s, a, r, s2, done, w):
        """One update on given columns and weights.  Returns (loss_critic, loss_actor, diff)."""
        y = self.targets(r, s2, done)
        gc, lc, diff = self.critic_grad_w(s, a, y, w)
        self.critic = self.opt_c.step(self.critic, gc)
        ga, la = self.actor_grad(s)
        self.actor = self.opt_a.step(self.actor, ga)
        self.actor_t = DO.soft_update(self.actor_t, self.actor)
        self.critic_t = DO.soft_update(self.critic_t, self.critic)
        return lc, la, diff

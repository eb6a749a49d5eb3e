"""NumPy twin of one TD3 update (include/shems_hip.h: shems_td3_update).  TEST INFRASTRUCTURE ONLY.

Everything DDPG has is taken from oracle/ddpg_oracle.py unchanged (philox, normalize, the forward passes, Learner.critic_grad(s, a, y),
Learner.actor_grad, Adam, soft_update); this file adds what TD3 adds: the target-noise stream, the smoothed target action, the twin
minimum, and one replay(update_policy).  Float32 throughout, as the oracle; the gradients can also be evaluated in float64 (the arbiter
the per-block bounds are held to).
"""
from __future__ import annotations

import numpy as np

import ddpg_oracle as DO

f32 = np.float32
STREAM_TARGET = 0x5452474E                   # kStreamTarget of csrc/philox.h
SIGMA_TRG, CLIP_TRG = 0.2, 0.5


def target_words(seed, tick, n):
    """The Philox block of minibatch column m < n: counter (m, 0, tick, STREAM_TARGET), key seed.  Returns (counter words [n][6] uint32
    as csrc/shems_td3_core.h's td3_counter lists them, block words (x, y, z, w))."""
    m = np.arange(n, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    ctr = np.stack([m.astype(np.uint32), np.zeros(n, np.uint32), np.full(n, tick & 0xFFFFFFFF, np.uint32), np.full(n, STREAM_TARGET, np.uint32),
                    np.full(n, k0, np.uint32), np.full(n, k1, np.uint32)], 1)
    return ctr, DO.philox(m, 0, tick, STREAM_TARGET, k0, k1)


def target_noise(seed, tick, n):
    """DO.gauss_noise with the target tag: Box-Muller on words x, y of one block per column, u1 from (x >> 8) + 1, u2 from y >> 8."""
    _, (x, y, _, _) = target_words(seed, tick, n)
    u1 = ((x >> np.uint32(8)).astype(f32) + f32(1)) * f32(1.0 / 16777216.0)
    u2 = (y >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)
    r = np.sqrt(f32(-2) * np.log(u1)).astype(f32)
    ang = (f32(6.28318530717958647692) * u2).astype(f32)
    return np.stack([r * np.cos(ang), r * np.sin(ang)], 1).astype(f32)


def noise_eps(z, sigma_trg, clip_trg):
    """eps = clamp(sigma_trg * z, -clip_trg, clip_trg)"""
    return np.clip((f32(sigma_trg) * np.asarray(z, f32)).astype(f32), -f32(clip_trg), f32(clip_trg)).astype(f32)


def smoothed_action(a_target, z, sigma_trg, clip_trg):
    """a~' = clamp(actor_t(s') + eps, -1, 1)"""
    return np.clip((np.asarray(a_target, f32) + noise_eps(z, sigma_trg, clip_trg)).astype(f32), f32(-1), f32(1)).astype(f32)


def twin_min(q1, q2):
    return np.where(q2 < q1, q2, q1).astype(f32)


def target_y(r, done, q1, q2, gamma=DO.GAMMA):
    """y = r + gamma (1 - done) min(q'1, q'2), rounded after every operation (no fused multiply-add)."""
    return (np.asarray(r, f32) + f32(gamma) * (f32(1) - np.asarray(done).astype(f32)) * twin_min(q1, q2)).astype(f32)


class Twin:
    """actor / critic / critic2 + targets + three ADAMs; replay(update_policy) = one TD3 update."""

    def __init__(self, actor, critic, critic2, s_min, s_max, sigma_trg=SIGMA_TRG, clip_trg=CLIP_TRG):
        self.L = DO.Learner(actor, critic, s_min, s_max)                 # actor + critic 1 and their optimisers
        self.L2 = DO.Learner(actor, critic2, s_min, s_max)               # critic 2 (its actor fields are not used)
        self.sigma_trg, self.clip_trg = float(sigma_trg), float(clip_trg)

    # the learner's arrays under the names the device uses
    actor = property(lambda self: self.L.actor)
    actor_t = property(lambda self: self.L.actor_t)
    critic = property(lambda self: self.L.critic)
    critic_t = property(lambda self: self.L.critic_t)
    critic2 = property(lambda self: self.L2.critic)
    critic2_t = property(lambda self: self.L2.critic_t)

    def targets(self, r, s2, done, seed, tick, a_smooth=None):
        """Every stage of the target: a' = actor_t(s'_n), z, eps, a~', q'1, q'2, y.  a_smooth: take the target critics from this a~'
        instead (the device's own previous stage)."""
        L = self.L
        s2n = DO.normalize(s2, L.s_min, L.s_max)
        a_t = DO.actor_forward(L.actor_t, s2n)
        z = target_noise(seed, tick, len(r))
        eps = noise_eps(z, self.sigma_trg, self.clip_trg)
        a_sm = smoothed_action(a_t, z, self.sigma_trg, self.clip_trg)
        a_in = a_sm if a_smooth is None else np.asarray(a_smooth, f32)
        q1 = DO.critic_forward(L.critic_t, s2n, a_in)
        q2 = DO.critic_forward(self.L2.critic_t, s2n, a_in)
        return dict(a_t=a_t, z=z, eps=eps, a_smooth=a_sm, q1=q1, q2=q2, y=target_y(r, done, q1, q2))

    def critic_grads(self, s, a, y, dtype=np.float32):
        """((g1, loss1), (g2, loss2)) of Flux.mse(critic_i([s_n; a]), y)."""
        return self.L.critic_grad(s, a, y, dtype=dtype), self.L2.critic_grad(s, a, y, dtype=dtype)

    def replay(self, s, a, r, s2, done, seed, tick, update_policy=True):
        """One update in replay()'s order (DDPG.jl:121-145).  Returns (loss_critic1, loss_critic2, loss_actor or None)."""
        L, L2 = self.L, self.L2
        y = self.targets(r, s2, done, seed, tick)["y"]
        (g1, l1), (g2, l2) = self.critic_grads(s, a, y)
        L.critic = L.opt_c.step(L.critic, g1)
        L2.critic = L2.opt_c.step(L2.critic, g2)
        if not update_policy:
            return l1, l2, None
        ga, la = L.actor_grad(s)                                         # through the updated critic 1
        L.actor = L.opt_a.step(L.actor, ga)
        L.actor_t = DO.soft_update(L.actor_t, L.actor)
        L.critic_t = DO.soft_update(L.critic_t, L.critic)
        L2.critic_t = DO.soft_update(L2.critic_t, L2.critic)
        return l1, l2, la

"""NumPy twin of the behaviour-regularised actor loss (csrc/shems_bc_core.h; include/shems_hip.h at shems_ddpg_update_bc):

    Qbar     = (1/B) sum_m |q_m|
    lambda   = normalise ? alpha / max(Qbar, 1e-8f) : alpha            (a constant of the update)
    loss_act = -lambda mean(q) + weight mse(a_pi, a)                    (mse over the 2 B elements)
    dloss    = lambda da + weight (a_pi - a) / B                        (da = d(-mean q) / d a_pi)

The scalar functions are float32, uncontracted (what tests/hostcheck/bc_hostcheck.cpp prints, bit for bit); actor_grad / loss take a
dtype and are the float64 arbiter of the GPU tests."""
import numpy as np

import ddpg_oracle as DO

f32 = np.float32
Q_FLOOR = f32(1e-8)


def lam(alpha, qbar, normalise):
    """bc_lambda: float32; the maximum is a compare, so a NaN Qbar meets the floor."""
    alpha, qbar = f32(alpha), f32(qbar)
    den = qbar if qbar > Q_FLOOR else Q_FLOOR
    return f32(alpha / den) if normalise else alpha


def dloss(lmbda, da, weight, diff, batch):
    """bc_dloss: every operation rounded to float32 (-ffp-contract=off)."""
    lmbda, weight, batch = f32(lmbda), f32(weight), f32(batch)
    da, diff = np.asarray(da, f32), np.asarray(diff, f32)
    return ((lmbda * da).astype(f32) + ((weight * diff).astype(f32) / batch).astype(f32)).astype(f32)


def loss(lmbda, neg_mean_q, weight, mse):
    """bc_loss, float32 uncontracted."""
    return f32(f32(f32(lmbda) * f32(neg_mean_q)) + f32(f32(weight) * f32(mse)))


def q_abs_mean(q, dtype=np.float64):
    q = np.asarray(q, dtype)
    return dtype(np.abs(q).sum() / dtype(len(q)))


def actor_parts(L, s, a, dtype=np.float64):
    """Through learner L's actor and critic on the minibatch (s, a): a_pi, q, da = d(-mean q)/d a_pi [B][2], the actor's cache."""
    sn = DO.normalize(s, L.s_min, L.s_max)
    a_pi, ca = DO.mlp_forward(L.actor, sn, 9, 2, True, keep=True, dtype=dtype)
    q, cc = DO.mlp_forward(L.critic, np.concatenate([sn.astype(dtype), a_pi], 1), 11, 1, False, keep=True, dtype=dtype)
    B = len(s)
    _, dx = DO.mlp_backward(L.critic, cc, np.full((B, 1), dtype(-1.0 / B), dtype), 11, 1, False, dtype=dtype)
    return a_pi, q[:, 0], dx[:, 9:], ca


def actor_grad(L, s, a, lmbda, weight, dtype=np.float64):
    """(gradient of loss_act wrt the actor's flat parameters with lambda held constant, loss_act, the two terms of step 4 [B][2],
    -mean q, mse)."""
    a_pi, q, da, ca = actor_parts(L, s, a, dtype)
    B = len(s)
    diff = a_pi - np.asarray(a, dtype)
    t_q, t_bc = dtype(lmbda) * da, dtype(weight) * diff / dtype(B)
    g, _ = DO.mlp_backward(L.actor, ca, t_q + t_bc, 9, 2, True, dtype=dtype)
    nmq, mse = -float(np.mean(q)), float(np.mean(diff ** 2))
    return g, float(lmbda) * nmq + float(weight) * mse, (t_q, t_bc), nmq, mse


def loss_of(L, actor, s, a, lmbda, weight):
    """loss_act in float64 for the flat actor `actor` with lambda held constant (the finite difference's function)."""
    sn = DO.normalize(s, L.s_min, L.s_max).astype(np.float64)
    a_pi = DO.mlp_forward(actor, sn, 9, 2, True, dtype=np.float64)
    q = DO.mlp_forward(L.critic, np.concatenate([sn, a_pi], 1), 11, 1, False, dtype=np.float64)[:, 0]
    return -float(lmbda) * float(np.mean(q)) + float(weight) * float(np.mean((a_pi - np.asarray(a, np.float64)) ** 2))

// shems_bc_core.h -- the scalar arithmetic of the behaviour-regularised actor loss (TD3+BC), written once (host + device functions).
//
// TD3+BC (Fujimoto, Gu 2021) holds the actor to the data while the critic improves it:
//   loss_act = -lambda mean_m(q_m) + weight Flux.mse(a_pi, a),   q_m = critic([s_n; a_pi])_m,  a = the ring's stored action
//   Qbar     = (1/B) sum_{m<B} |q_m|
//   lambda   = normalise ? alpha / max(Qbar, 1e-8f) : alpha       (a constant of the update: no gradient flows through it)
// and at the actor's output, for the live columns m < B,
//   d loss / d a_pi[o][m] = lambda da[o][m] + weight (a_pi - a)[o][m] / B,   da = d(-mean q) / d a_pi  (K4's partials, summed)
// (the mse runs over 2 B elements: d mse / d a_pi = 2 (a_pi - a) / (2 B)).  Pad columns m >= B give 0.  include/shems_hip.h states the
// whole update at shems_ddpg_update_bc; the summation orders of Qbar, mean q and the mse are the kernel's (head_actor_bc).
//
// Everything in here is IEEE multiply / add / divide / compare and is checked bit for bit by a host build
// (tests/hostcheck/bc_hostcheck.cpp, g++ -ffp-contract=off) against the NumPy twin (tests/bc_ref.py).
//
// Contraction: bc_lambda has no multiply feeding an add.  bc_dloss and bc_loss do: they take the contraction of the translation unit
// that includes this header.  The host check builds with -ffp-contract=off; shems_ddpg.hip keeps hipcc's default, under which
// lambda da + t becomes fma(lambda, da, t) -- with lambda = 1 and weight = 0 that is da + 0 = da exactly, which keeps the head on
// head_actor's bits (tests/test_bc_gpu.py pins it).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHEMS_BC_HD __host__ __device__ inline
#else
#define SHEMS_BC_HD inline
#endif

namespace shems {

constexpr float kBcQFloor = 1e-8f;

// lambda = normalise ? alpha / max(Qbar, 1e-8f) : alpha.  The maximum is a compare, so that a NaN Qbar meets the floor on both sides.
SHEMS_BC_HD float bc_lambda(float alpha, float qbar, int normalise)
{
    const float den = qbar > kBcQFloor ? qbar : kBcQFloor;
    return normalise ? alpha / den : alpha;
}
// d loss / d a_pi of one live element: lambda da + weight diff / B, diff = a_pi - a
SHEMS_BC_HD float bc_dloss(float lambda, float da, float weight, float diff, float batch) { return lambda * da + weight * diff / batch; }
// loss_act = lambda (-mean q) + weight mse
SHEMS_BC_HD float bc_loss(float lambda, float neg_mean_q, float weight, float mse) { return lambda * neg_mean_q + weight * mse; }

}  // namespace shems

// shems_td3_core.h -- the scalar arithmetic of TD3's target stage, written once (host + device functions).
//
// TD3 (Fujimoto, van Hoof, Meger 2018) forms the critics' common target from a SMOOTHED target action and the SMALLER of two target
// critics.  For minibatch column m of update `tick` with sampler key `seed`:
//   (z0, z1) = Box-Muller on words x, y of the Philox4x32-10 block at counter (m, 0, tick, kStreamTarget), key seed
//              (u1 from (x >> 8) + 1, u2 from y >> 8: the transform of the act noise, on a stream tag of its own)
//   eps_o    = clamp(sigma_trg * z_o, -clip_trg, clip_trg)
//   a~'_o    = clamp(actor_t(s'_n)_o + eps_o, -1, 1)
//   y        = r + gamma (1 - done) min(q'_1, q'_2),   q'_i = critic_i_t([s'_n; a~'])
// The logarithm, square root, sine and cosine of Box-Muller are NOT in here: they are library functions that differ between a host
// libm and the device (tolerance-class arithmetic, as in the act path); everything in here is IEEE multiply / add / compare, takes the
// two normals as inputs, and is checked bit for bit by a host build (tests/hostcheck/td3_hostcheck.cpp, g++ -ffp-contract=off).
//
// Contraction: eps and a~' have no multiply feeding an add, so they round the same under any -ffp-contract.  y = r + (gamma (1 - done))
// q' does: it takes the contraction of the translation unit that includes this header.  The host check builds with -ffp-contract=off
// and equals the NumPy twin bit for bit; shems_ddpg.hip keeps hipcc's default, under which this line contracts exactly as head_loss's
// y (DDPG.jl:133) does -- which is what keeps TD3 with sigma_trg = 0 and equal critics on DDPG's bits.
#pragma once

#include "philox.h"

namespace shems {

// The Philox block of column m: counter words and key.
struct Td3Counter { uint32_t c0, c1, c2, c3, k0, k1; };
PHILOX_HD Td3Counter td3_counter(uint64_t seed, uint32_t tick, uint32_t m)
{
    return Td3Counter{m, 0u, tick, (uint32_t)kStreamTarget, (uint32_t)seed, (uint32_t)(seed >> 32)};
}
PHILOX_HD u32x4 td3_block(uint64_t seed, uint32_t tick, uint32_t m)
{
    const Td3Counter c = td3_counter(seed, tick, m);
    return philox4x32_10(c.c0, c.c1, c.c2, c.c3, c.k0, c.k1);
}
// The two uniforms Box-Muller takes: u1 in (0, 1], u2 in [0, 1), both exact in float32.
PHILOX_HD float td3_u1(const u32x4 &x) { return ((float)(x.x >> 8) + 1.0f) * (1.0f / 16777216.0f); }
PHILOX_HD float td3_u2(const u32x4 &x) { return u01_24(x.y); }

// clamp(x, lo, hi) as Julia's clamp / np.clip: a NaN passes through.
PHILOX_HD float td3_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
// eps = clamp(sigma_trg * z, -clip_trg, clip_trg)
PHILOX_HD float td3_eps(float sigma_trg, float clip_trg, float z) { return td3_clamp(sigma_trg * z, -clip_trg, clip_trg); }
// a~' = clamp(a' + eps, -1, 1)
PHILOX_HD float td3_smooth(float a_target, float eps) { return td3_clamp(a_target + eps, -1.0f, 1.0f); }
// min(q'_1, q'_2): the first where they are equal
PHILOX_HD float td3_min(float q1, float q2) { return q2 < q1 ? q2 : q1; }
// y = r + gamma (1 - done) q'   (DDPG.jl:133 with the twin minimum in the place of q')
PHILOX_HD float td3_y(float r, float gamma, float done, float qmin) { return r + gamma * (1.0f - done) * qmin; }

}  // namespace shems

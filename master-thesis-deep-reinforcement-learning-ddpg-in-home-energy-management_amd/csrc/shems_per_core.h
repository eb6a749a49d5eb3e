// shems_per_core.h -- prioritized experience replay (Schaul et al. 2016, proportional variant): the arithmetic of the sampler and of the
// priority write-back, written once (host + device functions).  The reference has no such sampler; the definition is this one, in
// replay()'s conventions (Float32, fixed summation orders, the Philox counter generator).
//
// A prioritized ring is a shems_replay plus prio [capacity] (pi_j = p_j^alpha >= 0, the power already applied) and pmax [1] (the running
// maximum of every pi ever written, 1.0 at the start, never decreasing).  One draw of `batch` columns from the slots [0, ring_len):
//   1. fresh slots: slot i is fresh when fresh_count >= capacity or ((i - fresh_pos) mod capacity) < fresh_count; a fresh slot's
//      priority IS pmax[0] (stored before anything is summed).
//   2. sums: the slots are cut into blocks of 256 (the last one zero-padded), a block into four chunks of 64.
//        chunk sum  s   = the balanced pairwise tree over the 64 values: (x0 + x1), ((x0 + x1) + (x2 + x3)), ... six levels
//                         (what the six DPP adds of wave_sum compute; IEEE addition commutes, so the tree alone fixes the bits)
//        block sum  S_b = ((s0 + s1) + s2) + s3
//        running    C_b = C_{b-1} + S_b in block order, C_{-1} = 0 (so C_0 = S_0);  T = C_last
//   3. stratified draw: u_m = (w >> 8) 2^-24, w = word m & 3 of the Philox block at counter (m >> 2, 0, tick, kStreamPer), key seed;
//      t_m = (m + u_m) * (T / batch), the product rounded on its own (no contraction; the sum m + u_m rounds once).
//      block b_m = the first b with C_b > t_m; when there is none, the last block with S_b > 0 (block 0 when every priority is zero).
//      slot: r = C_{b-1}; for the slots j of the block in order, r = r + pi_j; j_m = the first j with r > t_m; when there is none
//      (the sequential order inside the block and the tree order of S_b may differ in the last place) the last slot of the block
//      with pi_j > 0, and the block's last slot when it has none; at most ring_len - 1.  A slot with pi_j = 0 is therefore drawn
//      only when every priority of the block the search ends in is zero.
//   4. importance weights: x_m = (ring_len * pi_{j_m}) / T, raw_m = x_m^(-beta) (1 where beta = 0, where T = 0 and where pi = 0: powf
//      would give an infinity there); w_m = raw_m / max over the live columns.  powf is a library function: tolerance class.
//   6. write-back: pi_new = (|diff| + eps_p)^alpha (powf: tolerance class); where several columns drew one slot the HIGHEST column's
//      value is stored; pmax = max(pmax, every pi_new of the live columns).
// Everything except the two powf calls is IEEE add / multiply / divide / compare and is checked bit for bit against the NumPy twin
// (tests/per_ref.py) by a host build (tests/hostcheck/per_hostcheck.cpp, g++ -ffp-contract=off).
#pragma once

#include <math.h>

#include "philox.h"

namespace shems {

constexpr int kPerBlock = 256;             // slots per block of the sum structure
constexpr int kPerChunk = 64;              // slots per chunk (one wave)
constexpr int kPerCols = 128;              // columns of a draw (the update's padded batch)
constexpr int64_t kPerMaxSlots = 262144;   // one workgroup holds every chunk and block sum in LDS: 4096 + 2 * 1024 floats

// Workspace carve of a prioritized ring (floats): what k_per_sample publishes.
constexpr int64_t PW_T = 0;                // [1] T   [1] max raw weight   [1] number of blocks (as int32)   [1] reserved
constexpr int64_t PW_IDX = 4;              // [128] int32: the drawn slots, -1 in the pad columns
constexpr int64_t PW_W = PW_IDX + kPerCols;    // [128] importance weights, 0 in the pad columns
constexpr int64_t PW_U = PW_W + kPerCols;      // [128] u_m
constexpr int64_t PW_TM = PW_U + kPerCols;     // [128] t_m
constexpr int64_t PW_S = PW_TM + kPerCols;     // [nb] S_b, then [nb] C_b, nb = ceil(capacity / 256)
PHILOX_HD int64_t per_blocks(int64_t slots) { return (slots + kPerBlock - 1) / kPerBlock; }
PHILOX_HD int64_t per_ws_floats(int64_t capacity) { return (PW_S + 2 * per_blocks(capacity) + 3) / 4 * 4; }

PHILOX_HD bool per_fresh(int64_t i, int64_t fresh_pos, int64_t fresh_count, int64_t capacity)
{
    if (fresh_count >= capacity) return true;
    int64_t d = i - fresh_pos;
    if (d < 0) d += capacity;
    return d < fresh_count;
}
PHILOX_HD bool per_fresh32(int i, int fresh_pos, int fresh_count, int capacity)        // the same predicate on 32-bit slots
{
    int d = i - fresh_pos;
    d = d < 0 ? d + capacity : d;
    return fresh_count >= capacity || d < fresh_count;
}
PHILOX_HD float per_block_sum(float s0, float s1, float s2, float s3) { return ((s0 + s1) + s2) + s3; }

PHILOX_HD float per_u(uint64_t seed, uint32_t tick, int m)
{
    const u32x4 x = philox4x32_10((uint32_t)(m >> 2), 0u, tick, (uint32_t)kStreamPer, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t w = (m & 3) == 0 ? x.x : (m & 3) == 1 ? x.y : (m & 3) == 2 ? x.z : x.w;
    return u01_24(w);
}
// t_m = (m + u_m) * (T / batch): three roundings, none fused (there is no multiply feeding an add here; the pragma keeps it so).
PHILOX_HD float per_target(int m, float u, float T, int batch)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = (float)m + u;
    const float seg = T / (float)batch;
    return a * seg;
}
// raw importance weight of a drawn slot
PHILOX_HD float per_raw_weight(int64_t ring_len, float pi, float T, float beta)
{
    if (beta == 0.0f || !(T > 0.0f) || !(pi > 0.0f)) return 1.0f;
    const float x = ((float)ring_len * pi) / T;
    return powf(x, -beta);
}
// new priority of a drawn slot
PHILOX_HD float per_priority(float diff, float eps_p, float alpha) { return powf(fabsf(diff) + eps_p, alpha); }

// The in-block search (step 3).  `at(j)` returns pi_j for an absolute slot j < ring_len.  (Every load is clamped and unconditional,
// and fetched 32 at a time ahead of the adds, so that a device caller has 32 independent loads in flight per round.)
template <class At>
PHILOX_HD int per_search_block(int b, float base, float t, int ring_len, At at)       // (32-bit slots: kPerMaxSlots bounds the ring)
{
    float r = base;
    int hit = -1, cand = -1;
    const int j0 = b * kPerBlock;
    for (int c = 0; c < kPerBlock && hit < 0; c += 32) {           // (a found slot ends the search: nothing behind it can change it)
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int j = j0 + c + i;
            v[i] = at(j < ring_len ? j : ring_len - 1);
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int j = j0 + c + i;
            const float p = j < ring_len ? v[i] : 0.0f;
            r = r + p;
            if (hit < 0 && r > t) hit = j;
            if (p > 0.0f) cand = j;
        }
    }
    int out = hit >= 0 ? hit : cand >= 0 ? cand : j0 + kPerBlock - 1;
    if (out > ring_len - 1) out = ring_len - 1;
    return out;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the whole sampler on the host (the hostcheck's and any CPU caller's): steps 1-4 over host arrays ----
inline float per_chunk_sum_host(const float *x /*64 values*/)
{
    float v[kPerChunk];
    for (int i = 0; i < kPerChunk; ++i) v[i] = x[i];
    for (int n = kPerChunk; n > 1; n >>= 1)
        for (int i = 0; i < n / 2; ++i) v[i] = v[2 * i] + v[2 * i + 1];
    return v[0];
}
struct PerDrawHost { float T; int64_t nb; };
// prio [capacity] is updated in place (fresh slots); S, C [per_blocks(ring_len)]; idx, w, u, tm [128].
inline PerDrawHost per_sample_host(float *prio, float pmax, int64_t capacity, int64_t ring_len, int64_t fresh_pos, int64_t fresh_count,
                                   uint64_t seed, uint32_t tick, int batch, float beta, float *S, float *C, int32_t *idx, float *w,
                                   float *u, float *tm)
{
    for (int64_t i = 0; i < ring_len; ++i)
        if (per_fresh(i, fresh_pos, fresh_count, capacity)) prio[i] = pmax;
    const int64_t nb = per_blocks(ring_len);
    float run = 0.0f;
    int64_t lastpos = 0;
    for (int64_t b = 0; b < nb; ++b) {
        float s[4];
        for (int k = 0; k < 4; ++k) {
            float x[kPerChunk];
            for (int i = 0; i < kPerChunk; ++i) {
                const int64_t j = b * kPerBlock + k * kPerChunk + i;
                x[i] = j < ring_len ? prio[j] : 0.0f;
            }
            s[k] = per_chunk_sum_host(x);
        }
        S[b] = per_block_sum(s[0], s[1], s[2], s[3]);
        run = b == 0 ? S[0] : run + S[b];
        C[b] = run;
        if (S[b] > 0.0f) lastpos = b;
    }
    const float T = C[nb - 1];
    float raw[kPerCols], mx = 0.0f;
    for (int m = 0; m < kPerCols; ++m) {
        u[m] = per_u(seed, tick, m);
        tm[m] = per_target(m, u[m], T, batch);
        int64_t b = -1;
        for (int64_t q = 0; q < nb; ++q)
            if (C[q] > tm[m]) { b = q; break; }
        if (b < 0) b = lastpos;
        const int j = per_search_block((int)b, b > 0 ? C[b - 1] : 0.0f, tm[m], (int)ring_len, [&](int q) { return prio[q]; });
        raw[m] = per_raw_weight(ring_len, prio[j], T, beta);
        idx[m] = m < batch ? (int32_t)j : -1;
        if (m < batch && raw[m] > mx) mx = raw[m];
    }
    for (int m = 0; m < kPerCols; ++m) w[m] = m < batch ? raw[m] / mx : 0.0f;
    return PerDrawHost{T, nb};
}
#endif

}  // namespace shems

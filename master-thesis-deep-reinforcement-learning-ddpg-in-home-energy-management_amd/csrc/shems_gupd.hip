// shems_gupd.hip -- replay() (DDPG.jl:121-145) for a GROUP of independent learners, throughput form.
//
// The thesis protocol trains 40 seeds x 10 chargers = 400 independent learners (RL-SHEMS_bs_scheduler_1179_08_on_01-98.sh:67-87).
// shems_ddpg.hip's five launches are shaped for ONE learner's latency (one exposed memory latency per launch, 1-2 workgroups per
// CU, E-product identities that trade FLOPs and 3 MB of slabs per learner for fewer grid-wide dependencies).  With hundreds of
// learners per launch nothing is latency-bound any more: per learner the update is 308 MFLOP (ten 250x500x128 products) against
// ~11 MB of parameter / moment traffic, i.e. ~2 us at the fp32 MFMA peak and ~1.6 us at 6.3 TB/s -- both roofs within a factor
// of two of each other.  This file is the same arithmetic laid out for that regime:
//
//   * plain back-propagation (no E slabs): per learner ten products, every one a stream of 32-deep weight chunks through a small
//     LDS ring against operands that live in REGISTERS in the MFMA layout (layer 1 is recomputed per chunk on the matrix pipe --
//     K = 12 -- and its D layout IS the next product's B operand; error signals are loaded from HBM straight into operand layout);
//   * 30-47 KB of LDS and 94-143 VGPRs per workgroup: 3-4 workgroups (12-16 waves) resident per CU, so one workgroup's barrier / global
//     latency is covered by the others' MFMAs;
//   * loads retire in order (s_waitcnt vmcnt counts from the oldest): every kernel issues LAST what it will wait for last -- the next
//     weight chunk is never waited for inside the chunk that requested it, the W2 tile's ADAM state is requested after every small operand
//     and arrives under the product (what this cost before it was looked for in the ISA: profiles/NOTES.md, round-5 log);
//   * activations that must cross a launch (relu(layer 2) of the two differentiated networks, 256 KB each) are written once and
//     read from L2 / Infinity Cache; layer-1 activations are never stored; gradients are never stored (ADAM + the soft target
//     update are applied by the lane that holds the finished element; SHEMS_TP_STORE_GRAD keeps the gradient for the tests).
//
// Launches (grid y = learner; all learners advance in lockstep, sharing the ADAM scalars):
//   P0 k_tp_prep   sample (StatsBase.sample with replacement, MPS:33) + gather + normalize (MPS:56); frozen layer-1 images of the
//                  four networks and frozen output layers (the in-place updates below must not be read half-way)
//   P1 k_tp_fwd    actor_target(s') | critic(s, a) | actor(s)                                      (DDPG.jl:131, 114-119)
//   P2 k_tp_fwd    critic_target(s', a')                                                           (DDPG.jl:132)
//   P3 k_tp_d1     y, dq = d mse / dq; D1 = mask1 .* (W2 D2); layer-1 gradient + ADAM (+ the updated layer-1 image P5 reads); b3   (DDPG.jl:133-137)
//   P4 k_tp_gw2    gW2 = h1 D2' + ADAM + soft update per tile; gb2, gW3 + ADAM
//   P5 k_tp_fwd<QG> updated critic on [s; actor(s)], forward and input gradient per n-tile          (DDPG.jl:117-119, 140)
//   P6 k_tp_d1     actor: through tanh, D1, layer-1 gradient + ADAM
//   P7 k_tp_gw2    actor: gW2 + ADAM + soft update, gb2, gW3                                        (DDPG.jl:140-143)
// Two subsets of these launches are updates of their own (behind the kernels above): the grouped SUPERVISED update
// (shems_ddpg_group_clone_update_tp: a sampler with a ring stride of its own, P1 with the actor(s) job alone, P6 with the cloning head
// chosen at compile time, P7) and the grouped CRITIC-ONLY update (shems_ddpg_group_critic_update_tp: that sampler, P1 without the
// actor(s) job, P2, P3, P4 -- the bits of the critic half of the sequence above).
// TD3 for groups (shems_td3_group_update_tp) is a second critic walked by the same kernels: a sampler of its own
// (k_tp_prep_td3), P1, a forward launch whose target jobs smooth the action (k_tp_fwd_smooth), P3 with the twin head and P4 once per
// critic (k_tp_d1_twin, k_tp_gw2), and on a policy step P5-P7 -- seven launches, ten on a policy step (the block in front of k_tp_prep_td3).
// Prioritized replay for groups (shems_ddpg_group_update_per_tp) is a sampler launch S, then P0 .. P7 with a sampler that
// gathers S's slots (k_tp_prep_per) and the weighted head in P3 (k_tp_d1_per).
// On the host (the end of this file) all of these are one launch plan: the shared checks, the launch context, the forward jobs, the
// records and the launch shape of every phase are written once, and an entry point is its own checks plus a sequence of phase calls.
// Summation orders differ from the latency form (64-wide n-tiles, chunked contractions): per learner the results agree with it to
// fp32 accumulation accuracy, not bit for bit -- the parity test holds every gradient block of every learner to the float64
// evaluation with the same bound as the latency form (tests/test_group_gpu.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <type_traits>

#include "philox.h"
#include "shems_adam.h"
#include "shems_internal.h"
#include "shems_per_core.h"
#include "shems_td3_core.h"

namespace shems {
namespace tp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BP = 128;
constexpr int H1N = SHEMS_L1, H2N = SHEMS_L2;
constexpr int SIN = 9, CIN = 11;
constexpr int NT = 8;              // n-tiles of 64 over the 500 (512) layer-2 units
constexpr int W1K = 12, W1C = 256; // layer-1 image: rows 0..in-1 = W1, row 11 = b1, everything else zero; columns >= 250 zero

__host__ __device__ constexpr int off_b1(int in) { return in * H1N; }
__host__ __device__ constexpr int off_w2(int in) { return in * H1N + H1N; }
__host__ __device__ constexpr int off_b2(int in) { return off_w2(in) + H1N * H2N; }
__host__ __device__ constexpr int off_w3(int in) { return off_b2(in) + H2N; }
__host__ __device__ constexpr int off_b3(int in, int out) { return off_w3(in) + H2N * out; }

// ---- TILED working layout of a network's layer-2 state (shems_group_w2t; round 6) ----------------------------------------------
// W2 [250][500], its two ADAM moments and its target as 4 x 8 tiles of 64 x 64 (rows / columns padded to 256 / 512 with zeros), the four
// arrays of a tile ADJACENT: region [kt][nt][m | v | p | target][64 rows][64 columns], 64 KB per tile, 2 MB per network.  P4 / P7 read and
// write one tile's 64 KB as ONE contiguous piece (tools/micro/adam_stream.hip: 4.78 TB/s against 3.85 TB/s for the 256-byte row pieces
// of the Flux order and 4.56 TB/s for a device copy of the same bytes); the forward / D1 launches find a 32-row chunk of a 64-wide n-tile
// as one contiguous 8 KB piece.  The Flux-order blocks keep every other parameter (layer 1, b2, W3, b3) and are the API's view of W2:
// shems_group_w2_to_tiled / _to_flux convert (csrc below), group.py keeps track of which copy is current.
constexpr int TL_TILE = 64 * 64;                   // floats of one array of one tile
constexpr int TL_BLOCK = 4 * TL_TILE;              // one tile: m | v | p | target
enum { TL_M = 0, TL_V = 1, TL_P = 2, TL_T = 3 };
static_assert(SHEMS_W2T_FLOATS == 32 * TL_BLOCK, "shems_hip.h and the kernels agree on the tiled region's size");
__host__ __device__ constexpr int64_t tl_tile(int kt, int nt) { return (int64_t)(kt * 8 + nt) * TL_BLOCK; }

// ---- workspace carve (floats, inside shems_ddpg.ws; see kTpWsFloats) -----------------------------------------------------------
constexpr int64_t TP_X = 0;                            // [12][BP]  rows 0..8 normalize(s), 9..10 stored action, 11 = 1
constexpr int64_t TP_X2 = TP_X + W1K * BP;             // [12][BP]  rows 0..8 normalize(s'), 9..10 zero, 11 = 1
constexpr int64_t TP_R = TP_X2 + W1K * BP;             // [BP]
constexpr int64_t TP_DONE = TP_R + BP;                 // [BP]
constexpr int64_t TP_IDX = TP_DONE + BP;               // [BP] int32 sampled ring slots (-1 in the pad columns)
constexpr int64_t TP_W1I = TP_IDX + BP;                // [5][12][256] frozen layer-1 images of the four networks + the critic's AFTER its update
constexpr int64_t TP_FW3C = TP_W1I + 5 * W1K * W1C;    // [512][2] frozen critic W3 ([.][1] and rows >= 500 zero)
constexpr int64_t TP_FW3A = TP_FW3C + 1024;            // [512][2] frozen actor W3
constexpr int64_t TP_FB3 = TP_FW3A + 1024;             // [8] frozen b3: critic, critic_target, actor[0], actor[1], actor_target[0], [1]
constexpr int64_t TP_P3 = TP_FB3 + 8;                  // [5 passes][NT][2][BP] layer-3 partial sums per n-tile
constexpr int64_t TP_DAP = TP_P3 + 5 * NT * 2 * BP;    // [NT][2][BP] partial d loss / d a_pi per n-tile (P5)
constexpr int64_t TP_D3C = TP_DAP + NT * 2 * BP;       // [2][BP] dq (row 1 zero)
constexpr int64_t TP_D3A = TP_D3C + 2 * BP;            // [2][BP] error at the actor's pre-tanh output
constexpr int64_t TP_API = TP_D3A + 2 * BP;            // [2][BP] a_pi = actor(s)
constexpr int64_t TP_H2C = TP_API + 2 * BP;            // [512][BP] relu(layer 2) of the critic (rows >= 500 zero)
constexpr int64_t TP_H2A = TP_H2C + 512 * BP;          // [512][BP] ... of the actor
constexpr int64_t TP_FLOATS = TP_H2A + 512 * BP;
static_assert(TP_FLOATS <= kTpWsFloats, "the throughput form's carve fits the workspace every caller allocates");
static_assert(TP_W1I % 4 == 0 && TP_H2C % 4 == 0 && TP_P3 % 4 == 0, "16-byte aligned blocks");
enum { NET_ACTOR_T = 0, NET_CRITIC_T = 1, NET_CRITIC = 2, NET_ACTOR = 3, PASS_CRITIC2 = 4 };
constexpr int IMG_CRITIC_NEW = 4;      // image slot P3 fills with the critic's updated layer 1 (P5 reads it; P3 / P4 keep reading the frozen one)
__host__ __device__ inline float *p3_of(float *ws, int pass) { return ws + TP_P3 + (int64_t)pass * NT * 2 * BP; }
__host__ __device__ inline float *w1i_of(float *ws, int net) { return ws + TP_W1I + (int64_t)net * W1K * W1C; }

// rows of a 32 x 32 MFMA accumulator held by register r of a lane in half lh
__device__ __forceinline__ int drow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

__device__ __forceinline__ float half_sum32(float x)      // sum over the 32 lanes of a half wave, in every lane of that half
{
    x += __shfl_xor(x, 1, 64); x += __shfl_xor(x, 2, 64); x += __shfl_xor(x, 4, 64); x += __shfl_xor(x, 8, 64); x += __shfl_xor(x, 16, 64);
    return x;
}
__device__ __forceinline__ float wave_sum64(float x) { x = half_sum32(x); return x + __shfl_xor(x, 32, 64); }

// ---- per-learner hyper-parameters (shems_group_hparams; the *_hp kernels below) ---------------------------------------------------
// A record is read whole by the workgroups of its learner (uniform: scalar loads).  batch is clamped to 1..BP whatever the record holds,
// so that no kernel indexes outside its tiles even if a record was overwritten after the host check.
__device__ __forceinline__ int hp_batch(const shems_group_hparams &h) { return min(max((int)h.batch, 1), BP); }
// learner l's ADAM scalars and soft-update rate in the shared context: k1 = eta_l / (1 - bp1), the correctly rounded Float64 quotient
// the host forms for the shared entry points (a true division, not a reciprocal: the bits must be the host's)
__device__ __forceinline__ void hp_adam(AdamCtx &c, const shems_group_hparams &h, bool critic)
{
    c.eta = critic ? h.eta_crit : h.eta_act;
    c.k1 = c.eta / (1.0 - c.bp1);
    c.tau = h.tau;
}

// a workgroup-uniform double moved into scalar registers (the same bits)
__device__ __forceinline__ double uniform_f64(double x)
{
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ void adam_at(const AdamCtx &c, int i, float g, bool store_grad)
{
    float m = c.mt[i], v = c.vt[i], p = c.p[i], t = c.target[i];
    adam_math(c, g, m, v, p, t);
    c.mt[i] = m; c.vt[i] = v; c.p[i] = p; c.target[i] = t;
    if (store_grad) const_cast<float *>(c.g)[i] = g;
}

// ================================================================================================================================
// P0: sample + gather + normalize; frozen images
// ================================================================================================================================
struct PrepArgs {
    shems_ddpg d;
    shems_replay ring;
    int64_t ring_len, gstride;
    uint64_t seed;
    uint32_t tick;
};
__device__ __forceinline__ void gshift(shems_ddpg &d, int64_t off)
{
    d.actor = gsh(d.actor, off); d.critic = gsh(d.critic, off); d.actor_t = gsh(d.actor_t, off); d.critic_t = gsh(d.critic_t, off);
    d.m_actor = gsh(d.m_actor, off); d.v_actor = gsh(d.v_actor, off); d.m_critic = gsh(d.m_critic, off); d.v_critic = gsh(d.v_critic, off);
    d.grad_actor = gsh(d.grad_actor, off); d.grad_critic = gsh(d.grad_critic, off);
    d.s_min = gsh(d.s_min, off); d.s_max = gsh(d.s_max, off); d.ws = gsh(d.ws, off); d.losses = gsh(d.losses, off);
}
__device__ __forceinline__ void gshift(shems_replay &r, int64_t off)
{
    r.s = gsh(r.s, off); r.a = gsh(r.a, off); r.r = gsh(r.r, off); r.s2 = gsh(r.s2, off); r.done = gsh(r.done, off);
}

// grid (5, learners): workgroup 0 samples / gathers / normalises and freezes the output layers, workgroups 1..4 pack one network's
// frozen layer-1 image each (one launch of 2 000 short workgroups instead of 400 long ones: 49 -> ~10 us at 400 learners)
// XP (shems_ddpg_group_update_tp_x): learner l's ring length is min(pushed[l], xp[l].mem_size) in place of A.ring_len
// PER (shems_ddpg_group_update_per_tp): column m's slot is the one published in learner l's sampler workspace (pws: learner 0's, PW_IDX;
// -1 in the pad columns, which gather slot 0 and store zeros / -1 as ever) in place of the Philox draw
template <bool HP, bool XP = false, bool PER = false>
__device__ __forceinline__ void prep_body(const PrepArgs &A, const int role, const int l, const shems_group_hparams *hp,
                                          const shems_group_xparams *xp = nullptr, const int64_t *pushed = nullptr, const float *pws = nullptr)
{
    const int tid = threadIdx.x;
    const int64_t off = (int64_t)l * A.gstride;
    shems_ddpg d = A.d;
    shems_replay ring = A.ring;
    gshift(d, off); gshift(ring, off);
    float *ws = d.ws;
    if (role > 0) {
        const int net = role - 1;
        const float *P = net == NET_ACTOR_T ? d.actor_t : net == NET_CRITIC_T ? d.critic_t : net == NET_CRITIC ? d.critic : d.actor;
        const int in = (net == NET_CRITIC_T || net == NET_CRITIC) ? CIN : SIN;
        float *img = w1i_of(ws, net);
        const int k = min(tid, H1N - 1);
        float v[W1K];
#pragma unroll
        for (int j = 0; j < W1K; ++j) v[j] = P[(j == W1K - 1 ? in : min(j, in - 1)) * H1N + k];       // clamped, all twelve loads in flight
#pragma unroll
        for (int j = 0; j < W1K; ++j) img[j * W1C + tid] = ((j < in || j == W1K - 1) && tid < H1N) ? v[j] : 0.0f;
        if (net == NET_CRITIC) {                 // the zeros of the slot P3 writes the updated elements into
            float *img2 = w1i_of(ws, IMG_CRITIC_NEW);
#pragma unroll
            for (int j = 0; j < W1K; ++j) img2[j * W1C + tid] = 0.0f;
        }
        return;
    }
    if constexpr (HP) d.batch = hp_batch(hp[l]);              // the first batch_l draws of the same stream are live
    const uint64_t seed = A.seed + (uint64_t)l;               // learner l: Philox key seed + l (as the latency form)
    int64_t ring_len = A.ring_len;
    if constexpr (XP)                                         // clamped to 1..capacity: no division by zero, no slot outside the arrays
        ring_len = min(max(min(pushed[l], (int64_t)xp[l].mem_size), (int64_t)1), ring.capacity);
    if (tid < BP) {
        const int m = tid;
        int64_t j;
        if constexpr (PER) {                     // clamped into the filled slots whatever the workspace holds
            j = min(max((int64_t)reinterpret_cast<const int32_t *>(gsh(pws, off) + PW_IDX)[m], (int64_t)0), ring_len - 1);
        } else {
            const u32x4 x = philox4x32_10((uint32_t)(m >> 2), 0u, A.tick, kStreamSample, (uint32_t)seed, (uint32_t)(seed >> 32));
            const uint32_t w = (m & 3) == 0 ? x.x : (m & 3) == 1 ? x.y : (m & 3) == 2 ? x.z : x.w;
            j = (int64_t)(w % (uint32_t)ring_len);
        }
        const bool live = m < d.batch;
        float sv[SIN], s2v[SIN], lo[SIN], hi[SIN];
#pragma unroll
        for (int k = 0; k < SIN; ++k) { sv[k] = ring.s[j * SIN + k]; s2v[k] = ring.s2[j * SIN + k]; lo[k] = d.s_min[k]; hi[k] = d.s_max[k]; }
        const float a0 = ring.a[j * 2], a1 = ring.a[j * 2 + 1], rr = ring.r[j];
        const bool dn = ring.done[j] != 0;
#pragma unroll
        for (int k = 0; k < SIN; ++k) {
            const float den = (hi[k] - lo[k]) + 1e-8f;                                     // MPS:56
            ws[TP_X + k * BP + m] = live ? (sv[k] - lo[k]) / den : 0.0f;
            ws[TP_X2 + k * BP + m] = live ? (s2v[k] - lo[k]) / den : 0.0f;
        }
        ws[TP_X + 9 * BP + m] = live ? a0 : 0.0f;
        ws[TP_X + 10 * BP + m] = live ? a1 : 0.0f;
        ws[TP_X + 11 * BP + m] = 1.0f;
        ws[TP_X2 + 9 * BP + m] = 0.0f; ws[TP_X2 + 10 * BP + m] = 0.0f; ws[TP_X2 + 11 * BP + m] = 1.0f;
        ws[TP_R + m] = live ? rr : 0.0f;
        ws[TP_DONE + m] = live && dn ? 1.0f : 0.0f;
        reinterpret_cast<int32_t *>(ws + TP_IDX)[m] = live ? (int32_t)j : -1;
    }
    // frozen output layers
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int e = it * 256 + tid, n = e >> 1, o = e & 1;
        const float wc = d.critic[off_w3(CIN) + min(n, H2N - 1)], wa = d.actor[off_w3(SIN) + min(e, 2 * H2N - 1)];
        ws[TP_FW3C + e] = (n < H2N && o == 0) ? wc : 0.0f;
        ws[TP_FW3A + e] = n < H2N ? wa : 0.0f;
    }
    if (tid < 8)
        ws[TP_FB3 + tid] = tid == 0 ? d.critic[off_b3(CIN, 1)] : tid == 1 ? d.critic_t[off_b3(CIN, 1)]
                         : tid == 2 ? d.actor[off_b3(SIN, 2)] : tid == 3 ? d.actor[off_b3(SIN, 2) + 1]
                         : tid == 4 ? d.actor_t[off_b3(SIN, 2)] : tid == 5 ? d.actor_t[off_b3(SIN, 2) + 1] : 0.0f;
}

// ================================================================================================================================
// P1 / P2 / P5: forward through layers 1 + 2 for one 64-wide n-tile and the whole batch; layer 3 as per-tile partial sums.
// QG (P5): the same workgroup then back-propagates the constant upstream gradient of -mean(q) through its own 64 hidden units.
// ================================================================================================================================
struct FwdJob {
    const float *w2t;      // tiled layout: the network's region + TL_P / TL_T array offset (its W2 is read from there); null: Flux order, from P
    const float *P;        // parameter block of the network
    const float *X;        // [12][BP] input block (workspace)
    const float *w1i;      // layer-1 image (workspace): frozen by P0, or written by P3 (the critic after its update)
    const float *ap3;      // rows 9, 10 = tanh(ab3 + sum of these [NT][2][BP] partials) of an actor pass, or null (rows as stored in X)
    const float *ab3;      // [2]
    float *api;            // n-tile 0 publishes the computed action here ([2][BP]), or null
    float *H2;             // [512][BP] relu(layer 2) (rows >= 500 stored as zero), or null
    float *P3;             // [NT][2][BP]
    float *DAP;            // QG: [NT][2][BP]
    int in, out;
};
struct FwdArgs { FwdJob job[3]; int64_t gstride; int batch; };
__device__ __forceinline__ void gshift(FwdJob &J, int64_t off)
{
    J.w2t = gsh(J.w2t, off); J.P = gsh(J.P, off); J.X = gsh(J.X, off); J.w1i = gsh(J.w1i, off); J.ap3 = gsh(J.ap3, off); J.ab3 = gsh(J.ab3, off);
    J.api = gsh(J.api, off); J.H2 = gsh(J.H2, off); J.P3 = gsh(J.P3, off); J.DAP = gsh(J.DAP, off);
}

// W2 chunk c of an n-tile of NTL MFMA tiles (64 or 128 columns): rows k = 32 c .. 32 c + 31, columns n0 .. (256 / 512 B per row), NTL float4
// per thread.  Rows >= 250 are
// copies of row 249 (clamped address): they only meet layer-1 activations that are exactly zero (the image has no columns >= 250)
// or output rows whose relu mask is off.  Columns >= 500 of the last tile read on into the next row / b2 (inside the parameter
// block) and only feed outputs that are discarded.
template <int NTL>
__device__ __forceinline__ void fwd_chunk_load(const float *__restrict__ W2, int n0, int c, f32x4 (&v)[NTL])
{
#pragma unroll
    for (int it = 0; it < NTL; ++it) {
        const int e = it * 256 + (int)threadIdx.x, k = min(32 * c + e / (8 * NTL), H1N - 1);
        v[it] = *reinterpret_cast<const f32x4 *>(W2 + (int64_t)k * H2N + n0 + 4 * (e % (8 * NTL)));
    }
}
// The same chunk from the tiled layout: per 64 columns the 32 rows are ONE contiguous 8 KB piece (512 float4) of the tile (kt = c / 2,
// rows 32 (c & 1) ..); pad rows / columns hold zeros.  fwd_chunk_store_t puts float4 r of piece j at LDS row r / 16, column 64 j + 4 (r % 16).
template <int NTL>
__device__ __forceinline__ void fwd_chunk_load_t(const float *__restrict__ Wt, int n0, int c, f32x4 (&v)[NTL])
{
    const float *base = Wt + tl_tile(c >> 1, n0 >> 6) + (c & 1) * (32 * 64);
#pragma unroll
    for (int it = 0; it < NTL; ++it) {
        const int e = it * 256 + (int)threadIdx.x;
        v[it] = *reinterpret_cast<const f32x4 *>(base + (int64_t)(e >> 9) * TL_BLOCK + 4 * (e & 511));
    }
}
template <int S, int NTL>
__device__ __forceinline__ void fwd_chunk_store_t(float *buf, const f32x4 (&v)[NTL])
{
#pragma unroll
    for (int it = 0; it < NTL; ++it) {
        const int e = it * 256 + (int)threadIdx.x, r = e & 511;
        float *p = buf + (r >> 4) * S + 64 * (e >> 9) + 4 * (r & 15);
        if constexpr (S % 4 == 0) *reinterpret_cast<f32x4 *>(p) = v[it];
        else { p[0] = v[it][0]; p[1] = v[it][1]; p[2] = v[it][2]; p[3] = v[it][3]; }
    }
}
template <int S, int NTL>
__device__ __forceinline__ void fwd_chunk_store(float *buf, const f32x4 (&v)[NTL])
{
#pragma unroll
    for (int it = 0; it < NTL; ++it) {
        const int e = it * 256 + (int)threadIdx.x;
        float *p = buf + (e / (8 * NTL)) * S + 4 * (e % (8 * NTL));
        if constexpr (S % 4 == 0) *reinterpret_cast<f32x4 *>(p) = v[it];
        else { p[0] = v[it][0]; p[1] = v[it][1]; p[2] = v[it][2]; p[3] = v[it][3]; }
    }
}

// layer-1 pre-activations of hidden units 32 c .. 32 c + 31 x this wave's 32 batch columns, D layout (row = unit, column = sample)
__device__ __forceinline__ f32x16 l1_tile(const float *w1s, int c, const float (&xreg)[6], int li, int lh)
{
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.0f;
    float a[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) a[s] = w1s[(2 * s + lh) * W1C + 32 * c + li];
#pragma unroll
    for (int s = 0; s < 6; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], xreg[s], t, 0, 0, 0);
    return t;
}

// NTL = MFMA tiles per wave along n.  4 = a 128-wide n-tile: layer 1 is recomputed per n-tile, 6 MFMAs per chunk beside 64 instead of
// beside 32 -- taken where the launch still has several rounds of workgroups (P1: three networks x 4 tiles x learners); 2 = 64-wide
// n-tiles, twice the workgroups at four per CU: P2 (one network: 1 600 workgroups of the wide form would be 2.1 rounds of 768 slots)
// and the pass with the input gradient (its second sweep holds 16 more accumulators).
template <bool QG, int NTL_> struct FwdShape {
    static constexpr int NTL = NTL_;
    static constexpr int NW = 32 * NTL;            // n-tile width
    static constexpr int TILES = 512 / NW;         // n-tiles per network
    static constexpr int S = QG ? NW + 1 : NW;     // chunk row stride: the backward pass reads the chunk along n (odd stride: conflict free)
    static constexpr int LDS = (W1K * W1C + NW * 4 + 2 * 32 * S) * 4;
};

// SMOOTH (TD3 for groups, k_tp_fwd_smooth): a job with ap3 takes the SMOOTHED target action a~' = clamp(tanh(..) + eps, -1, 1) into its
// action rows -- the same loads and the same summation of the actor-target partials, then learner `by`'s draw of the target-noise stream
// (key seed + by), the clip and the clamp of shems_td3_core.h.  sigma_trg = 0 leaves the bits of the plain path.
struct TpNoise { uint64_t seed; uint32_t tick; float sigma, clip; };
template <bool QG, int NTL_, bool TL, bool HP, bool SMOOTH = false>
__device__ __forceinline__ void fwd_body(const FwdArgs &A, const int bx, const int by, float *smem, const shems_group_hparams *hp,
                                         const TpNoise *tn = nullptr)
{
    typedef FwdShape<QG, NTL_> SH;
    constexpr int S = SH::S, NTL = SH::NTL, NW = SH::NW;
    float *w1s = smem;                           // [12][256]
    float *ep = w1s + W1K * W1C;                 // [NW][4]: b2, W3[.][0], W3[.][1], valid
    float *ring = ep + NW * 4;                   // [2][32][S]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int job = bx / SH::TILES, nt = bx % SH::TILES, n0 = NW * nt;
    FwdJob J = job == 0 ? A.job[0] : job == 1 ? A.job[1] : A.job[2];
    gshift(J, (int64_t)by * A.gstride);
    const float *__restrict__ P = J.P;
    const float *__restrict__ W2 = TL ? J.w2t : P + off_w2(J.in);
    const int m = 32 * w + li;
    auto chunk_load = [&](int c, f32x4 (&v)[NTL]) {
        if constexpr (TL) fwd_chunk_load_t<NTL>(W2, n0, c, v); else fwd_chunk_load<NTL>(W2, n0, c, v);
    };
    auto chunk_store = [&](float *buf, const f32x4 (&v)[NTL]) {
        if constexpr (TL) fwd_chunk_store_t<S, NTL>(buf, v); else fwd_chunk_store<S, NTL>(buf, v);
    };

    // Every request of the prologue is issued before the first wait: the workgroups of a CU start together (at the launch and, staying
    // in step, after each generation), so their prologues are not covered by anybody's matrix work -- one exposed round trip, not four.
    f32x4 pv[NTL];
    chunk_load(0, pv);
    f32x4 wi[3];
    {
        const f32x4 *g4 = reinterpret_cast<const f32x4 *>(J.w1i) + tid;
        wi[0] = g4[0]; wi[1] = g4[256]; wi[2] = g4[512];
    }
    float eb2 = 0.0f, ew30 = 0.0f, ew31 = 0.0f;
    if (tid < NW) {
        const int nc = min(n0 + tid, H2N - 1);
        eb2 = P[off_b2(J.in) + nc]; ew30 = P[off_w3(J.in) + nc * J.out];
        if (J.out == 2) ew31 = P[off_w3(J.in) + nc * 2 + 1];
    }
    // this lane's B operands of layer 1: x[2 s + lh][m]
    float xreg[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) xreg[s] = J.X[(2 * s + lh) * BP + m];
    float a0 = 0.0f, a1 = 0.0f, pa3[2 * NT];
    if (J.ap3) {
        a0 = J.ab3[0]; a1 = J.ab3[1];
#pragma unroll
        for (int t = 0; t < NT; ++t) { pa3[2 * t] = J.ap3[(t * 2 + 0) * BP + m]; pa3[2 * t + 1] = J.ap3[(t * 2 + 1) * BP + m]; }
    }
    __builtin_amdgcn_sched_barrier(0);
    // layer-1 image -> LDS
    {
        f32x4 *l4 = reinterpret_cast<f32x4 *>(w1s) + tid;
        l4[0] = wi[0]; l4[256] = wi[1]; l4[512] = wi[2];
    }
    if (tid < NW) {
        const float valid = n0 + tid < H2N ? 1.0f : 0.0f;
        ep[tid * 4 + 0] = eb2; ep[tid * 4 + 1] = ew30 * valid; ep[tid * 4 + 2] = ew31 * valid; ep[tid * 4 + 3] = valid;
    }
    if (J.ap3) {                                 // rows 9, 10 from an actor pass: a[o][m] = tanh(b3[o] + partials)
#pragma unroll
        for (int t = 0; t < NT; ++t) { a0 += pa3[2 * t]; a1 += pa3[2 * t + 1]; }
        a0 = tanhf(a0); a1 = tanhf(a1);          // Dense(500, 2, tanh)
        if constexpr (SMOOTH) {                  // column m's block of the learner's own stream; Box-Muller as gauss_pair (shems_policy.hip)
            const u32x4 x = td3_block(tn->seed + (uint64_t)by, tn->tick, (uint32_t)m);
            const float rr = sqrtf(-2.0f * logf(td3_u1(x)));
            float sn, cs;
            sincosf(6.28318530717958647692f * td3_u2(x), &sn, &cs);
            a0 = td3_smooth(a0, td3_eps(tn->sigma, tn->clip, rr * cs));
            a1 = td3_smooth(a1, td3_eps(tn->sigma, tn->clip, rr * sn));
        }
        if (lh == 1) xreg[4] = a0; else xreg[5] = a1;          // row 9 = (s 4, lh 1), row 10 = (s 5, lh 0)
        if (J.api && nt == 0) J.api[lh * BP + m] = lh ? a1 : a0;
    }
    chunk_store(ring, pv);
    // The operands above are consumed inside the chunk loop only.  Loads retire in order, so without this the compiler's wait in front of
    // their first use (counted for the loop's entry edge) also waits, on every later iteration, for the chunk prefetch issued just before it.
#pragma unroll
    for (int s = 0; s < 6; ++s) asm volatile("" : "+v"(xreg[s]));
    __syncthreads();

    f32x16 acc[NTL];
#pragma unroll
    for (int tt = 0; tt < NTL; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tt][r] = 0.0f;
    float da0 = 0.0f, da1 = 0.0f;
    unsigned mbits = 0u;                         // QG: bit 16 tt + r = (h2 > 0) of this lane's element (tt, r)
    const int batch = HP ? hp_batch(hp[by]) : A.batch;
    const float d3q = m < batch ? -1.0f / (float)batch : 0.0f;              // d(-mean q)/dq
    // One pass over the n-tile's eight weight chunks; chunk it + 1 is requested before chunk it is consumed and lands in the other half
    // of the ring.  BWD = false: layer 2 forward; BWD = true (QG only): the input gradient through this n-tile.
    auto pass = [&](auto bwd, int it0, bool wrap) {
        constexpr bool BWD = decltype(bwd)::value;
#pragma unroll 1
        for (int it = it0; it < it0 + 8; ++it) {
            const int c = it & 7;
            const float *buf = ring + (it & 1) * 32 * S;
            const bool more = wrap || c < 7;
            if (more) chunk_load((it + 1) & 7, pv);
            __builtin_amdgcn_sched_barrier(0);          // (where the request is unconditional the scheduler otherwise sinks it to the end of the iteration)
            if constexpr (!BWD) {
                // layer 2: k-step r contracts over the two hidden units {32 c + drow(r, 0), 32 c + drow(r, 1)}; B = relu(t[r]) from registers.
                // The A operands of step r + 1 are read from LDS before the products of step r are issued (read -> wait -> two products, as
                // the compiler lays the plain loop out, leaves the LDS latency uncovered behind every pair: ~3/4 of the pipe for one wave).
                const float *pa = buf + 4 * lh * S + li;
                float a0[NTL], a1[NTL];
#pragma unroll
                for (int tt = 0; tt < NTL; ++tt) a0[tt] = pa[32 * tt];
                const f32x16 t = l1_tile(w1s, c, xreg, li, lh);
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
#pragma unroll
                    for (int tt = 0; tt < NTL; ++tt) a1[tt] = pa[(((r + 1) & 3) + 8 * ((r + 1) >> 2)) * S + 32 * tt];
                    __builtin_amdgcn_sched_barrier(0);
                    const float b0 = fmaxf(t[r], 0.0f);
#pragma unroll
                    for (int tt = 0; tt < NTL; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[tt], b0, acc[tt], 0, 0, 0);
                    if (r < 14) {
#pragma unroll
                        for (int tt = 0; tt < NTL; ++tt) a0[tt] = pa[(((r + 2) & 3) + 8 * ((r + 2) >> 2)) * S + 32 * tt];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const float b1 = fmaxf(t[r + 1], 0.0f);
#pragma unroll
                    for (int tt = 0; tt < NTL; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[tt], b1, acc[tt], 0, 0, 0);
                }
            } else {
                // backward through this n-tile: D1part[k][m] = sum_{n in tile} W2[k][n] M[n][m], rows k = 32 c .. + 31; M[n][m] = d3q[m] W3[n]
                // (h2[n][m] > 0) is rebuilt per k-step from one mask bit and the epilogue block in LDS (32 registers less than keeping it:
                // with those the four-waves budget spilled, and a scratch reload in this loop waits for the chunk prefetch as well)
                f32x16 g;
#pragma unroll
                for (int r = 0; r < 16; ++r) g[r] = 0.0f;
                const float *pa = buf + li * S + 4 * lh;
                const float *pe = ep + 16 * lh + 1;
                // (operands of step i + 1 read before the product of step i is issued, as in the forward pass)
                auto nbof = [](int i) { return 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2); };
                float aA = pa[0], wA = pe[0], aB, wB;
#pragma unroll
                for (int i = 0; i < 16 * NTL; i += 2) {
                    aB = pa[nbof(i + 1)]; wB = pe[nbof(i + 1) * 4];
                    __builtin_amdgcn_sched_barrier(0);
                    g = __builtin_amdgcn_mfma_f32_32x32x2f32(aA, (mbits >> i) & 1u ? wA * d3q : 0.0f, g, 0, 0, 0);
                    if (i + 2 < 16 * NTL) { aA = pa[nbof(i + 2)]; wA = pe[nbof(i + 2) * 4]; }
                    __builtin_amdgcn_sched_barrier(0);
                    g = __builtin_amdgcn_mfma_f32_32x32x2f32(aB, (mbits >> (i + 1)) & 1u ? wB * d3q : 0.0f, g, 0, 0, 0);
                }
                // layer-1 pre-activations for the mask only now: 16 fewer live registers under the product (with them the 128-register
                // budget of four waves per SIMD spilled two of M's values, and a scratch reload waits for the chunk prefetch as well)
                __builtin_amdgcn_sched_barrier(0);
                const f32x16 t = l1_tile(w1s, c, xreg, li, lh);
                const float *pw = w1s + 9 * W1C + 32 * c + 4 * lh;             // W1[9 + o][k]: the action rows (columns >= 250 zero)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = t[r] > 0.0f ? g[r] : 0.0f;                // layer-1 relu mask
                    da0 = fmaf(pw[(r & 3) + 8 * (r >> 2)], v, da0);
                    da1 = fmaf(pw[W1C + (r & 3) + 8 * (r >> 2)], v, da1);
                }
            }
            if (more) chunk_store(ring + ((it + 1) & 1) * 32 * S, pv);
            __syncthreads();
        }
    };
    pass(std::false_type{}, 0, QG);
    // epilogue of the forward pass: bias, relu, store, layer-3 partials; QG: the relu mask of the tile is kept, one bit per element
    auto epilogue = [&](auto keep) {
        constexpr bool KEEP = decltype(keep)::value;
        const float *epl = ep + 16 * lh;
        float *hp = J.H2 + (n0 + 4 * lh) * BP + m;
#pragma unroll
        for (int hf = 0; hf < NTL / 2; ++hf) {                                  // one pair of layer-3 partials per 64 columns: the consumers add
            float p0 = 0.0f, p1 = 0.0f;                                         // NT = 8 of them whatever the tile width
#pragma unroll
            for (int th = 0; th < 2; ++th)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tt = 2 * hf + th;
                    const int nb = 32 * tt + (r & 3) + 8 * (r >> 2);          // + 4 lh = the tile row
                    const f32x4 e = *reinterpret_cast<const f32x4 *>(epl + nb * 4);
                    const float h = fmaxf(acc[tt][r] + e[0], 0.0f) * e[3];
                    if constexpr (KEEP) hp[nb * BP] = h;
                    p0 = fmaf(h, e[1], p0);
                    p1 = fmaf(h, e[2], p1);
                    if (QG && h > 0.0f) mbits |= 1u << (16 * tt + r);
                }
            p0 += __shfl_xor(p0, 32, 64);
            p1 += __shfl_xor(p1, 32, 64);
            const int slot = (NTL / 2) * nt + hf;
            if (lh == 0) { J.P3[(slot * 2 + 0) * BP + m] = p0; J.P3[(slot * 2 + 1) * BP + m] = p1; }
        }
    };
    if (J.H2) epilogue(std::true_type{}); else epilogue(std::false_type{});
    if constexpr (QG) pass(std::true_type{}, 8, false);
    if (QG) {
        da0 += __shfl_xor(da0, 32, 64);
        da1 += __shfl_xor(da1, 32, 64);
        if (lh == 0) { J.DAP[(nt * 2 + 0) * BP + m] = da0; J.DAP[(nt * 2 + 1) * BP + m] = da1; }
    }
}

// ================================================================================================================================
// The network being differentiated (P3 / P4: critic, P6 / P7: actor)
// ================================================================================================================================
struct NetArgs {
    shems_ddpg d;          // learner 0's record (heads, losses, workspace)
    float *w2t;            // tiled layout: the network's region (learner 0's); null: Flux order
    AdamCtx c;
    int64_t gstride;
    int head;              // 1 = critic loss head, 2 = actor head
    int store_grad;
    int learners;
};
template <int IN> struct NetOf {
    static constexpr bool critic = IN == CIN;
    static constexpr int OUT = critic ? 1 : 2;
    __device__ static const float *X(const float *ws) { return ws + TP_X; }
    __device__ static const float *w1i(float *ws) { return w1i_of(ws, critic ? NET_CRITIC : NET_ACTOR); }
    __device__ static const float *w3f(const float *ws) { return ws + (critic ? TP_FW3C : TP_FW3A); }
    __device__ static const float *H2(const float *ws) { return ws + (critic ? TP_H2C : TP_H2A); }
    __device__ static float *d3(float *ws) { return ws + (critic ? TP_D3C : TP_D3A); }
};

// ---- heads: the error signal at the output layer, d3 [2][BP] into LDS (every thread of the workgroup takes part); the publishing
// workgroup also stores it for P4 / P7, reports the loss and applies the b3 gradient ----
__device__ __forceinline__ void head_critic(const NetArgs &A, const shems_ddpg &d, const AdamCtx &c, float *d3s, float *red, bool publisher)
{
    float *ws = d.ws;
    const int t = threadIdx.x, m = t & 127;
    float dq = 0.0f, diff = 0.0f;
    if (t < BP) {
        const float *Pt = p3_of(ws, NET_CRITIC_T), *Pc = p3_of(ws, NET_CRITIC);
        float q2 = ws[TP_FB3 + 1], q = ws[TP_FB3 + 0];
#pragma unroll
        for (int i = 0; i < NT; ++i) { q2 += Pt[(i * 2) * BP + m]; q += Pc[(i * 2) * BP + m]; }
        const float y = ws[TP_R + m] + d.gamma * (1.0f - ws[TP_DONE + m]) * q2;            // DDPG.jl:133
        diff = m < d.batch ? q - y : 0.0f;
        dq = 2.0f * diff / (float)d.batch;                                                  // d mse / d q
    }
    d3s[t] = t < BP ? dq : 0.0f;
    if (publisher) {
        d.ws[TP_D3C + t] = t < BP ? dq : 0.0f;
        const float s1 = wave_sum64(diff * diff), s2 = wave_sum64(dq);
        if ((t & 63) == 0) { red[t >> 6] = s1; red[4 + (t >> 6)] = s2; }
        __syncthreads();
        if (t == 0) {
            d.losses[0] = (red[0] + red[1]) / (float)d.batch;                               // Flux.mse
            adam_at(c, off_b3(CIN, 1), red[4] + red[5], A.store_grad != 0);
        }
    }
}
__device__ __forceinline__ void head_actor(const NetArgs &A, const shems_ddpg &d, const AdamCtx &c, float *d3s, float *red, bool publisher)
{
    float *ws = d.ws;
    const int t = threadIdx.x, o = t >> 7, m = t & 127;
    float da = 0.0f;
#pragma unroll
    for (int p = 0; p < NT; ++p) da += ws[TP_DAP + (int64_t)(p * 2 + o) * BP + m];
    const float a = ws[TP_API + t];
    const float g = da * (1.0f - a * a);                       // through tanh
    d3s[t] = g;
    if (publisher) {
        ws[TP_D3A + t] = g;
        float q = 0.0f;
        if (o == 0 && m < d.batch) {
            const float *Pq = p3_of(ws, PASS_CRITIC2);
            q = d.critic[off_b3(CIN, 1)];
#pragma unroll
            for (int i = 0; i < NT; ++i) q += Pq[(i * 2) * BP + m];
        }
        const float sg = wave_sum64(g), sq = wave_sum64(q);
        if ((t & 63) == 0) { red[t >> 6] = sg; red[4 + (t >> 6)] = sq; }
        __syncthreads();
        if (t == 0) {
            d.losses[1] = -(red[4] + red[5]) / (float)d.batch;     // loss_act = -mean(critic(vcat(s, actor(s))))
            adam_at(c, off_b3(SIN, 2), red[0] + red[1], A.store_grad != 0);
            adam_at(c, off_b3(SIN, 2) + 1, red[2] + red[3], A.store_grad != 0);
        }
    }
}
// The cloning head (shems_ddpg_group_clone_update_tp): loss = Flux.mse(actor(normalize(s)), a_demo), the mean over the 2 * batch
// elements.  a_pi = tanh(b3 + the NT layer-3 partials of the actor pass), the frozen b3 first and the partials in ascending n-tile order
// (the order in which fwd_body forms an actor pass's action); d3[o][m] = (a_pi - a_demo)(1 - a_pi^2) / batch, 0 in the pad columns.
// a_demo [2][BP] lies where the full sampler keeps r and done (TP_ADEMO).  The loss sums in ONE order: per wave of 64 lanes the butterfly
// of wave_sum64 over its 64 squared differences, then ((w0 + w1) + w2) + w3 with waves 0, 1 = output 0 (columns 0..63, 64..127) and
// waves 2, 3 = output 1, divided by float(2 batch).
constexpr int64_t TP_ADEMO = TP_R;
static_assert(TP_DONE == TP_R + BP, "a_demo [2][BP] takes the r and done rows of the full sampler");
__device__ __forceinline__ void head_clone(const NetArgs &A, const shems_ddpg &d, const AdamCtx &c, float *d3s, float *red, bool publisher)
{
    float *ws = d.ws;
    const int t = threadIdx.x, o = t >> 7, m = t & 127;
    const float *Pa = p3_of(ws, NET_ACTOR);
    float z = ws[TP_FB3 + 2 + o];
#pragma unroll
    for (int i = 0; i < NT; ++i) z += Pa[(i * 2 + o) * BP + m];
    const float a = tanhf(z);                                  // Dense(500, 2, tanh)
    const float diff = m < d.batch ? a - ws[TP_ADEMO + t] : 0.0f;
    const float g = diff * (1.0f - a * a) / (float)d.batch;    // d mse / d a_pi = (a_pi - a_demo) / batch, through tanh
    d3s[t] = g;
    if (publisher) {
        ws[TP_D3A + t] = g;
        const float sl = wave_sum64(diff * diff), sg = wave_sum64(g);
        if ((t & 63) == 0) { red[t >> 6] = sl; red[4 + (t >> 6)] = sg; }
        __syncthreads();
        if (t == 0) {
            d.losses[1] = (((red[0] + red[1]) + red[2]) + red[3]) / (float)(2 * d.batch);
            adam_at(c, off_b3(SIN, 2), red[4] + red[5], A.store_grad != 0);
            adam_at(c, off_b3(SIN, 2) + 1, red[6] + red[7], A.store_grad != 0);
        }
    }
}

// The twin head (shems_td3_group_update_tp, k_tp_d1_twin): head_critic with TD3's target.  Both target critics' layer-3 partials and
// frozen b3 give q'1 (critic 1's workspace) and q'2 (critic 2's), td3_min and td3_y give the one y of both critics; the differentiated
// critic's own q, dq, loss and b3 gradient are head_critic's, in head_critic's summation orders (equal target critics leave its bits).
// The publishing workgroup also stores y, q'1, q'2 [3][BP] at `pub`.  d.ws is the DIFFERENTIATED critic's workspace (critic 2: ws2, which
// mirrors the carve where NetOf<CIN> points); r and done are read from critic 1's.
struct TwinX { const float *ws1, *ws2; float *pub; };
// td3_y's expression (shems_td3_core.h) with head_critic's rounding.  In every instantiation of d1_body the compiler forms head_critic's
// y = r + gamma (1 - done) q' as a rounded product and an add (it pairs that add with the last add of q into one packed add, so no fused
// multiply-add appears; read in the ISA of all sixteen k_tp_d1 / k_tp_d1_hp kernels), while td3_y inlined beside the twin minimum is
// contracted into one.  The degenerate case (sigma_trg = 0, equal critics) must leave head_critic's bits, so the contraction is pinned
// off here: this is also the arithmetic of the host check of shems_td3_core.h (-ffp-contract=off) and of tests/td3_ref.py.
__device__ __forceinline__ float td3_y_rounded(float r, float gamma, float done, float qmin)
{
#pragma clang fp contract(off)
    return r + gamma * (1.0f - done) * qmin;
}
__device__ __forceinline__ void head_twin(const NetArgs &A, const shems_ddpg &d, const AdamCtx &c, float *d3s, float *red, bool publisher,
                                          const TwinX &X, const int64_t off)
{
    const float *ws = d.ws, *w1 = gsh(X.ws1, off), *w2 = gsh(X.ws2, off);
    float *pub = gsh(X.pub, off);
    const int t = threadIdx.x, m = t & 127;
    float dq = 0.0f, diff = 0.0f;
    if (t < BP) {
        const float *Pt1 = w1 + TP_P3 + (int64_t)NET_CRITIC_T * NT * 2 * BP, *Pt2 = w2 + TP_P3 + (int64_t)NET_CRITIC_T * NT * 2 * BP;
        const float *Pc = ws + TP_P3 + (int64_t)NET_CRITIC * NT * 2 * BP;
        float q1 = w1[TP_FB3 + 1], q2 = w2[TP_FB3 + 1], q = ws[TP_FB3 + 0];
#pragma unroll
        for (int i = 0; i < NT; ++i) { q1 += Pt1[(i * 2) * BP + m]; q2 += Pt2[(i * 2) * BP + m]; q += Pc[(i * 2) * BP + m]; }
        const float y = td3_y_rounded(w1[TP_R + m], d.gamma, w1[TP_DONE + m], td3_min(q1, q2));
        diff = m < d.batch ? q - y : 0.0f;
        dq = 2.0f * diff / (float)d.batch;                                                  // d mse / d q
        if (publisher) { pub[m] = y; pub[BP + m] = q1; pub[2 * BP + m] = q2; }
    }
    d3s[t] = t < BP ? dq : 0.0f;
    if (publisher) {
        d.ws[TP_D3C + t] = t < BP ? dq : 0.0f;
        const float s1 = wave_sum64(diff * diff), s2 = wave_sum64(dq);
        if ((t & 63) == 0) { red[t >> 6] = s1; red[4 + (t >> 6)] = s2; }
        __syncthreads();
        if (t == 0) {
            d.losses[0] = (red[0] + red[1]) / (float)d.batch;                               // Flux.mse
            adam_at(c, off_b3(CIN, 1), red[4] + red[5], A.store_grad != 0);
        }
    }
}

// The weighted head of prioritized replay (shems_ddpg_group_update_per_tp, k_tp_d1_per; shems_per_core.h steps 5 and 6): head_critic with
// dq = 2 w diff / B and losses[0] = sum (w diff) diff / B in head_critic's summation orders, the importance weights w [BP] read by every
// workgroup of the learner from its sampler workspace (PW_W; 0 in the pad columns).  Weights of 1.0 leave head_critic's bits: y is
// head_critic's rounded product and add (pinned, as td3_y_rounded), 2 * 1 * diff and (1 * diff) * diff are head_critic's operands.
// The publishing workgroup also writes the drawn slots' new priorities back when X.prio is set: pi = (|diff| + eps_p)^alpha, ONE writer
// per slot -- the highest live column that drew it, decided over the 128 slots in LDS (scr: the weight ring, not yet filled) -- and
// pmax = max(pmax, every new pi).  Slots are clamped into [0, ring_len) before they index anything.  It also publishes y and q [2][BP]
// at ws + TP_PERQ (diff = q - y is what the priorities are formed from).
constexpr int64_t TP_PERQ = TP_FLOATS;            // [2][BP] y, q of the weighted head (behind the carve above: no other launch touches it)
static_assert(TP_PERQ == SHEMS_TP_PER_PUB && TP_PERQ % 4 == 0 && TP_PERQ + 2 * BP <= kTpWsFloats, "shems_hip.h names where y and q are published");
struct PerX {
    const float *pw;                   // learner 0's sampler workspace (PW_IDX, PW_W)
    float *prio, *pmax;                // learner 0's write-back targets, or null: no write-back (SHEMS_TP_PER_GIVEN)
    int64_t ring_len;
    float alpha, eps_p;
};
__device__ __forceinline__ float per_y_rounded(float r, float gamma, float done, float q2)
{
#pragma clang fp contract(off)
    return r + gamma * (1.0f - done) * q2;
}
__device__ __forceinline__ void head_critic_per(const NetArgs &A, const shems_ddpg &d, const AdamCtx &c, float *d3s, float *red, bool publisher,
                                                const PerX &X, const int64_t off, float *scr /*LDS, >= BP + 2 words*/)
{
    float *ws = d.ws;
    const float *pw = gsh(X.pw, off);
    const int t = threadIdx.x, m = t & 127;
    float dq = 0.0f, diff = 0.0f, wm = 0.0f;
    if (t < BP) {
        const float *Pt = p3_of(ws, NET_CRITIC_T), *Pc = p3_of(ws, NET_CRITIC);
        float q2 = ws[TP_FB3 + 1], q = ws[TP_FB3 + 0];
        wm = pw[PW_W + m];
#pragma unroll
        for (int i = 0; i < NT; ++i) { q2 += Pt[(i * 2) * BP + m]; q += Pc[(i * 2) * BP + m]; }
        const float y = per_y_rounded(ws[TP_R + m], d.gamma, ws[TP_DONE + m], q2);           // DDPG.jl:133
        diff = m < d.batch ? q - y : 0.0f;
        dq = 2.0f * wm * diff / (float)d.batch;                                             // d (sum w diff^2 / B) / d q
        if (publisher) { ws[TP_PERQ + m] = y; ws[TP_PERQ + BP + m] = q; }
    }
    d3s[t] = t < BP ? dq : 0.0f;
    if (publisher) {
        d.ws[TP_D3C + t] = t < BP ? dq : 0.0f;
        const bool wb = X.prio != nullptr, live = t < BP && m < d.batch;               // (wb: the same for every thread of the launch)
        float *prio = gsh(X.prio, off), *pmax = gsh(X.pmax, off);
        int32_t *sj = reinterpret_cast<int32_t *>(scr);
        int32_t j = 0;
        float pnew = 0.0f, pm0 = 0.0f;
        if (wb) {
            if (t < BP) j = (int32_t)min(max((int64_t)reinterpret_cast<const int32_t *>(pw + PW_IDX)[m], (int64_t)0), X.ring_len - 1);
            if (t == 0) pm0 = pmax[0];
            if (live) pnew = per_priority(diff, X.eps_p, X.alpha);
            if (t < BP) sj[t] = live ? j : -1;
            float pm = pnew;                                                                // >= 0; threads outside the batch hold 0
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) pm = fmaxf(pm, __shfl_xor(pm, o, 64));
            if ((t & 63) == 0 && t < BP) scr[BP + (t >> 6)] = pm;
        }
        const float wd = wm * diff;                                                         // (w diff) diff: head_critic's product shape
        const float s1 = wave_sum64(wd * diff), s2 = wave_sum64(dq);
        if ((t & 63) == 0) { red[t >> 6] = s1; red[4 + (t >> 6)] = s2; }
        __syncthreads();
        if (t == 0) {
            d.losses[0] = (red[0] + red[1]) / (float)d.batch;
            adam_at(c, off_b3(CIN, 1), red[4] + red[5], A.store_grad != 0);
            if (wb) pmax[0] = fmaxf(pm0, fmaxf(scr[BP], scr[BP + 1]));                      // only ever raised
        }
        if (wb) {
            if (live) {
                bool last = true;
                const int4 *sj4 = reinterpret_cast<const int4 *>(sj);
#pragma unroll
                for (int q = 0; q < BP / 4; ++q) {
                    const int4 v = sj4[q];
                    last = last && !((4 * q + 0 > t && v.x == j) || (4 * q + 1 > t && v.y == j) || (4 * q + 2 > t && v.z == j) || (4 * q + 3 > t && v.w == j));
                }
                if (last) prio[j] = pnew;
            }
            __syncthreads();                     // scr is the weight ring: the caller fills it next
        }
    }
}

// ================================================================================================================================
// P3 / P6: D1' [m][k] = mask1 .* sum_n D2[n][m] W2[k][n] for one 64-wide k-tile and the whole batch, D2[n][m] = (sum_o W3[n][o]
// d3[o][m]) (h2[n][m] > 0) generated from relu(layer 2) as it is loaded -- straight into MFMA operand layout, no LDS; the weights
// stream through an LDS ring in 32-deep n-chunks.  The product is computed TRANSPOSED (rows = samples, columns = hidden units): its
// D layout is then the B operand of the layer-1 gradient gW1[j][k] = sum_m x[j][m] D1[k][m], which follows on the matrix pipe without
// any LDS round trip (the bias gradient is the row of ones of the input block).  ADAM + soft update for the k-tile's layer-1 columns.
// ================================================================================================================================
#ifndef SHEMS_D1_PAD
#define SHEMS_D1_PAD 0      // (diagnostic builds: extra dynamic LDS = fewer resident workgroups, to read the launch's sensitivity to occupancy)
#endif
constexpr int D1_S = 33;
constexpr unsigned kNarrowBelow = 48;
// KT = 32-wide sub-tiles per workgroup: 2 = a 64-wide k-tile (four workgroups per learner -- the form for wide groups, fewest reads of
// relu(layer 2)); 1 = a 32-wide one (eight per learner: with few learners four do not fill the chip -- 128 workgroups at 32 learners)
constexpr int d1_ring(int KT) { return 2 * 32 * KT * D1_S > 4 * KT * 8 * 64 ? 2 * 32 * KT * D1_S : 4 * KT * 8 * 64; }      // floats: the ring, later the four waves' gW1 partials
constexpr int d1_lds(int KT) { return (d1_ring(KT) + 1024 + 2 * BP + 8 + W1K * BP + W1K * 32 * KT) * 4; }

// CLONE: the supervised update's instantiation (k_tp_d1_clone) takes the cloning head at compile time; TWIN: TD3's (k_tp_d1_twin) the twin
// head, PER: prioritized replay's (k_tp_d1_per) the weighted head; otherwise NetArgs.head decides.
template <int IN, int KT, bool TL, bool HP, bool CLONE = false, bool TWIN = false, bool PER = false>
__device__ __forceinline__ void d1_body(const NetArgs &A, const int bx, const int by, float *smem, const shems_group_hparams *hp,
                                        const TwinX *tx = nullptr, const PerX *px = nullptr)
{
    typedef NetOf<IN> N;
    constexpr int OUT = N::OUT;
    constexpr int KW = 32 * KT;                  // k-tile width
    float *ring = smem;                          // [2][KW k][33]
    float *w3s = ring + d1_ring(KT);             // [512][2] frozen W3
    float *d3s = w3s + 1024;                     // [2][BP]
    float *red = d3s + 2 * BP;                   // [8]
    float *xs = red + 8;                         // [12][BP] the input block        } operands of what follows the chunk loop: staged by the
    float *wls = xs + W1K * BP;                  // [12][KW] layer-1 image, k-tile  } prologue's requests, no round trip after the loop
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int kt = bx, k0 = KW * kt;
    const int64_t off = (int64_t)by * A.gstride;
    shems_ddpg d = A.d;
    AdamCtx c = A.c;
    gshift(d, off); gshift(c, off);
    if constexpr (HP) {                          // the heads read gamma / batch from d
        const shems_group_hparams h = hp[by];
        d.gamma = h.gamma; d.batch = hp_batch(h);
        hp_adam(c, h, N::critic);
        // (the quotient is formed on the vector ALU and lives to the kernel's end: left in vector registers it is the one value the narrow
        // Flux-order form spills, 12 bytes of scratch in k_tp_d1_hp<SIN, 1, false>; the new instantiations keep it in scalar registers)
        if constexpr (CLONE || TWIN || PER) c.k1 = uniform_f64(c.k1);
    }
    float *ws = d.ws;
    const float *__restrict__ P = c.p;
    const float *__restrict__ W2 = P + off_w2(IN);
    const float *__restrict__ H2 = N::H2(ws);
    const int m = 32 * w + li;

    // A chunk q: W2[k0 .. k0 + 63][32 q .. 32 q + 31] (128 B per row), two float4 per thread; rows >= 250 clamped (their outputs are
    // never stored), columns >= 500 of the last chunk meet D2 rows that are exactly zero
    // (tiled layout: the same 32 columns of rows k0 .. are 128-byte pieces 256 bytes apart inside tile (k0 / 64, q / 2); pad rows are zeros)
    const float *__restrict__ Wt = TL ? gsh(A.w2t, off) + TL_P * TL_TILE + (int64_t)(k0 >> 6) * 8 * TL_BLOCK + (k0 & 63) * 64 : nullptr;
    auto a_load = [&](int q, f32x4 (&v)[KT]) {
#pragma unroll
        for (int it = 0; it < KT; ++it) {
            const int e = it * 256 + tid;
            if constexpr (TL) v[it] = *reinterpret_cast<const f32x4 *>(Wt + (int64_t)(q >> 1) * TL_BLOCK + (e >> 3) * 64 + 32 * (q & 1) + 4 * (e & 7));
            else {
                const int k = min(k0 + (e >> 3), H1N - 1);
                v[it] = *reinterpret_cast<const f32x4 *>(W2 + (int64_t)k * H2N + 32 * q + 4 * (e & 7));
            }
        }
    };
    auto a_store = [&](float *buf, const f32x4 (&v)[KT]) {
#pragma unroll
        for (int it = 0; it < KT; ++it) {
            const int e = it * 256 + tid;
            float *p = buf + (e >> 3) * D1_S + 4 * (e & 7);
            p[0] = v[it][0]; p[1] = v[it][1]; p[2] = v[it][2]; p[3] = v[it][3];
        }
    };
    // B operand source of chunk q: h2[32 q + 2 s + lh][m]
    auto h_load = [&](int q, float (&h)[16]) {
#pragma unroll
        for (int s = 0; s < 16; ++s) h[s] = H2[(int64_t)(32 * q + 2 * s + lh) * BP + m];
    };
    f32x4 pv[KT];
    float hc[16], hn[16];
    a_load(0, pv);
    h_load(0, hc);
    const f32x4 w3v = reinterpret_cast<const f32x4 *>(N::w3f(ws))[tid];
    const float *w1i = N::w1i(ws);
    const float *X = N::X(ws);
    constexpr int WLN = (W1K * KW + 255) / 256;          // 3 (KT = 2) / 2 (KT = 1: 384 floats)
    float xv[6], wlv[WLN];
#pragma unroll
    for (int s = 0; s < 6; ++s) xv[s] = X[s * 256 + tid];
#pragma unroll
    for (int s = 0; s < WLN; ++s) { const int e = min(s * 256 + tid, W1K * KW - 1); wlv[s] = w1i[(e / KW) * W1C + k0 + e % KW]; }
    if constexpr (CLONE) head_clone(A, d, c, d3s, red, kt == 0);
    else if constexpr (TWIN) head_twin(A, d, c, d3s, red, kt == 0, *tx, off);
    else if constexpr (PER) head_critic_per(A, d, c, d3s, red, kt == 0, *px, off, ring);
    else if (A.head == 1) head_critic(A, d, c, d3s, red, kt == 0); else head_actor(A, d, c, d3s, red, kt == 0);
    reinterpret_cast<f32x4 *>(w3s)[tid] = w3v;
#pragma unroll
    for (int s = 0; s < 6; ++s) xs[s * 256 + tid] = xv[s];
#pragma unroll
    for (int s = 0; s < WLN; ++s) if (s * 256 + tid < W1K * KW) wls[s * 256 + tid] = wlv[s];
    a_store(ring, pv);
    __syncthreads();
    const float d30 = d3s[m], d31 = d3s[BP + m];

    f32x16 acc[KT];
#pragma unroll
    for (int tt = 0; tt < KT; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tt][r] = 0.0f;
    // One n-chunk: the next chunk's weights and error-signal source are requested first and are not touched before the following step
    // (two register sets taken in turn: a copy `hc = hn` at the end of the step is moved up by the scheduler into the product, where its
    // wait for the just-issued loads -- loads retire in order -- stalls the matrix pipe every chunk).
    auto step = [&](auto prefetch, int q, const float (&hcur)[16], float (&hnext)[16]) {
        constexpr bool PF = decltype(prefetch)::value;
        const float *buf = ring + (q & 1) * KW * D1_S;
        // (never behind a run-time branch: the compiler's wait in front of hcur would be the one of the path WITHOUT new requests, which
        // on the other path waits for them; the last step is a separate instance instead)
        if constexpr (PF) { a_load(q + 1, pv); h_load(q + 1, hnext); }
        __builtin_amdgcn_sched_barrier(0);
        const float *pb = buf + li * D1_S + lh;
        const float *pw = w3s + 2 * (32 * q + lh);
        // (the LDS operands of k-step s + 1 are read before the products of step s are issued: read -> wait -> products leaves the LDS
        // latency uncovered behind every pair)
        float2 wA = *reinterpret_cast<const float2 *>(pw), wB;
        constexpr int T1 = KT == 2 ? 32 * D1_S : 0;          // second sub-tile's rows (KT = 1: the same operand, unused)
        float bA0 = pb[0], bA1 = pb[T1], bB0, bB1;
        auto prod = [&](int s, const float2 w3, float b0, float b1) {
            const float gsum = OUT == 2 ? fmaf(w3.y, d31, w3.x * d30) : w3.x * d30;
            const float d2 = hcur[s] > 0.0f ? gsum : 0.0f;
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(d2, b0, acc[0], 0, 0, 0);
            if constexpr (KT == 2) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(d2, b1, acc[1], 0, 0, 0);
        };
#pragma unroll
        for (int s = 0; s < 16; s += 2) {
            wB = *reinterpret_cast<const float2 *>(pw + 4 * (s + 1)); bB0 = pb[2 * (s + 1)]; bB1 = pb[T1 + 2 * (s + 1)];
            __builtin_amdgcn_sched_barrier(0);
            prod(s, wA, bA0, bA1);
            if (s < 14) { wA = *reinterpret_cast<const float2 *>(pw + 4 * (s + 2)); bA0 = pb[2 * (s + 2)]; bA1 = pb[T1 + 2 * (s + 2)]; }
            __builtin_amdgcn_sched_barrier(0);
            prod(s + 1, wB, bB0, bB1);
        }
        if constexpr (PF) a_store(ring + ((q + 1) & 1) * KW * D1_S, pv);
        __syncthreads();
    };
#pragma unroll 1
    for (int q = 0; q < 14; q += 2) {
        step(std::true_type{}, q, hc, hn);
        step(std::true_type{}, q + 1, hn, hc);
    }
    step(std::true_type{}, 14, hc, hn);
    step(std::false_type{}, 15, hn, hc);
    // ---- this thread's four layer-1 elements: their ADAM state is requested now and arrives under the products below ----
    constexpr int NE = 2 * KT;                   // elements per thread: [KT tt][8 r][64 lanes] over 256 threads
    int ei[NE];
    float em[NE], ev[NE], epp[NE], et[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int sidx = u * 256 + tid, ln = sidx & 63, rr = (sidx >> 6) & 7, tt = sidx >> 9;
        const int j = drow(rr, ln >> 5), k = k0 + 32 * tt + (ln & 31);
        ei[u] = (k < H1N && (j < IN || j == W1K - 1)) ? (j == W1K - 1 ? off_b1(IN) + k : j * H1N + k) : -1;
        const int e = max(ei[u], 0);
        em[u] = c.mt[e]; ev[u] = c.vt[e]; epp[u] = c.p[e]; et[u] = c.target[e];
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- layer-1 relu mask: pre-activations transposed, rows = samples of this wave's column tile, columns = the k-tile's units ----
    float xa[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) xa[s] = xs[(2 * s + lh) * BP + m];
    // A operands of the layer-1 gradient: x[j = li][32 w + drow(r, lh)] (rows >= 12 zero)
    f32x4 xq[4];
    {
        const float keep = li < W1K ? 1.0f : 0.0f;
        const float *px = xs + min(li, W1K - 1) * BP + 32 * w + 4 * lh;
#pragma unroll
        for (int q = 0; q < 4; ++q) xq[q] = *reinterpret_cast<const f32x4 *>(px + 8 * q) * keep;
    }
    float *redp = ring;                          // [4 waves][KT tt][8 r][64 lanes]  (the ring is free: the loop ended with a barrier)
#pragma unroll
    for (int tt = 0; tt < KT; ++tt) {
        float wb[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) wb[s] = wls[(2 * s + lh) * KW + 32 * tt + li];
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < 6; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s], wb[s], t, 0, 0, 0);
        f32x16 g;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float dv = t[r] > 0.0f ? acc[tt][r] : 0.0f;                 // D1'[m = drow(r, lh)][k = li]
            g = __builtin_amdgcn_mfma_f32_32x32x2f32(xq[r >> 2][r & 3], dv, g, 0, 0, 0);
        }
        // rows j = drow(r, lh) < 12: r = 0..3 (both halves), r = 4..7 (lh = 0)
#pragma unroll
        for (int r = 0; r < 8; ++r) redp[((w * KT + tt) * 8 + r) * 64 + lane] = g[r];
    }
    __syncthreads();
    // (consumed unconditionally: left to itself the compiler moves the requests above behind the `ei >= 0` that guards the stores)
#pragma unroll
    for (int u = 0; u < NE; ++u) asm volatile("" : "+v"(em[u]), "+v"(ev[u]), "+v"(epp[u]), "+v"(et[u]));
    float *gP = const_cast<float *>(c.g);
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int sidx = u * 256 + tid, ln = sidx & 63, rr = (sidx >> 6) & 7, tt = sidx >> 9;
        const float *pr = redp + (tt * 8 + rr) * 64 + ln;
        const float gsum = ((pr[0] + pr[KT * 8 * 64]) + pr[2 * KT * 8 * 64]) + pr[3 * KT * 8 * 64];
        adam_math(c, gsum, em[u], ev[u], epp[u], et[u]);
        if (ei[u] >= 0) {
            const int e = ei[u];
            c.mt[e] = em[u]; c.vt[e] = ev[u]; c.p[e] = epp[u]; c.target[e] = et[u];
            if (A.store_grad != 0) gP[e] = gsum;
            if constexpr (N::critic) {           // P5 runs the UPDATED critic: its layer-1 image, element by element (zeros from P0)
                const int j = drow(rr, ln >> 5), k = k0 + 32 * tt + (ln & 31);
                w1i_of(ws, IMG_CRITIC_NEW)[j * W1C + k] = epp[u];
            }
        }
    }
}

// ================================================================================================================================
// P4 / P7: gW2[k][n] = sum_m h1[k][m] D2[n][m] for one 64 x 64 tile, ADAM + soft target update on it; the k-tile-0 workgroups also
// finish gb2[n] = sum_m D2[n][m] and gW3[n][o] = sum_m h2[n][m] d3[o][m] of their n-tile.  h1' (samples x units) is recomputed on the
// matrix pipe per 32-sample block -- its D layout is the A operand; D2 goes through LDS.
// This phase is the update's HBM stream: 32 B in and out per parameter of W2 (moments, parameter, target) against 64 FLOP.  What it
// reaches depends on how the four arrays are touched and on how many bytes a CU keeps in flight (measured with the matrix work switched
// off, 400 learners, 1.65 GB per launch; profiles/r05_gw2_stream_forms.txt): 4-byte accesses in the accumulator's layout (128-byte row
// pieces) 3.85 TB/s; 16-byte accesses in row-major order of the tile, 256-byte pieces 4.1 TB/s, 1 KB pieces 4.7 TB/s = the rate of a
// plain elementwise ADAM sweep (a device copy of the same bytes: 5.5 TB/s) -- but only with ~256 KB in flight per CU: a 32 x 256 tile
// whose state is requested in quarters (to fit the registers beside the product) fell to 1.9 TB/s.  So: the whole tile's state is
// requested FIRST, 16 bytes per lane in row-major order (thread -> four consecutive columns of one row), the product runs under those
// loads, and the finished tile changes hands through LDS (accumulator layout -> rows) before ADAM.
// ================================================================================================================================
constexpr int GW_S = BP + 1;
constexpr int GW_TS = 68;          // row stride of the row-major copy of the finished tile [64 k][68] (over the D2 panel)
constexpr int GW_WGS = 4 * NT;     // k-tiles x n-tiles of 64 per learner
// (Round 6 also built a four-workgroups-per-CU form -- the error signal from registers instead of LDS: 40 448 B, and a 128-register budget, which
// spills 12 registers -- no gain at 400 learners (1.926-1.938 against 1.927-1.935 ms per step), 3 % slower at 32 (profiles/r06_gw2_ab.txt); removed.)
constexpr int GW_LDS = (64 * GW_S + 2 * BP + 64 * 2 + 64 * 3 + W1K * BP) * 4;
static_assert(64 * GW_TS <= 64 * GW_S, "the row-major copy of a tile fits the D2 panel it replaces");

template <int IN, bool TL, bool HP>
__device__ __forceinline__ void gw2_body(const NetArgs &A, const int bx, const int by, float *smem, const shems_group_hparams *hp)
{
    typedef NetOf<IN> N;
    constexpr int OUT = N::OUT;
    float *d2s = smem;                           // [64 n][129]; later the tile [64 k][68]
    float *d3s = d2s + 64 * GW_S;                // [2][BP]
    float *w3s = d3s + 2 * BP;                   // [64][2]
    float *rs = w3s + 64 * 2;                    // [64][3] row sums: gb2, gW3[.][0], gW3[.][1]
    float *xs = rs + 64 * 3;                     // [12][BP] the input block
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int nt = bx & 7, kt = bx >> 3, n0 = 64 * nt, k0 = 64 * kt;
    const int kw = w >> 1, nw = w & 1;
    const int64_t off = (int64_t)by * A.gstride;
    shems_ddpg d = A.d;
    AdamCtx c = A.c;
    gshift(d, off); gshift(c, off);
    if constexpr (HP) hp_adam(c, hp[by], N::critic);
    float *ws = d.ws;
    const float *__restrict__ H2 = N::H2(ws);
    const bool store_grad = A.store_grad != 0;

    // Requests, in the order the workgroup needs them: loads retire in order, so a wait for any operand also waits for everything requested
    // before it.  The small operands of the panel and of the product come first; the tile's state -- 16 float4, the kernel's HBM stream --
    // is requested LAST and is still arriving while the panel is built and the product runs (nothing later in the kernel issues a load).
    f32x4 hv[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int e = it * 256 + tid;
        hv[it] = *reinterpret_cast<const f32x4 *>(H2 + (int64_t)(n0 + (e >> 5)) * BP + 4 * (e & 31));
    }
    const float d3v = N::d3(ws)[tid];
    const float w3v = N::w3f(ws)[2 * n0 + (tid & 127)];
    const float *w1i = N::w1i(ws);
    float wb[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) wb[s] = w1i[(2 * s + lh) * W1C + k0 + 32 * kw + li];
    const float *X = N::X(ws);
    float xv[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) xv[s] = X[s * 256 + tid];
    __builtin_amdgcn_sched_barrier(0);
    // this thread's 16 elements of the tile, row-major: float4 it = row 16 it + (tid >> 4), columns 4 (tid & 15) .. + 3
    // Tiled layout: the same float4 (row 16 it + tid / 16, columns 4 (tid % 16) ..) is float4 number 256 it + tid of each of the tile's
    // four arrays, which lie one behind the other: the workgroup's whole state is ONE contiguous 64 KB piece, read here, written below.
    int eidx[4];
    f32x4 am[4], av[4], ap[4], at[4];
    float *tile = TL ? gsh(A.w2t, off) + tl_tile(kt, nt) + 4 * tid : nullptr;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int k = k0 + 16 * it + (tid >> 4), n = n0 + 4 * (tid & 15);
        eidx[it] = (k < H1N && n < H2N) ? off_w2(IN) + k * H2N + n : -1;          // (500 is a multiple of 4: a float4 is all in or all out)
        if constexpr (TL) {
            // (non-temporal: a tile's state is next touched one whole grouped update -- 4 GB of other traffic -- later; on the 64 KB
            // pieces the hint is worth 4.90 -> 5.13 TB/s, a device copy's rate; on the Flux order's 256-byte pieces it costs a third:
            // tools/micro/adam_stream.hip, profiles/r06_micro_adam_stream.txt)
            const float *q = tile + 1024 * it;
            am[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(q + TL_M * TL_TILE));
            av[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(q + TL_V * TL_TILE));
            ap[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(q + TL_P * TL_TILE));
            at[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(q + TL_T * TL_TILE));
        } else {
            const int e = off_w2(IN) + min(k, H1N - 1) * H2N + min(n, H2N - 4);
            am[it] = *reinterpret_cast<const f32x4 *>(c.mt + e); av[it] = *reinterpret_cast<const f32x4 *>(c.vt + e);
            ap[it] = *reinterpret_cast<const f32x4 *>(c.p + e); at[it] = *reinterpret_cast<const f32x4 *>(c.target + e);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    d3s[tid] = d3v;
    if (tid < 128) w3s[tid] = w3v;
#pragma unroll
    for (int s = 0; s < 6; ++s) xs[s * 256 + tid] = xv[s];
    __syncthreads();
    // D2 panel + row sums
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int e = it * 256 + tid, nl = e >> 5, m4 = 4 * (e & 31);
        const float2 w3 = *reinterpret_cast<const float2 *>(w3s + 2 * nl);
        float sb = 0.0f, s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float h = hv[it][i], e0 = d3s[m4 + i], e1 = d3s[BP + m4 + i];
            const float gsum = OUT == 2 ? fmaf(w3.y, e1, w3.x * e0) : w3.x * e0;
            const float d2 = h > 0.0f ? gsum : 0.0f;
            d2s[nl * GW_S + m4 + i] = d2;
            sb += d2; s0 = fmaf(h, e0, s0); s1 = fmaf(h, e1, s1);
        }
        if (kt == 0) {                           // (workgroup-uniform)
            sb = half_sum32(sb); s0 = half_sum32(s0); s1 = half_sum32(s1);
            if (li == 0) { rs[nl * 3 + 0] = sb; rs[nl * 3 + 1] = s0; rs[nl * 3 + 2] = s1; }
        }
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float *pb = d2s + (32 * nw + li) * GW_S + 4 * lh;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        float xa[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) xa[s] = xs[(2 * s + lh) * BP + 32 * mt + li];
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < 6; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s], wb[s], t, 0, 0, 0);       // h1'[m][k] pre-activations
        // (B operand of k-step r + 1 read from LDS before the product of step r is issued)
        float bA = pb[32 * mt], bB;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            bB = pb[32 * mt + ((r + 1) & 3) + 8 * ((r + 1) >> 2)];
            __builtin_amdgcn_sched_barrier(0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fmaxf(t[r], 0.0f), bA, acc, 0, 0, 0);
            if (r < 14) bA = pb[32 * mt + ((r + 2) & 3) + 8 * ((r + 2) >> 2)];
            __builtin_amdgcn_sched_barrier(0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fmaxf(t[r + 1], 0.0f), bB, acc, 0, 0, 0);
        }
    }
    // the tile changes hands: accumulator layout -> LDS [64 k][68] (over the D2 panel, which every wave has finished reading) -> rows
    __syncthreads();
    float *T = d2s;
#pragma unroll
    for (int r = 0; r < 16; ++r) T[(32 * kw + drow(r, lh)) * GW_TS + 32 * nw + li] = acc[r];
    __syncthreads();
    {
        float *gW = const_cast<float *>(c.g);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const f32x4 g4 = *reinterpret_cast<const f32x4 *>(T + (16 * it + (tid >> 4)) * GW_TS + 4 * (tid & 15));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float m_ = am[it][i], v_ = av[it][i], p_ = ap[it][i], t_ = at[it][i];
                adam_math(c, g4[i], m_, v_, p_, t_);
                am[it][i] = m_; av[it][i] = v_; ap[it][i] = p_; at[it][i] = t_;
            }
            if (eidx[it] >= 0) {                 // (pad rows / columns of the tiled layout stay zero: never written)
                const int e = eidx[it];
                if constexpr (TL) {
                    float *q = tile + 1024 * it;
                    __builtin_nontemporal_store(am[it], reinterpret_cast<f32x4 *>(q + TL_M * TL_TILE));
                    __builtin_nontemporal_store(av[it], reinterpret_cast<f32x4 *>(q + TL_V * TL_TILE));
                    __builtin_nontemporal_store(ap[it], reinterpret_cast<f32x4 *>(q + TL_P * TL_TILE));
                    __builtin_nontemporal_store(at[it], reinterpret_cast<f32x4 *>(q + TL_T * TL_TILE));
                } else {
                    *reinterpret_cast<f32x4 *>(c.mt + e) = am[it]; *reinterpret_cast<f32x4 *>(c.vt + e) = av[it];
                    *reinterpret_cast<f32x4 *>(c.p + e) = ap[it]; *reinterpret_cast<f32x4 *>(c.target + e) = at[it];
                }
                if (store_grad) *reinterpret_cast<f32x4 *>(gW + e) = g4;
            }
        }
    }
    if (kt == 0 && tid < 64 * 3) {               // one element per thread: (row, b2 | W3[.][0] | W3[.][1])
        const int nl = tid / 3, col = tid - nl * 3, n = n0 + nl;
        if (n < H2N && col - 1 < OUT) adam_at(c, col == 0 ? off_b2(IN) + n : off_w3(IN) + n * OUT + (col - 1), rs[tid], store_grad);
    }
}

// ---- one launch per phase (the plain form: every learner of the group in the same phase) ---------------------------------------
__global__ __launch_bounds__(256) void k_tp_prep(PrepArgs A) { prep_body<false>(A, blockIdx.x, blockIdx.y, nullptr); }
template <bool QG, int NTL, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NTL == 4 ? 3 : 4, 4))) void k_tp_fwd(FwdArgs A)      // (the wide form's LDS allows three workgroups per CU)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    fwd_body<QG, NTL, TL, false>(A, blockIdx.x, blockIdx.y, smem, nullptr);
}
// (Round 6 also built the forward launches as PERSISTENT workgroups -- 768 / 1 024 of them drawing their (n-tile, learner) items from a counter, which
// tools/micro/fwd_anatomy.hip rates 0.86 against 0.82 of the peak for loops without prologues -- verified against the float64 oracle, measured slower
// with the real prologues and epilogues (P1 373.5 against 355.3 us, P2 143.0 / 133.6, P5 278.9 / 273.8; 204.4 against 207.6 k updates/s), removed:
// profiles/r06_fwd_persistent_ab.txt.)
// A learner's k-tile workgroups (T = 8 / KT of them) read the same 256 KB of relu(layer 2): they are placed on ONE XCD (workgroup id
// mod 8 picks the XCD and its L2), consecutive in its dispatch order -- learner = 8 (q / T) + xcd, k-tile = q mod T with q = id / 8.
template <int IN, int KT, bool TL, bool HP, bool CLONE = false, bool TWIN = false, bool PER = false>
__device__ __forceinline__ void d1_entry(const NetArgs &A, float *smem, const shems_group_hparams *hp, const TwinX *tx = nullptr,
                                         const PerX *px = nullptr)
{
    constexpr unsigned T = 8 / KT;
    const unsigned id = blockIdx.x, xcd = id & 7u, q = id >> 3;
    const unsigned learner = 8u * (q / T) + xcd;
    if (learner >= (unsigned)A.learners) return;
    d1_body<IN, KT, TL, HP, CLONE, TWIN, PER>(A, (int)(q % T), (int)learner, smem, hp, tx, px);
}
template <int IN, int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1(NetArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<IN, KT, TL, false>(A, smem, nullptr);
}
template <int IN, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_gw2(NetArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    gw2_body<IN, TL, false>(A, blockIdx.x, blockIdx.y, smem, nullptr);
}

// ---- the same launches with per-learner hyper-parameters (shems_ddpg_group_update_tp with d_hp): own names, the bodies above with HP = true ----
__global__ __launch_bounds__(256) void k_tp_prep_hp(PrepArgs A, const shems_group_hparams *hp) { prep_body<true>(A, blockIdx.x, blockIdx.y, hp); }
// (shems_ddpg_group_update_tp_x: the sampler with per-learner ring lengths; the other seven launches are the *_hp kernels)
__global__ __launch_bounds__(256) void k_tp_prep_x(PrepArgs A, const shems_group_hparams *hp, const shems_group_xparams *xp, const int64_t *pushed)
{
    prep_body<true, true>(A, blockIdx.x, blockIdx.y, hp, xp, pushed);
}
template <bool QG, int NTL, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NTL == 4 ? 3 : 4, 4))) void k_tp_fwd_hp(FwdArgs A, const shems_group_hparams *hp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    fwd_body<QG, NTL, TL, true>(A, blockIdx.x, blockIdx.y, smem, hp);
}
template <int IN, int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1_hp(NetArgs A, const shems_group_hparams *hp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<IN, KT, TL, true>(A, smem, hp);
}
template <int IN, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_gw2_hp(NetArgs A, const shems_group_hparams *hp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    gw2_body<IN, TL, true>(A, blockIdx.x, blockIdx.y, smem, hp);
}

// ================================================================================================================================
// The grouped supervised and critic-only updates (shems_ddpg_group_clone_update_tp / _critic_update_tp): their own sampler and the
// actor's D1 launch with the cloning head; every other launch of theirs is one of the kernels above.
// The sampler shifts the ring by a stride of ITS OWN (demonstrations and an "mc" ring of returns live outside the learners' slabs);
// the images come from prep_body's own roles.  Role 0 writes what prep_body's writes, from the same expressions (the critic-only update
// leaves the bits of the update's critic half); CLONE reads s and a of a slot alone, leaves a_demo in TP_ADEMO and zeros in the action
// rows of the input block (the actor's image has zeros there: the rows must only be finite), and freezes the actor's output layer alone.
// grid (CLONE ? 2 : 5, learners): CLONE's workgroup 1 packs the actor's image.
// ================================================================================================================================
struct PrepRingArgs { PrepArgs p; int64_t rstride; };
template <bool HP, bool CLONE>
__device__ __forceinline__ void prep_ring_body(const PrepRingArgs &R, const int role, const int l, const shems_group_hparams *hp)
{
    const PrepArgs &A = R.p;
    if (role > 0) { prep_body<HP>(A, CLONE ? 1 + NET_ACTOR : role, l, hp); return; }
    const int tid = threadIdx.x;
    shems_ddpg d = A.d;
    shems_replay ring = A.ring;
    gshift(d, (int64_t)l * A.gstride); gshift(ring, (int64_t)l * R.rstride);
    float *ws = d.ws;
    if constexpr (HP) d.batch = hp_batch(hp[l]);
    const uint64_t seed = A.seed + (uint64_t)l;
    if (tid < BP) {
        const int m = tid;
        const u32x4 x = philox4x32_10((uint32_t)(m >> 2), 0u, A.tick, kStreamSample, (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t w = (m & 3) == 0 ? x.x : (m & 3) == 1 ? x.y : (m & 3) == 2 ? x.z : x.w;
        const int64_t j = (int64_t)(w % (uint32_t)A.ring_len);
        const bool live = m < d.batch;
        float sv[SIN], s2v[SIN], lo[SIN], hi[SIN];
#pragma unroll
        for (int k = 0; k < SIN; ++k) {
            sv[k] = ring.s[j * SIN + k]; lo[k] = d.s_min[k]; hi[k] = d.s_max[k];
            if constexpr (!CLONE) s2v[k] = ring.s2[j * SIN + k];
        }
        const float a0 = ring.a[j * 2], a1 = ring.a[j * 2 + 1];
#pragma unroll
        for (int k = 0; k < SIN; ++k) {
            const float den = (hi[k] - lo[k]) + 1e-8f;                                     // MPS:56
            ws[TP_X + k * BP + m] = live ? (sv[k] - lo[k]) / den : 0.0f;
            if constexpr (!CLONE) ws[TP_X2 + k * BP + m] = live ? (s2v[k] - lo[k]) / den : 0.0f;
        }
        ws[TP_X + 11 * BP + m] = 1.0f;
        if constexpr (CLONE) {
            ws[TP_X + 9 * BP + m] = 0.0f; ws[TP_X + 10 * BP + m] = 0.0f;
            ws[TP_ADEMO + m] = live ? a0 : 0.0f;
            ws[TP_ADEMO + BP + m] = live ? a1 : 0.0f;
        } else {
            const float rr = ring.r[j];
            const bool dn = ring.done[j] != 0;
            ws[TP_X + 9 * BP + m] = live ? a0 : 0.0f;
            ws[TP_X + 10 * BP + m] = live ? a1 : 0.0f;
            ws[TP_X2 + 9 * BP + m] = 0.0f; ws[TP_X2 + 10 * BP + m] = 0.0f; ws[TP_X2 + 11 * BP + m] = 1.0f;
            ws[TP_R + m] = live ? rr : 0.0f;
            ws[TP_DONE + m] = live && dn ? 1.0f : 0.0f;
        }
        reinterpret_cast<int32_t *>(ws + TP_IDX)[m] = live ? (int32_t)j : -1;
    }
    // frozen output layers
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int e = it * 256 + tid, n = e >> 1, o = e & 1;
        ws[TP_FW3A + e] = n < H2N ? d.actor[off_w3(SIN) + min(e, 2 * H2N - 1)] : 0.0f;
        if constexpr (!CLONE) ws[TP_FW3C + e] = (n < H2N && o == 0) ? d.critic[off_w3(CIN) + min(n, H2N - 1)] : 0.0f;
    }
    if constexpr (CLONE) {
        if (tid < 2) ws[TP_FB3 + 2 + tid] = d.actor[off_b3(SIN, 2) + tid];
    } else if (tid < 8)
        ws[TP_FB3 + tid] = tid == 0 ? d.critic[off_b3(CIN, 1)] : tid == 1 ? d.critic_t[off_b3(CIN, 1)]
                         : tid == 2 ? d.actor[off_b3(SIN, 2)] : tid == 3 ? d.actor[off_b3(SIN, 2) + 1]
                         : tid == 4 ? d.actor_t[off_b3(SIN, 2)] : tid == 5 ? d.actor_t[off_b3(SIN, 2) + 1] : 0.0f;
}
template <bool CLONE>
__global__ __launch_bounds__(256) void k_tp_prep_ring(PrepRingArgs R) { prep_ring_body<false, CLONE>(R, blockIdx.x, blockIdx.y, nullptr); }
template <bool CLONE>
__global__ __launch_bounds__(256) void k_tp_prep_ring_hp(PrepRingArgs R, const shems_group_hparams *hp)
{
    prep_ring_body<true, CLONE>(R, blockIdx.x, blockIdx.y, hp);
}
// the actor's D1 launch with the cloning head: d1_body's instantiation of its own, the twins of k_tp_d1<SIN, ..> / k_tp_d1_hp<SIN, ..>
template <int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1_clone(NetArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<SIN, KT, TL, false, true>(A, smem, nullptr);
}
template <int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1_clone_hp(NetArgs A, const shems_group_hparams *hp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<SIN, KT, TL, true, true>(A, smem, hp);
}

// ================================================================================================================================
// TD3 for groups (shems_td3_group_update_tp; include/shems_hip.h): a second critic beside every learner's first.
// Critic 2 has a workspace of its own, ws2, which MIRRORS the carve above wherever NetOf<CIN> and the forward jobs point: the unchanged
// k_tp_gw2<CIN> and d1_body walk critic 2 through a NetArgs whose shems_ddpg names critic 2's blocks and ws2.
//   ws2 + TP_X      [12][BP] the input block [s; a; 1] again (the sampler writes both)
//   ws2 + TP_W1I    slot NET_CRITIC_T: critic2_t's layer-1 image, slot NET_CRITIC: critic2's, slot IMG_CRITIC_NEW: critic2's after its update (unread)
//   ws2 + TP_FW3C   frozen W3 of critic2;  ws2 + TP_FB3: [0] b3 of critic2, [1] b3 of critic2_t
//   ws2 + TP_P3     pass NET_CRITIC_T: critic2_t(s', a~') partials, pass NET_CRITIC: critic2(s, a) partials
//   ws2 + TP_D3C    dq of critic 2's loss;  ws2 + TP_H2C: relu(layer 2) of critic2(s, a)
//   ws2 + T2_AT     [2][BP] a~' (n-tile 0 of critic_t's pass);  T2_PUB: y, q'1, q'2 [3][BP] from critic 1's head, T2_PUB2: from critic 2's
// (T2_* take the rows the actor's input gradient has in ws; TP_X2, TP_R, TP_DONE, TP_IDX and the actor slots of ws2 are not used.)
// ================================================================================================================================
constexpr int64_t T2_AT = TP_DAP;
constexpr int64_t T2_PUB = T2_AT + 2 * BP;
constexpr int64_t T2_PUB2 = T2_PUB + 3 * BP;
constexpr int64_t T2_FLOATS = TP_H2A;              // (no second relu(layer 2) block: ws2 ends where the actor's begins in ws)
static_assert(T2_PUB2 + 3 * BP <= TP_D3C, "the published rows fit the input gradient's block");
static_assert(T2_AT == SHEMS_TD3_GROUP_WS2_PUB && T2_AT % 4 == 0, "shems_hip.h names where the published rows begin");

// The sampler: roles 0..4 are prep_body's on the learner's own record; role 0 then repeats its input block in ws2; roles 5, 6 are
// prep_body's image roles on a record whose critic blocks and workspace are critic 2's (critic2_t, critic2); role 5 also freezes critic
// 2's output layers (prep_body's expressions for critic 1's).  grid (7, learners).
struct PrepTd3Args { PrepArgs p; float *critic2, *critic2_t, *ws2; };
template <bool HP>
__device__ __forceinline__ void prep_td3_body(const PrepTd3Args &T, const int role, const int l, const shems_group_hparams *hp)
{
    const int tid = threadIdx.x;
    const int64_t off = (int64_t)l * T.p.gstride;
    if (role < 5) {
        prep_body<HP>(T.p, role, l, hp);
        if (role == 0 && tid < BP) {             // (thread m wrote every row of column m itself)
            const float *ws = gsh(T.p.d.ws, off);
            float *ws2 = gsh(T.ws2, off);
            float v[W1K];
#pragma unroll
            for (int k = 0; k < W1K; ++k) v[k] = ws[TP_X + k * BP + tid];
#pragma unroll
            for (int k = 0; k < W1K; ++k) ws2[TP_X + k * BP + tid] = v[k];
        }
        return;
    }
    PrepArgs A = T.p;
    A.d.critic = T.critic2; A.d.critic_t = T.critic2_t; A.d.ws = T.ws2;
    prep_body<HP>(A, 1 + (role == 5 ? NET_CRITIC_T : NET_CRITIC), l, hp);
    if (role == 5) {
        const float *c2 = gsh(T.critic2, off), *c2t = gsh(T.critic2_t, off);
        float *ws2 = gsh(T.ws2, off);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int e = it * 256 + tid, n = e >> 1, o = e & 1;
            const float wc = c2[off_w3(CIN) + min(n, H2N - 1)];
            ws2[TP_FW3C + e] = (n < H2N && o == 0) ? wc : 0.0f;
        }
        if (tid < 8) ws2[TP_FB3 + tid] = tid == 0 ? c2[off_b3(CIN, 1)] : tid == 1 ? c2t[off_b3(CIN, 1)] : 0.0f;
    }
}
__global__ __launch_bounds__(256) void k_tp_prep_td3(PrepTd3Args T) { prep_td3_body<false>(T, blockIdx.x, blockIdx.y, nullptr); }
__global__ __launch_bounds__(256) void k_tp_prep_td3_hp(PrepTd3Args T, const shems_group_hparams *hp) { prep_td3_body<true>(T, blockIdx.x, blockIdx.y, hp); }

// T2: critic_t(s', a~') | critic2_t(s', a~') | critic2(s, a) on 64-wide n-tiles: fwd_body's SMOOTH instantiation, the twin of k_tp_fwd<false, 2, TL>
struct FwdSmoothArgs { FwdArgs f; TpNoise tn; };
template <bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_tp_fwd_smooth(FwdSmoothArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    fwd_body<false, 2, TL, false, true>(A.f, blockIdx.x, blockIdx.y, smem, nullptr, &A.tn);
}
template <bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_tp_fwd_smooth_hp(FwdSmoothArgs A, const shems_group_hparams *hp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    fwd_body<false, 2, TL, true, true>(A.f, blockIdx.x, blockIdx.y, smem, hp, &A.tn);
}
// T3: a critic's D1 launch with the twin head, the twins of k_tp_d1<CIN, ..> / k_tp_d1_hp<CIN, ..> (one launch per critic)
struct TwinArgs { NetArgs n; TwinX x; };
template <int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1_twin(TwinArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<CIN, KT, TL, false, false, true>(A.n, smem, nullptr, &A.x);
}
template <int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1_twin_hp(TwinArgs A, const shems_group_hparams *hp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<CIN, KT, TL, true, false, true>(A.n, smem, hp, &A.x);
}

// ================================================================================================================================
// Prioritized replay for groups (shems_ddpg_group_update_per_tp; include/shems_hip.h): every learner draws its minibatch
// by priority (shems_per_core.h, steps 1-4 per learner with the Philox key seed + l on kStreamPer), the critic's head is weighted and
// the drawn slots' priorities are written back.  prio [capacity], pmax [1] and the sampler workspace per_ws lie in every learner's slab
// (learner l's at learner 0's + l * gstride).  Nine launches:
//   S  k_tp_per_sample    grid (learners), 1024 threads: steps 1-4 on learner l's arrays -- the arithmetic and summation orders of
//                         k_per_sample (shems_ddpg.hip), whose body this repeats (that kernel keeps its code: its chunk sums are DPP adds,
//                         these the xor butterfly of wave_sum64, the same balanced tree and so the same bits); batch_l from the record
//   P0 k_tp_prep_per      prep_body<.., PER>: role 0 gathers the published slots
//   P1, P2                unchanged
//   P3 k_tp_d1_per        d1_body<.., PER>: the weighted head; the publishing workgroup (kt == 0) writes the priorities back
//   P4 .. P7              unchanged (P4 reads the weighted dq P3 published)
// SHEMS_TP_PER_GIVEN: no S and no write-back (X.prio null); the caller has filled every learner's PW_IDX / PW_W.
// ================================================================================================================================
struct PerGroupSampleArgs {
    float *prio; const float *pmax; float *ws;       // learner 0's
    int64_t gstride, capacity, ring_len, fresh_pos, fresh_count;
    uint64_t seed; uint32_t tick; int batch; float beta;
};
template <bool HP>
__device__ __forceinline__ void per_sample_body(const PerGroupSampleArgs &A, const int l, const shems_group_hparams *hp)
{
    __shared__ float sc[kPerMaxSlots / kPerChunk];          // chunk sums
    __shared__ float sS[kPerMaxSlots / kPerBlock], sC[kPerMaxSlots / kPerBlock];
    __shared__ float sraw[kPerCols];
    __shared__ int slast;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = (int64_t)l * A.gstride;
    float *gprio = gsh(A.prio, off);
    float *gws = gsh(A.ws, off);
    const uint64_t seed = A.seed + (uint64_t)l;             // learner l: Philox key seed + l (prep_body's convention)
    int batch = A.batch;
    if constexpr (HP) batch = hp_batch(hp[l]);
    const int nb = (int)per_blocks(A.ring_len);
    const float pmax = gsh(A.pmax, off)[0];
    // steps 1 + 2a: fresh slots take pmax (stored, and used from the register); every chunk's tree sum
    for (int b0 = 0; b0 < nb; b0 += 32) {                  // eight chunks per wave and round
        float x[8];
        int64_t jj[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            jj[i] = ((int64_t)(b0 + (wave >> 2) + 4 * i) * 4 + (wave & 3)) * kPerChunk + lane;
            x[i] = gprio[min(jj[i], A.ring_len - 1)];                                        // clamped, consumed under the bound below
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool in = jj[i] < A.ring_len;
            if (in && per_fresh(jj[i], A.fresh_pos, A.fresh_count, A.capacity)) { x[i] = pmax; gprio[jj[i]] = pmax; }
            const float s = wave_sum64(in ? x[i] : 0.0f);
            const int c = (b0 + (wave >> 2) + 4 * i) * 4 + (wave & 3);
            if (lane == 0 && c < 4 * nb) sc[c] = s;
        }
    }
    __syncthreads();
    // step 2b: block sums, then the running sums in block order (one thread)
    for (int b = tid; b < nb; b += 1024) sS[b] = per_block_sum(sc[4 * b], sc[4 * b + 1], sc[4 * b + 2], sc[4 * b + 3]);
    __syncthreads();
    if (tid == 0) {
        float run = 0.0f;
        int lastpos = 0;
#pragma unroll 16
        for (int b = 0; b < nb; ++b) {
            const float s = sS[b];
            run = b == 0 ? s : run + s;
            sC[b] = run;
            lastpos = s > 0.0f ? b : lastpos;
        }
        slast = lastpos;
    }
    __syncthreads();
    for (int b = tid; b < nb; b += 1024) { gws[PW_S + b] = sS[b]; gws[PW_S + nb + b] = sC[b]; }
    const float T = sC[nb - 1];
    // steps 3 + 4: one column per thread
    float raw = 0.0f;
    int64_t j = 0;
    float u = 0.0f, tm = 0.0f;
    if (tid < kPerCols) {
        u = per_u(seed, A.tick, tid);
        tm = per_target(tid, u, T, batch);
        int lo = 0, hi = nb;                                        // first b with C_b > t (C never decreases): bisection
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (sC[mid] > tm) hi = mid; else lo = mid + 1; }
        const int b = lo < nb ? lo : slast;
        const float *prio = gprio;
        const int cap = (int)A.capacity, fp = (int)A.fresh_pos, fc = (int)min(A.fresh_count, A.capacity);      // (all <= kPerMaxSlots)
        auto at = [=](int q) { const float v = prio[q]; return per_fresh32(q, fp, fc, cap) ? pmax : v; };
        j = per_search_block(b, b > 0 ? sC[b - 1] : 0.0f, tm, (int)A.ring_len, at);
        raw = per_raw_weight(A.ring_len, at((int)j), T, A.beta);
        sraw[tid] = tid < batch ? raw : 0.0f;
    }
    __syncthreads();
    if (tid < kPerCols) {
        float mx = 0.0f;
        for (int m = 0; m < kPerCols; ++m) mx = fmaxf(mx, sraw[m]);
        const bool live = tid < batch;
        reinterpret_cast<int32_t *>(gws + PW_IDX)[tid] = live ? (int32_t)j : -1;
        gws[PW_W + tid] = live ? raw / mx : 0.0f;
        gws[PW_U + tid] = u;
        gws[PW_TM + tid] = tm;
        if (tid == 0) { gws[PW_T] = T; gws[PW_T + 1] = mx; reinterpret_cast<int32_t *>(gws + PW_T)[2] = nb; gws[PW_T + 3] = 0.0f; }
    }
}
__global__ __launch_bounds__(1024) void k_tp_per_sample(PerGroupSampleArgs A) { per_sample_body<false>(A, blockIdx.x, nullptr); }
__global__ __launch_bounds__(1024) void k_tp_per_sample_hp(PerGroupSampleArgs A, const shems_group_hparams *hp) { per_sample_body<true>(A, blockIdx.x, hp); }

struct PrepPerArgs { PrepArgs p; const float *pw; };
__global__ __launch_bounds__(256) void k_tp_prep_per(PrepPerArgs R) { prep_body<false, false, true>(R.p, blockIdx.x, blockIdx.y, nullptr, nullptr, nullptr, R.pw); }
__global__ __launch_bounds__(256) void k_tp_prep_per_hp(PrepPerArgs R, const shems_group_hparams *hp)
{
    prep_body<true, false, true>(R.p, blockIdx.x, blockIdx.y, hp, nullptr, nullptr, R.pw);
}
// P3 with the weighted head: the twins of k_tp_d1<CIN, ..> / k_tp_d1_hp<CIN, ..>
struct PerD1Args { NetArgs n; PerX x; };
template <int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1_per(PerD1Args A)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<CIN, KT, TL, false, false, false, true>(A.n, smem, nullptr, nullptr, &A.x);
}
template <int KT, bool TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_tp_d1_per_hp(PerD1Args A, const shems_group_hparams *hp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    d1_entry<CIN, KT, TL, true, false, false, true>(A.n, smem, hp, nullptr, &A.x);
}

// (Round 5 also built two ways of running the HBM-bound phases (P4, P7) under the MFMA-bound ones (P1, P2, P5) of OTHER learners: cohorts
// of learners on separate streams, and a launch that runs different phases for different cohorts with their workgroups interleaved.
// Both verified, both measured slower than the plain sequence above (2.11-3.27 ms and 2.17-2.34 ms against 2.08-2.11 ms), both removed:
// profiles/r05_tp_overlap_probe.json.)

// ================================================================================================================================
// Flux order <-> tiled layout of the two networks' layer-2 state (W2, m, v, target): one workgroup per (tile, network, learner).
// TO_TILED writes the pad rows / columns as zeros (the kernels above rely on that and never write them); TO_FLUX skips them.
// ================================================================================================================================
struct LayoutArgs { shems_ddpg d; float *w2t_actor, *w2t_critic; int64_t gstride; };
template <bool TO_TILED>
__global__ __launch_bounds__(256) void k_tp_w2_layout(LayoutArgs A)
{
    const int tid = threadIdx.x, nt = blockIdx.x & 7, kt = blockIdx.x >> 3;
    const bool critic = blockIdx.y == 1;
    const int64_t off = (int64_t)blockIdx.z * A.gstride;
    shems_ddpg d = A.d;
    gshift(d, off);
    float *flux[4] = {critic ? d.m_critic : d.m_actor, critic ? d.v_critic : d.v_actor, critic ? d.critic : d.actor, critic ? d.critic_t : d.actor_t};
    float *tile = gsh(critic ? A.w2t_critic : A.w2t_actor, off) + tl_tile(kt, nt) + 4 * tid;
    const int w2 = off_w2(critic ? CIN : SIN);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int k = 64 * kt + 16 * it + (tid >> 4), n = 64 * nt + 4 * (tid & 15);
        const bool in = k < H1N && n < H2N;
        const int e = w2 + min(k, H1N - 1) * H2N + min(n, H2N - 4);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f32x4 *t4 = reinterpret_cast<f32x4 *>(tile + 1024 * it + a * TL_TILE), *f4 = reinterpret_cast<f32x4 *>(flux[a] + e);
            if constexpr (TO_TILED) *t4 = in ? *f4 : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            else if (in) *f4 = *t4;
        }
    }
}

// ================================================================================================================================
// The evaluation sweep's bookkeeping (run_episodes, DDPG.jl:273-290) for every learner: one workgroup per learner.  score_l = the mean of
// the learner's first `runs` eval returns, summed in ascending order in float64 (a host loop reproduces it bit for bit); strictly better
// than best_score[l] -> best_score / best_run / improved and a Flux-order copy of the actor, s_min and s_max into snapshot row l.  W2
// comes from the actor's p tiles when the group trains on the tiled layout (the Flux-order W2 is stale then), everything else from the
// Flux-order block.  Nothing of the training state is written.
// ================================================================================================================================
struct EvalBestArgs {
    const float *actor, *s_min, *s_max, *w2t;          // learner 0's; w2t: the tiled actor region or null
    int64_t gstride;                                   // bytes between learners' slabs
    int64_t n_actor;                                   // floats of one actor (129 002, or shems_wide_params at the wide size)
    const double *returns; int64_t e_eval; int32_t runs, episode;
    double *score, *best_score; int32_t *best_run; uint8_t *improved;
    float *best; int64_t best_stride;                  // snapshot row l at best + l * best_stride bytes
};
__global__ __launch_bounds__(256) void k_group_eval_best(EvalBestArgs A)
{
    __shared__ int s_imp;
    const int64_t l = blockIdx.x, off = l * A.gstride;
    const int tid = threadIdx.x;
    if (tid == 0) {
        const double *r = A.returns + l * A.e_eval;
        double s = 0.0;
        for (int j = 0; j < A.runs; ++j) s += r[j];    // ascending j: the documented order
        const double score = s / (double)A.runs;
        A.score[l] = score;
        const bool imp = score > A.best_score[l];      // strict (DDPG.jl:282): an equal score keeps the old snapshot
        if (imp) { A.best_score[l] = score; A.best_run[l] = A.episode; }
        A.improved[l] = imp ? 1 : 0;
        s_imp = imp;
    }
    __syncthreads();
    if (!s_imp) return;
    const float *src = gsh(A.actor, off);
    float *dst = reinterpret_cast<float *>(reinterpret_cast<char *>(A.best) + l * A.best_stride);
    const float *tiles = A.w2t ? gsh(A.w2t, off) + TL_P * TL_TILE : nullptr;
    const int64_t w2 = off_w2(SIN), w2_end = w2 + (int64_t)H1N * H2N;
    const int64_t n4 = A.n_actor >> 2;
    // float4 pieces: W2 starts on a multiple of 4 and its rows are 500 wide, so a piece lies inside W2 or outside it, and inside it four
    // adjacent columns of one row of one 64 x 64 tile
    for (int64_t q = tid; q < n4; q += 256) {
        const int64_t e = 4 * q;
        f32x4 v;
        if (tiles && e >= w2 && e < w2_end) {
            const int k = (int)((e - w2) / H2N), n = (int)((e - w2) % H2N);
            v = *reinterpret_cast<const f32x4 *>(tiles + tl_tile(k >> 6, n >> 6) + (k & 63) * 64 + (n & 63));
        } else {
            v = *reinterpret_cast<const f32x4 *>(src + e);
        }
        *reinterpret_cast<f32x4 *>(dst + e) = v;
    }
    for (int64_t e = 4 * n4 + tid; e < A.n_actor; e += 256) dst[e] = src[e];     // the tail (b3) is never W2
    const int64_t o_min = (A.n_actor + 3) & ~(int64_t)3;
    if (tid < SHEMS_NSTATE) {
        dst[o_min + tid] = gsh(A.s_min, off)[tid];
        dst[o_min + 16 + tid] = gsh(A.s_max, off)[tid];
    }
}

}  // namespace tp
}  // namespace shems

using namespace shems;
using namespace shems::tp;

static int check_w2t(const shems_group_w2t *t, const char *fn)
{
    if (!t || !t->actor || !t->critic) return set_error(SHEMS_ERR_ARG, "%s: shems_group_w2t needs both regions", fn);
    if ((((uintptr_t)t->actor | (uintptr_t)t->critic) & 15) != 0) return set_error(SHEMS_ERR_ARG, "%s: the tiled regions must be 16-byte aligned", fn);
    return SHEMS_OK;
}
static int check_group_tp(const shems_group *g, const char *fn)
{
    if (!g || g->count < 1 || g->count > 65535 || g->stride_bytes < 0 || (g->stride_bytes & 15) != 0 || (g->count > 1 && g->stride_bytes == 0))
        return set_error(SHEMS_ERR_ARG, "%s: shems_group needs 1 <= count <= 65535 and a 16-byte-multiple stride", fn);
    return SHEMS_OK;
}

// ================================================================================================================================
// Host side of the throughput form: one launch plan behind the entry points
// ================================================================================================================================
// Every entry point below reads: its own checks -> check_tp -> tp_ctx, jobs and records -> the phase launchers in the order of the
// P0 .. P7 list at the top of this file.  A check, a job, a record and a launch shape (grid, LDS, the narrow / wide choice) are each
// written once, here.

struct TpAdam { double eta, bp1, bp2; };       // one network's ADAM scalars as the entry points take them (eta = 0 with records: the
                                               // *_hp kernels form k1 from the records; the host context's k1 is never read by them)

// What every throughput entry point refuses, with nothing launched.  crit / act: the scalars of the halves the call updates, null for a
// half it leaves alone -- the supervised update needs no critic, the critic-only update no actor moments; every call reads the actor and
// its target.  hp null: d->batch is the batch; t null: Flux order.  The two half updates word their STORE_GRAD and ring refusals in their
// own way.
static int check_tp(const char *fn, const shems_ddpg *d, const shems_group *g, const shems_group_w2t *t, const shems_group_hparams *hp,
                    const shems_replay *ring, int64_t ring_len, int32_t flags, int32_t flags_ok, const TpAdam *crit, const TpAdam *act)
{
    const bool both = crit && act;
    if (int rc = check_group_tp(g, fn)) return rc;
    if (!d || !d->actor || !d->actor_t || !d->s_min || !d->s_max || !d->ws || !d->losses || (act && (!d->m_actor || !d->v_actor)) ||
        (crit && (!d->critic || !d->critic_t || !d->m_critic || !d->v_critic)))
        return set_error(SHEMS_ERR_ARG, "%s: shems_ddpg has a NULL buffer", fn);
    if ((flags & SHEMS_TP_STORE_GRAD) && ((act && !d->grad_actor) || (crit && !d->grad_critic)))
        return set_error(SHEMS_ERR_ARG, both ? "%s: STORE_GRAD needs gradient buffers" : "%s: STORE_GRAD needs the gradient buffer", fn);
    if (flags & ~flags_ok) return set_error(SHEMS_ERR_ARG, "%s: unknown flag bits", fn);
    if (!hp && (d->batch < 1 || d->batch > BP)) return set_error(SHEMS_ERR_ARG, "%s: batch must be in 1..128 (got %d)", fn, d->batch);
    if (((uintptr_t)hp & 7) != 0) return set_error(SHEMS_ERR_ARG, "%s: d_hp must be an 8-byte aligned device array of count records", fn);
    const float *const aligned[] = {d->actor, d->actor_t, d->ws, crit ? d->critic : nullptr, crit ? d->critic_t : nullptr};
    for (const float *p : aligned)
        if (((uintptr_t)p & 15) != 0) return set_error(SHEMS_ERR_ARG, "%s: parameter blocks and the workspace must be 16-byte aligned", fn);
    if (int rc = w2t_flux_guard(d->actor, fn)) return rc;       // (a single learner's own tiled mode, shems_ddpg_tiled_enter: not a group's t)
    const bool arrays = ring && ring->s && ring->a && (!crit || (ring->r && ring->s2 && ring->done));
    if (!arrays && !both)
        return set_error(SHEMS_ERR_ARG, crit ? "%s: the ring needs s, a, r, s2 and done" : "%s: the demonstration ring needs s and a", fn);
    if (!arrays || ring_len < 1 || ring_len > ring->capacity)
        return set_error(SHEMS_ERR_ARG, both ? "%s: bad replay ring / length" : "%s: bad ring length", fn);
    for (const TpAdam *a : {crit, act})
        if (a && !(a->bp1 > 0.0 && a->bp1 < 1.0 && a->bp2 > 0.0 && a->bp2 < 1.0)) return set_error(SHEMS_ERR_ARG, "%s: beta powers must be in (0,1)", fn);
    if (t) if (int rc = check_w2t(t, fn)) return rc;
    return SHEMS_OK;
}

// One call's launch context.  Few learners (narrow): the shapes with twice the workgroups (P1 on 64-wide n-tiles, P3 / P6 on 32-wide
// k-tiles).  Below kNarrowBelow learners the wide shapes leave CUs without work (P3 at 32 learners: 128 workgroups); measured per grouped
// update, wide / narrow: 32 learners 247 / 226 us, 48 learners 322 / 320, 64 learners 362 / 372, 128 learners 669 / 695
// (profiles/NOTES.md, round-5 log).
struct TpCtx {
    hipStream_t st;
    unsigned L;                            // learners: grid y
    int64_t gs;                            // slab stride in bytes, 0 for one learner
    int sg, batch;                         // STORE_GRAD; d->batch (the *_hp kernels read the records' instead)
    bool narrow;
    unsigned g8;                           // learners rounded up to eight: the D1 grids
    float *ws, *ta, *tc;                   // learner 0's workspace; the tiled regions of actor and critic, null in Flux order
    const shems_group_hparams *hp;         // the records the *_hp twins read, null without
};
static TpCtx tp_ctx(const shems_ddpg *d, const shems_group *g, const shems_group_w2t *t, const shems_group_hparams *hp, int32_t flags, void *stream)
{
    const unsigned L = (unsigned)g->count;
    return TpCtx{(hipStream_t)stream, L, g->count > 1 ? g->stride_bytes : 0, (flags & SHEMS_TP_STORE_GRAD) ? 1 : 0, d->batch, L < kNarrowBelow,
                 8 * ((L + 7) / 8), d->ws, t ? t->actor : nullptr, t ? t->critic : nullptr, hp};
}
// the plain kernel, or with HP its *_hp twin with the context's records appended: the same launches, each reading its learner's record
template <bool HP, class K, class KH, class A>
static void launch(const TpCtx &c, K plain, KH twin, dim3 grid, unsigned lds, const A &args)
{
    if constexpr (HP) hipLaunchKernelGGL(twin, grid, dim3(256), lds, c.st, args, c.hp);
    else hipLaunchKernelGGL(plain, grid, dim3(256), lds, c.st, args);
}
// f(TL, HP), the two as std::true_type / false_type: the <TL, HP> instantiation of a call's launches -- with (t) or without tiled regions,
// with (hp) or without per-learner records
template <class F>
static int pick(bool tl, bool hp, F f)
{
    using Y = std::true_type;
    using N = std::false_type;
    return tl ? (hp ? f(Y{}, Y{}) : f(Y{}, N{})) : (hp ? f(N{}, Y{}) : f(N{}, N{}));
}

// ---- jobs and records -------------------------------------------------------------------------------------------------------------------
// ws: the learner's workspace (the sampled batch, the actor's passes, the frozen b3).  wn: the workspace that holds the job's own network
// images and partial sums -- ws again, or ws2 for TD3's second critic.  region: the network's tiled region, null in Flux order.
static const float *arr(float *region, int a) { return region ? region + a * TL_TILE : nullptr; }
static FwdJob job_actor_target(float *ws, float *ta, const float *actor_t)         // P1: actor_target(s')
{
    return FwdJob{arr(ta, TL_T), actor_t, ws + TP_X2, w1i_of(ws, NET_ACTOR_T), nullptr, nullptr, nullptr, nullptr, p3_of(ws, NET_ACTOR_T), nullptr, SIN, 2};
}
static FwdJob job_critic(float *ws, float *wn, float *tc, const float *critic)     // P1: critic(s, a)
{
    return FwdJob{arr(tc, TL_P), critic, ws + TP_X, w1i_of(wn, NET_CRITIC), nullptr, nullptr, nullptr, wn + TP_H2C, p3_of(wn, NET_CRITIC), nullptr, CIN, 1};
}
static FwdJob job_actor(float *ws, float *ta, const float *actor)                  // P1: actor(s)
{
    return FwdJob{arr(ta, TL_P), actor, ws + TP_X, w1i_of(ws, NET_ACTOR), nullptr, nullptr, nullptr, ws + TP_H2A, p3_of(ws, NET_ACTOR), nullptr, SIN, 2};
}
// P2: critic_target on [s'; actor_target(s')]; publish: where n-tile 0 leaves the action it computed (TD3's first target critic), or null
static FwdJob job_critic_target(float *ws, float *wn, float *tc, const float *critic_t, float *publish)
{
    return FwdJob{arr(tc, TL_T), critic_t, ws + TP_X2, w1i_of(wn, NET_CRITIC_T), p3_of(ws, NET_ACTOR_T), ws + TP_FB3 + 4, publish, nullptr,
                  p3_of(wn, NET_CRITIC_T), nullptr, CIN, 1};
}
static FwdJob job_critic_new(float *ws, float *tc, const float *critic)            // P5: updated critic on [s; actor(s)], forward + input gradient
{
    return FwdJob{arr(tc, TL_P), critic, ws + TP_X, w1i_of(ws, IMG_CRITIC_NEW), p3_of(ws, NET_ACTOR), ws + TP_FB3 + 2, ws + TP_API, nullptr,
                  p3_of(ws, PASS_CRITIC2), ws + TP_DAP, CIN, 1};
}
static FwdArgs fwd_args(const TpCtx &c, std::initializer_list<FwdJob> jobs)         // up to three jobs; the unused slots stay zero
{
    FwdArgs f{};
    int i = 0;
    for (const FwdJob &j : jobs) f.job[i++] = j;
    f.gstride = c.gs;
    f.batch = c.batch;
    return f;
}
static FwdArgs fwd_p1(const TpCtx &c, const shems_ddpg &d)                          // P1's three jobs; a launch of fewer takes the first ones
{
    return fwd_args(c, {job_actor_target(c.ws, c.ta, d.actor_t), job_critic(c.ws, c.ws, c.tc, d.critic), job_actor(c.ws, c.ta, d.actor)});
}
static FwdArgs fwd_p2(const TpCtx &c, const shems_ddpg &d) { return fwd_args(c, {job_critic_target(c.ws, c.ws, c.tc, d.critic_t, nullptr)}); }
static AdamCtx adam_ctx(const shems_ddpg &d, bool critic, const TpAdam &a)
{
    AdamCtx c{d.actor, d.grad_actor, d.m_actor, d.v_actor, d.actor_t, nullptr, SHEMS_ACTOR_PARAMS, (int)SIN,
              a.eta, a.bp1, a.bp2, 1.0, a.eta / (1.0 - a.bp1), 1.0 / (1.0 - a.bp2), d.tau};
    if (critic) { c.p = d.critic; c.g = d.grad_critic; c.mt = d.m_critic; c.vt = d.v_critic; c.target = d.critic_t; c.n = SHEMS_CRITIC_PARAMS; c.in = CIN; }
    return c;
}
// the record of the launches that differentiate d's critic (P3 / P4: loss head 1) or actor (P6 / P7: head 2); region: its tiled region
static NetArgs net_args(const TpCtx &c, const shems_ddpg &d, float *region, bool critic, const TpAdam &a)
{
    return NetArgs{d, region, adam_ctx(d, critic, a), c.gs, critic ? 1 : 2, c.sg, (int)c.L};
}

// ---- phase launchers --------------------------------------------------------------------------------------------------------------------
typedef FwdShape<false, 4> SW;
typedef FwdShape<false, 2> SN;
typedef FwdShape<true, 2> SQ;
template <bool TL, bool HP>
static void launch_p1(const TpCtx &c, const FwdArgs &f, unsigned jobs)               // P1: `jobs` independent forward passes
{
    if (c.narrow) launch<HP>(c, k_tp_fwd<false, 2, TL>, k_tp_fwd_hp<false, 2, TL>, dim3(jobs * SN::TILES, c.L), SN::LDS, f);
    else launch<HP>(c, k_tp_fwd<false, 4, TL>, k_tp_fwd_hp<false, 4, TL>, dim3(jobs * SW::TILES, c.L), SW::LDS, f);
}
template <bool TL, bool HP>
static void launch_p2(const TpCtx &c, const FwdArgs &f)                              // P2: one forward pass on the narrow shape
{
    launch<HP>(c, k_tp_fwd<false, 2, TL>, k_tp_fwd_hp<false, 2, TL>, dim3(SN::TILES, c.L), SN::LDS, f);
}
// P3 / P6 for a kernel family (k_tp_d1, _clone, _twin, _per), given at 32-wide (k1*) and at 64-wide (k2*) k-tiles
template <bool HP, class K, class KH, class A>
static void launch_d1(const TpCtx &c, K k1, KH k1_hp, K k2, KH k2_hp, const A &args)
{
    if (c.narrow) launch<HP>(c, k1, k1_hp, dim3(8 * c.g8), d1_lds(1), args);
    else launch<HP>(c, k2, k2_hp, dim3(4 * c.g8), d1_lds(2) + SHEMS_D1_PAD, args);
}
template <int IN, bool TL, bool HP>
static void launch_d1_net(const TpCtx &c, const NetArgs &n)                          // ... with the DDPG heads: the critic's P3, the actor's P6
{
    launch_d1<HP>(c, k_tp_d1<IN, 1, TL>, k_tp_d1_hp<IN, 1, TL>, k_tp_d1<IN, 2, TL>, k_tp_d1_hp<IN, 2, TL>, n);
}
template <int IN, bool TL, bool HP>
static void launch_gw2(const TpCtx &c, const NetArgs &n)                             // P4 / P7
{
    launch<HP>(c, k_tp_gw2<IN, TL>, k_tp_gw2_hp<IN, TL>, dim3(GW_WGS, c.L), GW_LDS, n);
}
template <bool TL, bool HP>
static void launch_actor_half(const TpCtx &c, const shems_ddpg &d, const TpAdam &act)          // P5, P6, P7
{
    const FwdArgs f5 = fwd_args(c, {job_critic_new(c.ws, c.tc, d.critic)});
    const NetArgs na = net_args(c, d, c.ta, false, act);
    launch<HP>(c, k_tp_fwd<true, 2, TL>, k_tp_fwd_hp<true, 2, TL>, dim3(SQ::TILES, c.L), SQ::LDS, f5);
    launch_d1_net<SIN, TL, HP>(c, na);
    launch_gw2<SIN, TL, HP>(c, na);
}

// ---- the DDPG update: P0 .. P7 ------------------------------------------------------------------------------------------------------------
// t == null: every array in Flux order (round 5's form); else the layer-2 state of both networks lives in the tiled regions.
// hp: learner l's batch / gamma / tau / eta from hp[l] (device), the *_hp kernels; d->batch / gamma / tau and eta_* are not used.
// xp / pushed (shems_ddpg_group_update_tp_x, with hp): per-learner ring lengths on the device; ring_len is not used then.
static int ddpg_update_tp(const char *fn, const shems_ddpg *d, const shems_replay *ring, const shems_group *g, const shems_group_w2t *t,
                          const shems_group_hparams *hp, const shems_group_xparams *xp, const int64_t *pushed, int64_t ring_len, uint64_t seed,
                          uint32_t tick, const TpAdam &crit, const TpAdam &act, int32_t flags, void *stream)
{
    if (xp && (((uintptr_t)xp | (uintptr_t)pushed) & 7) != 0)
        return set_error(SHEMS_ERR_ARG, "%s: d_xp and d_pushed must be 8-byte aligned device arrays of count records", fn);
    if (int rc = check_tp(fn, d, g, t, hp, ring, ring_len, flags, SHEMS_TP_STORE_GRAD, &crit, &act)) return rc;
    const TpCtx c = tp_ctx(d, g, t, hp, flags, stream);
    const PrepArgs pa{*d, *ring, ring_len, c.gs, seed, tick};
    const FwdArgs f1 = fwd_p1(c, *d), f2 = fwd_p2(c, *d);
    const NetArgs nc = net_args(c, *d, c.tc, true, crit);
    return pick(t, hp, [&](auto tl, auto rec) {
        constexpr bool TL = decltype(tl)::value, HP = decltype(rec)::value;
        if (HP && xp) hipLaunchKernelGGL(k_tp_prep_x, dim3(5, c.L), dim3(256), 0, c.st, pa, hp, xp, pushed);
        else launch<HP>(c, k_tp_prep, k_tp_prep_hp, dim3(5, c.L), 0, pa);
        launch_p1<TL, HP>(c, f1, 3);
        launch_p2<TL, HP>(c, f2);
        launch_d1_net<CIN, TL, HP>(c, nc);
        launch_gw2<CIN, TL, HP>(c, nc);
        launch_actor_half<TL, HP>(c, *d, act);
        return hip_ok(hipGetLastError(), HP ? "grouped update (throughput form, per-learner hyper-parameters) launches" : "grouped update (throughput form) launches");
    });
}

extern "C" int shems_ddpg_group_update_tp(const shems_ddpg *d, const shems_replay *ring, const shems_group *g, const shems_group_w2t *t,
                                          const shems_group_hparams *d_hp, int64_t ring_len, uint64_t seed, uint32_t tick, double eta_crit,
                                          double bp1_crit, double bp2_crit, double eta_act, double bp1_act, double bp2_act, int32_t flags, void *stream)
{
    return ddpg_update_tp("shems_ddpg_group_update_tp", d, ring, g, t, d_hp, nullptr, nullptr, ring_len, seed, tick,
                          TpAdam{d_hp ? 0.0 : eta_crit, bp1_crit, bp2_crit}, TpAdam{d_hp ? 0.0 : eta_act, bp1_act, bp2_act}, flags, stream);
}

extern "C" int shems_ddpg_group_update_tp_x(const shems_ddpg *d, const shems_replay *ring, const shems_group *g, const shems_group_w2t *t,
                                            const shems_group_hparams *d_hp, const shems_group_xparams *d_xp, const int64_t *d_pushed, uint64_t seed,
                                            uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit, double eta_act, double bp1_act,
                                            double bp2_act, int32_t flags, void *stream)
{
    if (!d_hp || !d_xp || !d_pushed) return set_error(SHEMS_ERR_ARG, "shems_ddpg_group_update_tp_x: d_hp, d_xp and d_pushed are all required");
    return ddpg_update_tp("shems_ddpg_group_update_tp_x", d, ring, g, t, d_hp, d_xp, d_pushed, 1, seed, tick, TpAdam{0.0, bp1_crit, bp2_crit},
                          TpAdam{0.0, bp1_act, bp2_act}, flags, stream);
}

// ---- the grouped supervised update (clone) and the grouped critic-only update: subsets of the launches above ------------------------
//   clone   sampler | P1 with the actor(s) job alone | the actor's D1 with the cloning head | the actor's gW2
//   else    sampler | P1 with the actor_target(s') and critic(s, a) jobs | P2 | P3 | P4 -- the update's own kernels on the update's own
//           inputs: the critic half of the DDPG update, bit for bit
// The ring is learner 0's arrays + l * ring_stride bytes (its own stride: the rings need not live in the slabs).
static int half_update_tp(bool clone, const shems_ddpg *d, const shems_replay *ring, int64_t ring_stride, const shems_group *g, const shems_group_w2t *t,
                          const shems_group_hparams *hp, int64_t ring_len, uint64_t seed, uint32_t tick, const TpAdam &adam, int32_t flags, void *stream)
{
    const char *fn = clone ? "shems_ddpg_group_clone_update_tp" : "shems_ddpg_group_critic_update_tp";
    if (int rc = check_tp(fn, d, g, t, hp, ring, ring_len, flags, SHEMS_TP_STORE_GRAD, clone ? nullptr : &adam, clone ? &adam : nullptr)) return rc;
    if (ring_stride < 0 || (ring_stride & 3) != 0 || (g->count > 1 && ring_stride == 0))
        return set_error(SHEMS_ERR_ARG, "%s: bad ring stride %lld: a non-negative multiple of 4 bytes, and not 0 for more than one learner", fn,
                         (long long)ring_stride);
    const TpCtx c = tp_ctx(d, g, t, hp, flags, stream);
    const PrepRingArgs pa{PrepArgs{*d, *ring, ring_len, c.gs, seed, tick}, g->count > 1 ? ring_stride : 0};
    const FwdArgs f1 = clone ? fwd_args(c, {job_actor(c.ws, c.ta, d->actor)}) : fwd_p1(c, *d);
    const NetArgs n = net_args(c, *d, clone ? c.ta : c.tc, !clone, adam);
    return pick(t, hp, [&](auto tl, auto rec) {
        constexpr bool TL = decltype(tl)::value, HP = decltype(rec)::value;
        if (clone) {
            launch<HP>(c, k_tp_prep_ring<true>, k_tp_prep_ring_hp<true>, dim3(2, c.L), 0, pa);
            launch_p1<TL, HP>(c, f1, 1);
            launch_d1<HP>(c, k_tp_d1_clone<1, TL>, k_tp_d1_clone_hp<1, TL>, k_tp_d1_clone<2, TL>, k_tp_d1_clone_hp<2, TL>, n);
            launch_gw2<SIN, TL, HP>(c, n);
            return hip_ok(hipGetLastError(), "grouped supervised update (throughput form) launches");
        }
        launch<HP>(c, k_tp_prep_ring<false>, k_tp_prep_ring_hp<false>, dim3(5, c.L), 0, pa);
        launch_p1<TL, HP>(c, f1, 2);
        launch_p2<TL, HP>(c, fwd_p2(c, *d));
        launch_d1_net<CIN, TL, HP>(c, n);
        launch_gw2<CIN, TL, HP>(c, n);
        return hip_ok(hipGetLastError(), "grouped critic-only update (throughput form) launches");
    });
}
extern "C" int shems_ddpg_group_clone_update_tp(const shems_ddpg *d, const shems_replay *ring, int64_t ring_stride_bytes, const shems_group *g,
                                                const shems_group_w2t *t, const shems_group_hparams *d_hp, int64_t ring_len, uint64_t seed,
                                                uint32_t tick, double eta, double bp1, double bp2, int32_t flags, void *stream)
{
    return half_update_tp(true, d, ring, ring_stride_bytes, g, t, d_hp, ring_len, seed, tick, TpAdam{d_hp ? 0.0 : eta, bp1, bp2}, flags, stream);
}
extern "C" int shems_ddpg_group_critic_update_tp(const shems_ddpg *d, const shems_replay *ring, int64_t ring_stride_bytes, const shems_group *g,
                                                 const shems_group_w2t *t, const shems_group_hparams *d_hp, int64_t ring_len, uint64_t seed,
                                                 uint32_t tick, double eta, double bp1, double bp2, int32_t flags, void *stream)
{
    return half_update_tp(false, d, ring, ring_stride_bytes, g, t, d_hp, ring_len, seed, tick, TpAdam{d_hp ? 0.0 : eta, bp1, bp2}, flags, stream);
}

// ---- TD3 for groups: seven launches, ten on a policy step -----------------------------------------------------------------------------
//   sampler k_tp_prep_td3 | T1 = P1 (actor(s) job on a policy step only) | T2 k_tp_fwd_smooth | T3 k_tp_d1_twin for critic 1, again for
//   critic 2 | T4 k_tp_gw2<CIN> for critic 1, again for critic 2 | policy step: P5, P6, P7.
// Off a policy step the critic launches run with tau = 0 (1 t + 0 p: the targets keep their bytes): d->tau = 0 in their records, or
// hp_hold (the records with tau = 0) in the place of hp.
extern "C" int shems_td3_group_workspace_floats(int64_t *out)
{
    if (!out) return set_error(SHEMS_ERR_ARG, "shems_td3_group_workspace_floats: NULL");
    *out = T2_FLOATS;
    return SHEMS_OK;
}

// what shems_td3_group_update_tp refuses beyond check_tp: the second critic's blocks, the schedule and the smoothing noise
static int check_td3_group(const char *fn, const shems_td3 *t0, const shems_group_w2t *t, const float *w2t_critic2, const shems_group_hparams *hp,
                           const shems_group_hparams *hp_hold, int update_policy, int32_t flags)
{
    const shems_ddpg *d = &t0->d;
    if (!t0->critic2 || !t0->critic2_t || !t0->m_critic2 || !t0->v_critic2 || !t0->ws2 || !t0->losses2)
        return set_error(SHEMS_ERR_ARG, "%s: shems_td3 has a NULL critic-2 buffer", fn);
    if ((flags & SHEMS_TP_STORE_GRAD) && !t0->grad_critic2) return set_error(SHEMS_ERR_ARG, "%s: STORE_GRAD needs gradient buffers", fn);
    if (update_policy != 0 && update_policy != 1) return set_error(SHEMS_ERR_ARG, "%s: update_policy must be 0 or 1 (got %d)", fn, update_policy);
    if (!(t0->sigma_trg >= 0.0f) || !(t0->clip_trg >= 0.0f) || t0->sigma_trg > 3.0e38f || t0->clip_trg > 3.0e38f)
        return set_error(SHEMS_ERR_ARG, "%s: sigma_trg and clip_trg must be finite and >= 0", fn);
    if (hp && !update_policy && !hp_hold)
        return set_error(SHEMS_ERR_ARG, "%s: update_policy = 0 with d_hp needs d_hp_hold (the records with tau = 0)", fn);
    for (const float *p : {(const float *)t0->critic2, (const float *)t0->critic2_t, (const float *)t0->m_critic2, (const float *)t0->v_critic2,
                           (const float *)t0->ws2})
        if (((uintptr_t)p & 15) != 0) return set_error(SHEMS_ERR_ARG, "%s: critic-2 blocks and ws2 must be 16-byte aligned", fn);
    if (((uintptr_t)t0->grad_critic2 & 15) != 0 || ((uintptr_t)t0->losses2 & 3) != 0)
        return set_error(SHEMS_ERR_ARG, "%s: grad_critic2 must be 16-byte and losses2 float aligned", fn);
    const float *one[5] = {d->critic, d->critic_t, d->m_critic, d->v_critic, d->grad_critic};
    const float *two[5] = {t0->critic2, t0->critic2_t, t0->m_critic2, t0->v_critic2, t0->grad_critic2};
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
            if (two[i] && one[j] && two[i] < one[j] + SHEMS_CRITIC_PARAMS && one[j] < two[i] + SHEMS_CRITIC_PARAMS)
                return set_error(SHEMS_ERR_ARG, "%s: a critic-2 buffer overlaps one of critic 1's", fn);
            if (i < j && two[i] && two[j] && two[i] < two[j] + SHEMS_CRITIC_PARAMS && two[j] < two[i] + SHEMS_CRITIC_PARAMS)
                return set_error(SHEMS_ERR_ARG, "%s: two critic-2 buffers overlap", fn);
        }
    if (t0->ws2 < d->ws + TP_FLOATS && d->ws < t0->ws2 + T2_FLOATS) return set_error(SHEMS_ERR_ARG, "%s: ws2 overlaps ws", fn);
    if (t0->losses2 < d->losses + 2 && d->losses < t0->losses2 + 1) return set_error(SHEMS_ERR_ARG, "%s: losses2 overlaps losses", fn);
    if (t) {
        if (((uintptr_t)w2t_critic2 & 15) != 0) return set_error(SHEMS_ERR_ARG, "%s: the tiled regions must be 16-byte aligned", fn);
        if (w2t_critic2 < t->critic + SHEMS_W2T_FLOATS && t->critic < w2t_critic2 + SHEMS_W2T_FLOATS)
            return set_error(SHEMS_ERR_ARG, "%s: critic 2's tiled region overlaps critic 1's", fn);
        if (w2t_critic2 < t->actor + SHEMS_W2T_FLOATS && t->actor < w2t_critic2 + SHEMS_W2T_FLOATS)
            return set_error(SHEMS_ERR_ARG, "%s: critic 2's tiled region overlaps the actor's", fn);
    }
    return SHEMS_OK;
}

extern "C" int shems_td3_group_update_tp(const shems_td3 *t0, const shems_replay *ring0, const shems_group *g, const shems_group_w2t *w,
                                         float *w2t_critic2, const shems_group_hparams *d_hp, const shems_group_hparams *d_hp_hold, int64_t ring_len,
                                         uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit, double eta_act,
                                         double bp1_act, double bp2_act, int update_policy, int32_t flags, void *stream)
{
    const char *fn = "shems_td3_group_update_tp";
    if (!t0) return set_error(SHEMS_ERR_ARG, "shems_td3_group_update_tp: NULL");
    if ((w != nullptr) != (w2t_critic2 != nullptr))
        return set_error(SHEMS_ERR_ARG, "shems_td3_group_update_tp: the tiled layout needs w AND w2t_critic2 (or neither: Flux order)");
    if (d_hp && (((uintptr_t)d_hp | (uintptr_t)d_hp_hold) & 7) != 0)
        return set_error(SHEMS_ERR_ARG, "%s: d_hp and d_hp_hold must be 8-byte aligned device arrays of count records", fn);
    const shems_ddpg *d = &t0->d;
    const TpAdam crit{d_hp ? 0.0 : eta_crit, bp1_crit, bp2_crit}, act{d_hp ? 0.0 : eta_act, bp1_act, bp2_act};
    if (int rc = check_tp(fn, d, g, w, d_hp, ring0, ring_len, flags, SHEMS_TP_STORE_GRAD, &crit, &act)) return rc;
    if (int rc = check_td3_group(fn, t0, w, w2t_critic2, d_hp, d_hp_hold, update_policy, flags)) return rc;
    const TpCtx c = tp_ctx(d, g, w, d_hp, flags, stream);
    TpCtx cc = c;                            // the critic launches' context: off a policy step their records are the held ones
    if (!update_policy) cc.hp = d_hp_hold;
    float *ws = c.ws, *ws2 = t0->ws2, *tc2 = w2t_critic2;
    // the records of the critic launches: critic 2's names critic 2's blocks, ws2 and losses2; off a policy step both hold tau = 0
    shems_ddpg d1 = *d, d2 = *d;
    d2.critic = t0->critic2; d2.critic_t = t0->critic2_t; d2.m_critic = t0->m_critic2; d2.v_critic = t0->v_critic2;
    d2.grad_critic = t0->grad_critic2; d2.ws = ws2; d2.losses = t0->losses2;
    if (!update_policy) d1.tau = d2.tau = 0.0f;
    const PrepTd3Args pa{PrepArgs{*d, *ring0, ring_len, c.gs, seed, tick}, t0->critic2, t0->critic2_t, ws2};
    const FwdArgs f1 = fwd_p1(c, *d);
    // T2: both target critics on [s'; a~'] (the first publishes a~'), critic 2 on [s; a]
    const FwdSmoothArgs f2{fwd_args(c, {job_critic_target(ws, ws, c.tc, d->critic_t, ws2 + T2_AT), job_critic_target(ws, ws2, tc2, t0->critic2_t, nullptr),
                                        job_critic(ws, ws2, tc2, t0->critic2)}),
                           TpNoise{seed, tick, t0->sigma_trg, t0->clip_trg}};
    const TwinArgs n1{net_args(c, d1, c.tc, true, crit), TwinX{ws, ws2, ws2 + T2_PUB}}, n2{net_args(c, d2, tc2, true, crit), TwinX{ws, ws2, ws2 + T2_PUB2}};
    return pick(w, d_hp, [&](auto tl, auto rec) {
        constexpr bool TL = decltype(tl)::value, HP = decltype(rec)::value;
        launch<HP>(c, k_tp_prep_td3, k_tp_prep_td3_hp, dim3(7, c.L), 0, pa);
        launch_p1<TL, HP>(c, f1, update_policy ? 3 : 2);
        launch<HP>(c, k_tp_fwd_smooth<TL>, k_tp_fwd_smooth_hp<TL>, dim3(3 * SN::TILES, c.L), SN::LDS, f2);
        for (const TwinArgs *n : {&n1, &n2}) launch_d1<HP>(cc, k_tp_d1_twin<1, TL>, k_tp_d1_twin_hp<1, TL>, k_tp_d1_twin<2, TL>, k_tp_d1_twin_hp<2, TL>, *n);
        for (const TwinArgs *n : {&n1, &n2}) launch_gw2<CIN, TL, HP>(cc, n->n);
        if (update_policy) launch_actor_half<TL, HP>(c, *d, act);
        return hip_ok(hipGetLastError(), "grouped TD3 update (throughput form) launches");
    });
}

// ---- prioritized replay for groups: S, P0 (k_tp_prep_per), P1, P2, P3 (k_tp_d1_per), P4 .. P7 -----------------------------------------
// The three blocks of learner 0's shems_per against the slab: with more than one learner they must end inside one stride of the lowest
// of `blocks` and of themselves (learner l's copy would otherwise reach into learner l + 1's slab), and overlap none of `blocks`.
struct SlabBlock { const void *p; size_t bytes; };
static int check_per_slab(const shems_per *per, int64_t capacity, const shems_group *g, const SlabBlock *blocks, int nblocks, const char *fn)
{
    const SlabBlock pb[3] = {{per->prio, (size_t)capacity * 4}, {per->pmax, 4}, {per->ws, (size_t)per_ws_floats(capacity) * 4}};
    uintptr_t lo = (uintptr_t)per->prio;
    for (const SlabBlock &b : pb) lo = (uintptr_t)b.p < lo ? (uintptr_t)b.p : lo;
    for (int i = 0; i < nblocks; ++i)
        if (blocks[i].p && (uintptr_t)blocks[i].p < lo) lo = (uintptr_t)blocks[i].p;
    for (const SlabBlock &b : pb) {
        for (int i = 0; i < nblocks; ++i)
            if (blocks[i].p && ranges_overlap(b.p, b.bytes, blocks[i].p, blocks[i].bytes))
                return set_error(SHEMS_ERR_ARG, "%s: the prioritized ring's arrays overlap a block of the learner (DDPG blocks, workspace or ring)", fn);
        if (g->count > 1 && (uintptr_t)b.p + b.bytes > lo + (uintptr_t)g->stride_bytes)
            return set_error(SHEMS_ERR_ARG, "%s: the prioritized ring's arrays run past the slab stride of %lld bytes", fn, (long long)g->stride_bytes);
    }
    return SHEMS_OK;
}
static int per_group_sample_launch(const shems_per *per, const shems_group *g, const shems_group_hparams *hp, int64_t capacity, int64_t ring_len,
                                   int64_t fresh_pos, int64_t fresh_count, uint64_t seed, uint32_t tick, int32_t batch, hipStream_t st)
{
    const PerGroupSampleArgs a{per->prio, per->pmax, per->ws, g->count > 1 ? g->stride_bytes : 0, capacity, ring_len, fresh_pos, fresh_count,
                               seed, tick, batch, per->beta};
    if (hp) hipLaunchKernelGGL(k_tp_per_sample_hp, dim3((unsigned)g->count), dim3(1024), 0, st, a, hp);
    else hipLaunchKernelGGL(k_tp_per_sample, dim3((unsigned)g->count), dim3(1024), 0, st, a);
    return hip_ok(hipGetLastError(), "k_tp_per_sample launch");
}

extern "C" int shems_per_group_sample_dev(const shems_per *per0, const shems_group *g, const shems_group_hparams *d_hp, int64_t capacity,
                                          int64_t ring_len, int64_t fresh_pos, int64_t fresh_count, uint64_t seed, uint32_t tick, int32_t batch,
                                          void *stream)
{
    const char *fn = "shems_per_group_sample_dev";
    if (int rc = check_group_tp(g, fn)) return rc;
    if (d_hp && ((uintptr_t)d_hp & 7) != 0) return set_error(SHEMS_ERR_ARG, "%s: d_hp must be an 8-byte aligned device array of count records", fn);
    const int32_t shown = batch < 1 ? 0 : batch;             // (the refusal names every batch below 1 as 0)
    if (int rc = check_per(per0, capacity, ring_len, fresh_pos, fresh_count, d_hp ? nullptr : &shown, fn)) return rc;
    if (int rc = check_per_slab(per0, capacity, g, nullptr, 0, fn)) return rc;
    return per_group_sample_launch(per0, g, d_hp, capacity, ring_len, fresh_pos, fresh_count, seed, tick, batch, (hipStream_t)stream);
}

extern "C" int shems_ddpg_group_update_per_tp(const shems_ddpg *d, const shems_replay *ring, const shems_group *g, const shems_group_w2t *t,
                                              const shems_group_hparams *d_hp, const shems_per *per, int64_t ring_len, int64_t fresh_pos,
                                              int64_t fresh_count, uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit,
                                              double eta_act, double bp1_act, double bp2_act, int32_t flags, void *stream)
{
    const char *fn = "shems_ddpg_group_update_per_tp";
    const TpAdam crit{d_hp ? 0.0 : eta_crit, bp1_crit, bp2_crit}, act{d_hp ? 0.0 : eta_act, bp1_act, bp2_act};
    if (int rc = check_tp(fn, d, g, t, d_hp, ring, ring_len, flags, SHEMS_TP_STORE_GRAD | SHEMS_TP_PER_GIVEN, &crit, &act)) return rc;
    // the prioritized ring's own arguments, and its blocks against the slab
    if (int rc = check_per(per, ring->capacity, ring_len, fresh_pos, fresh_count, d_hp ? nullptr : &d->batch, fn)) return rc;
    {
        const size_t na = (size_t)SHEMS_ACTOR_PARAMS * 4, nc = (size_t)SHEMS_CRITIC_PARAMS * 4, cap = (size_t)ring->capacity;
        const SlabBlock blocks[] = {
            {d->actor, na}, {d->critic, nc}, {d->actor_t, na}, {d->critic_t, nc}, {d->m_actor, na}, {d->v_actor, na}, {d->m_critic, nc}, {d->v_critic, nc},
            {d->grad_actor, na}, {d->grad_critic, nc}, {d->s_min, SHEMS_NSTATE * 4}, {d->s_max, SHEMS_NSTATE * 4}, {d->ws, (size_t)kTpWsFloats * 4},
            {d->losses, 8}, {ring->s, cap * SHEMS_NSTATE * 4}, {ring->a, cap * 2 * 4}, {ring->r, cap * 4}, {ring->s2, cap * SHEMS_NSTATE * 4},
            {ring->done, cap}, {t ? t->actor : nullptr, (size_t)SHEMS_W2T_FLOATS * 4}, {t ? t->critic : nullptr, (size_t)SHEMS_W2T_FLOATS * 4}};
        if (int rc = check_per_slab(per, ring->capacity, g, blocks, (int)(sizeof blocks / sizeof blocks[0]), fn)) return rc;
    }
    const TpCtx c = tp_ctx(d, g, t, d_hp, flags, stream);
    const bool given = (flags & SHEMS_TP_PER_GIVEN) != 0;
    const PrepPerArgs pa{PrepArgs{*d, *ring, ring_len, c.gs, seed, tick}, per->ws};
    const FwdArgs f1 = fwd_p1(c, *d), f2 = fwd_p2(c, *d);
    const NetArgs nc = net_args(c, *d, c.tc, true, crit);
    const PerD1Args np{nc, PerX{per->ws, given ? nullptr : per->prio, given ? nullptr : per->pmax, ring_len, per->alpha, per->eps_p}};
    if (!given)
        if (int rc = per_group_sample_launch(per, g, d_hp, ring->capacity, ring_len, fresh_pos, fresh_count, seed, tick, d->batch, c.st)) return rc;
    return pick(t, d_hp, [&](auto tl, auto rec) {
        constexpr bool TL = decltype(tl)::value, HP = decltype(rec)::value;
        launch<HP>(c, k_tp_prep_per, k_tp_prep_per_hp, dim3(5, c.L), 0, pa);
        launch_p1<TL, HP>(c, f1, 3);
        launch_p2<TL, HP>(c, f2);
        launch_d1<HP>(c, k_tp_d1_per<1, TL>, k_tp_d1_per_hp<1, TL>, k_tp_d1_per<2, TL>, k_tp_d1_per_hp<2, TL>, np);
        launch_gw2<CIN, TL, HP>(c, nc);
        launch_actor_half<TL, HP>(c, *d, act);
        return hip_ok(hipGetLastError(), "grouped prioritized update (throughput form) launches");
    });
}

static_assert(sizeof(shems_group_xparams) == 16 && offsetof(shems_group_xparams, ou_dt) == 4 && offsetof(shems_group_xparams, mem_size) == 8 &&
              offsetof(shems_group_xparams, reserved) == 12, "shems_group_xparams: 16 bytes, the layout of include/shems_hip.h and group.XParams");
static_assert(sizeof(shems_group_hparams) == 40 && offsetof(shems_group_hparams, gamma) == 16 && offsetof(shems_group_hparams, noise_mu) == 24 &&
              offsetof(shems_group_hparams, batch) == 32, "shems_group_hparams: 40 bytes, the layout of include/shems_hip.h and group.HParams");

static int hparams_check(const char *fn, const shems_group_hparams *hp, int32_t count, int max_batch)
{
    if (!hp || count < 1) return set_error(SHEMS_ERR_ARG, "%s: need count >= 1 records", fn);
    for (int32_t l = 0; l < count; ++l) {
        const shems_group_hparams &h = hp[l];
        if (h.batch < 1 || h.batch > max_batch) return set_error(SHEMS_ERR_ARG, "%s: learner %d: batch %d outside 1..%d", fn, l, h.batch, max_batch);
        if (!(std::isfinite(h.eta_act) && h.eta_act > 0.0)) return set_error(SHEMS_ERR_ARG, "%s: learner %d: eta_act %g must be finite and > 0", fn, l, h.eta_act);
        if (!(std::isfinite(h.eta_crit) && h.eta_crit > 0.0)) return set_error(SHEMS_ERR_ARG, "%s: learner %d: eta_crit %g must be finite and > 0", fn, l, h.eta_crit);
        if (!(h.tau > 0.0f && h.tau <= 1.0f)) return set_error(SHEMS_ERR_ARG, "%s: learner %d: tau %g outside (0, 1]", fn, l, (double)h.tau);
        if (!(h.gamma >= 0.0f && h.gamma <= 1.0f)) return set_error(SHEMS_ERR_ARG, "%s: learner %d: gamma %g outside [0, 1]", fn, l, (double)h.gamma);
        if (!std::isfinite(h.noise_mu)) return set_error(SHEMS_ERR_ARG, "%s: learner %d: noise_mu %g is not finite", fn, l, (double)h.noise_mu);
        if (!(std::isfinite(h.noise_sigma) && h.noise_sigma >= 0.0f))
            return set_error(SHEMS_ERR_ARG, "%s: learner %d: noise_sigma %g must be finite and >= 0", fn, l, (double)h.noise_sigma);
        if (h.reserved != 0) return set_error(SHEMS_ERR_ARG, "%s: learner %d: reserved must be 0", fn, l);
    }
    return SHEMS_OK;
}
extern "C" int shems_group_xparams_check(const shems_group_xparams *xp, int32_t count, int64_t capacity)
{
    const char *fn = "shems_group_xparams_check";
    if (!xp || count < 1) return set_error(SHEMS_ERR_ARG, "%s: need count >= 1 records", fn);
    if (capacity < 1 || capacity > INT32_MAX) return set_error(SHEMS_ERR_ARG, "%s: capacity %lld outside 1..2^31 - 1", fn, (long long)capacity);
    for (int32_t l = 0; l < count; ++l) {
        const shems_group_xparams &x = xp[l];
        if (!(std::isfinite(x.ou_theta) && x.ou_theta >= 0.0f))
            return set_error(SHEMS_ERR_ARG, "%s: learner %d: ou_theta %g must be finite and >= 0", fn, l, (double)x.ou_theta);
        if (!(std::isfinite(x.ou_dt) && x.ou_dt > 0.0f)) return set_error(SHEMS_ERR_ARG, "%s: learner %d: ou_dt %g must be finite and > 0", fn, l, (double)x.ou_dt);
        if (x.mem_size < 1 || x.mem_size > capacity)
            return set_error(SHEMS_ERR_ARG, "%s: learner %d: mem_size %d outside 1..%lld", fn, l, x.mem_size, (long long)capacity);
        if (x.reserved != 0) return set_error(SHEMS_ERR_ARG, "%s: learner %d: reserved must be 0", fn, l);
    }
    return SHEMS_OK;
}
extern "C" int shems_group_hparams_check(const shems_group_hparams *hp, int32_t count)
{
    return hparams_check("shems_group_hparams_check", hp, count, BP);
}
/* the wide group form (shems_wide_group_update): batch in 1..max_batch, max_batch <= 256 */
extern "C" int shems_group_hparams_check_wide(const shems_group_hparams *hp, int32_t count, int32_t max_batch)
{
    if (max_batch < 1 || max_batch > 256)
        return set_error(SHEMS_ERR_ARG, "shems_group_hparams_check_wide: max_batch must be in 1..256 (got %d)", max_batch);
    return hparams_check("shems_group_hparams_check_wide", hp, count, max_batch);
}

static int w2_layout(const char *fn, bool to_tiled, const shems_ddpg *d, const shems_group *g, const shems_group_w2t *t, void *stream)
{
    if (int rc = check_group_tp(g, fn)) return rc;
    if (int rc = check_w2t(t, fn)) return rc;
    if (!d || !d->actor || !d->critic || !d->actor_t || !d->critic_t || !d->m_actor || !d->v_actor || !d->m_critic || !d->v_critic)
        return set_error(SHEMS_ERR_ARG, "%s: shems_ddpg has a NULL network / moment buffer", fn);
    for (const float *p : {(const float *)d->actor, (const float *)d->critic, (const float *)d->actor_t, (const float *)d->critic_t, (const float *)d->m_actor,
                           (const float *)d->v_actor, (const float *)d->m_critic, (const float *)d->v_critic})
        if (((uintptr_t)p & 15) != 0) return set_error(SHEMS_ERR_ARG, "%s: parameter and moment blocks must be 16-byte aligned", fn);
    LayoutArgs A{*d, t->actor, t->critic, g->count > 1 ? g->stride_bytes : 0};
    const dim3 grid(32, 2, (unsigned)g->count);
    if (to_tiled) hipLaunchKernelGGL(k_tp_w2_layout<true>, grid, dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(k_tp_w2_layout<false>, grid, dim3(256), 0, (hipStream_t)stream, A);
    return hip_ok(hipGetLastError(), fn);
}
extern "C" int shems_group_w2_to_tiled(const shems_ddpg *d0, const shems_group *g, const shems_group_w2t *t, void *stream)
{
    return w2_layout("shems_group_w2_to_tiled", true, d0, g, t, stream);
}
extern "C" int shems_group_w2_to_flux(const shems_ddpg *d0, const shems_group *g, const shems_group_w2t *t, void *stream)
{
    return w2_layout("shems_group_w2_to_flux", false, d0, g, t, stream);
}

// The evaluation sweep's score / compare / snapshot for a whole group (k_group_eval_best above); every argument is checked before any
// device call.
extern "C" int shems_group_eval_best_dev(const shems_ddpg *d0, const shems_group *g, const shems_group_w2t *t, int32_t l1, int32_t l2,
                                         const double *d_returns, int32_t runs, int32_t episode, double *d_score, double *d_best_score,
                                         int32_t *d_best_run, uint8_t *d_improved, float *d_best0, int64_t best_stride_bytes, void *stream)
{
    const char *fn = "shems_group_eval_best_dev";
    if (!g || g->count < 1 || g->stride_bytes < 0 || (g->stride_bytes & 15) != 0 || (g->count > 1 && g->stride_bytes == 0))
        return set_error(SHEMS_ERR_ARG, "%s: shems_group needs count >= 1 and a 16-byte-multiple stride", fn);
    const int64_t e_eval = g->envs_per_learner;
    if (e_eval < 32 || e_eval % 32 != 0)
        return set_error(SHEMS_ERR_ARG, "%s: envs_per_learner (the eval block) must be a positive multiple of 32 (got %lld)", fn, (long long)e_eval);
    if (runs < 1 || runs > e_eval)
        return set_error(SHEMS_ERR_ARG, "%s: runs must be in 1..envs_per_learner = %lld (got %d)", fn, (long long)e_eval, runs);
    if (!d0 || !d0->actor || !d0->s_min || !d0->s_max) return set_error(SHEMS_ERR_ARG, "%s: shems_ddpg needs actor, s_min and s_max", fn);
    if (int rc = w2t_flux_guard(d0->actor, fn)) return rc;
    const bool wide = l1 != 0 || l2 != 0;
    int64_t n_actor = SHEMS_ACTOR_PARAMS;
    if (wide) {
        int64_t nc = 0;
        if (t) return set_error(SHEMS_ERR_ARG, "%s: the wide form (l1, l2) = (%d, %d) has no tiled layout: t must be NULL", fn, l1, l2);
        if (shems_wide_params(l1, l2, &n_actor, &nc) != SHEMS_OK)
            return set_error(SHEMS_ERR_ARG, "%s: hidden sizes (%d, %d) outside 1..4096", fn, l1, l2);
    }
    if (t && (!t->actor || ((uintptr_t)t->actor & 15) != 0))
        return set_error(SHEMS_ERR_ARG, "%s: shems_group_w2t.actor must be a 16-byte aligned device pointer", fn);
    if (((uintptr_t)d0->actor & 15) != 0) return set_error(SHEMS_ERR_ARG, "%s: the actor block must be 16-byte aligned", fn);
    if (!d_returns || !d_score || !d_best_score || !d_best_run || !d_improved || !d_best0)
        return set_error(SHEMS_ERR_ARG, "%s: returns, score, best_score, best_run, improved and the snapshot slab are required", fn);
    if ((((uintptr_t)d_returns | (uintptr_t)d_score | (uintptr_t)d_best_score) & 7) != 0 || ((uintptr_t)d_best_run & 3) != 0)
        return set_error(SHEMS_ERR_ARG, "%s: returns / score / best_score must be 8-byte and best_run 4-byte aligned", fn);
    const int64_t row = 4 * (((n_actor + 3) & ~(int64_t)3) + 32);     // actor | pad | s_min[9] | pad | s_max[9] | pad
    if (((uintptr_t)d_best0 & 15) != 0 || (best_stride_bytes & 15) != 0 || best_stride_bytes < row)
        return set_error(SHEMS_ERR_ARG, "%s: the snapshot slab must be 16-byte aligned with a 16-byte-multiple stride of at least %lld bytes "
                         "(got %lld)", fn, (long long)row, (long long)best_stride_bytes);
    EvalBestArgs A{d0->actor, d0->s_min, d0->s_max, t ? t->actor : nullptr, g->count > 1 ? g->stride_bytes : 0, n_actor, d_returns, e_eval, runs,
                   episode, d_score, d_best_score, d_best_run, d_improved, d_best0, best_stride_bytes};
    hipLaunchKernelGGL(k_group_eval_best, dim3((unsigned)g->count), dim3(256), 0, (hipStream_t)stream, A);
    return hip_ok(hipGetLastError(), "k_group_eval_best launch");
}

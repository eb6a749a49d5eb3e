// shems_wide.hip -- networks LARGER than the (250, 500) the tile maps of shems_policy.hip / shems_ddpg.hip are written for.
//
// The reference's hyper-parameter grids hold one such point: (L1, L2) = (300, 600) (input09_08_on_01-09_eval.jl:62-66 digit 3 = 0,
// input.jl:58-66).  Smaller networks run on the tuned kernels by zero padding (ddpg.pad_net); a larger one cannot, so it runs
// here, layer by layer, exactly as the reference's Flux / CUBLAS path does (Dense = W*x .+ b, Zygote's pullbacks: DDPG.jl:21-46,
// 99-145): every layer, forward or backward, is ONE general matrix product with a fused bias / relu / relu' epilogue.
//
// All on v_mfma_f32_32x32x2_f32 with fp32 accumulation in fixed orders (reproducible bit for bit; tolerance-class against the oracle like
// the tuned kernels, tests/test_wide_gpu.py); both operands by (row, column) element strides, so W (Flux layout [in][out]), its
// transpose, and the sample-major activations [m][features] go in without a copy.
//   k_wgemm       64 x 64 tile per workgroup of 4 waves, K in stages of 16 through double-buffered LDS: the vector step's layer 1.
//   k_wgemm128    128 x 128 tile, each wave a 64 x 64 quarter as 2 x 2 MFMA blocks: the vector step's layer 2 -- with the output layer
//                 folded into its epilogue, so relu(layer 2) never leaves the registers.
//   k_wgemm_sk    32 x 32 tile, K stage split over the four waves, up to four independent products per launch: everything in replay(),
//                 where one of M, N, K is the 128-row minibatch.
//   the rest      elementwise kernels: normalize, minibatch sample + gather (the same Philox sampler as the tuned path: the same
//                 (seed, tick) draws the same slots), tanh + concatenation, the two loss heads.
// ADAM + soft target update are shems_ddpg.hip's sweep (adam_soft_sweep: the same arithmetic on any parameter count).
//
// This path is about running the grid point, not about the roofline: sampler + 24 launches per replay() (0.22 ms at (300, 600)), a
// vector step of 65 536 envs 0.28 ms (87 TFLOP/s).  The headline configuration never comes here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>

#include "philox.h"
#include "shems_internal.h"
#include "shems_adam.h"

namespace shems {

typedef float wf32x16 __attribute__((ext_vector_type(16)));

constexpr int WBP = 128;                 // minibatch rows one update pass holds (as shems_ddpg.hip's BP)
constexpr int WSIN = 9, WAIN = 2, WCIN = 11;
constexpr int GT = 64, GK = 16, GKB = 4, GLD = GT + 4, GR = GT * GK / 256;   // tile, K per stage (2^GKB), LDS row stride, elements per thread and operand
static_assert((1 << GKB) == GK, "GK");

struct GemmArgs {
    const float *A, *B;
    float *C;
    int M, N, K;
    int64_t sai, sak, sbk, sbj, ldc;     // A(i, k) = A[i sai + k sak], B(k, j) = B[k sbk + j sbj], C[i ldc + j]
    const float *bias;                   // [N] or null
    const float *gate;                   // [M][ldg] or null: C = gate > 0 ? C : 0  (relu' read off the stored post-relu activations)
    int64_t ldg;
    int relu;
    // k_wgemm128<true> only: the output layer folded into this product's epilogue.  With C = relu(A B + bias) never stored,
    // head_out[(2 t + h) * M + i][o] = sum over the 64 columns j of half h of column tile t of C[i][j] * head_w[j * head_n + o]
    const float *head_w;
    float *head_out;
    int head_n;
};

// Learner groups (shems_wide_group_*): per operand, the float distance between learner l's copy and learner l - 1's.  A learner's
// networks, workspace and ring lie in its slab (one stride for all of them); the fused step's activations lie in a learner's env rows.
struct GStride { int64_t a, b, c, bias, gate, hw, ho; };
__device__ __forceinline__ GemmArgs gemm_at(GemmArgs G, const GStride &s, int64_t l)
{
    auto sh = [&](auto *p, int64_t d) { return p ? p + l * d : p; };
    G.A = sh(G.A, s.a); G.B = sh(G.B, s.b); G.C = sh(G.C, s.c); G.bias = sh(G.bias, s.bias); G.gate = sh(G.gate, s.gate);
    G.head_w = sh(G.head_w, s.hw); G.head_out = sh(G.head_out, s.ho);
    return G;
}

__global__ __launch_bounds__(256) void k_wgemm(GemmArgs G)
{
#include "wgemm_body.h"
}
// grid z = learner
__global__ __launch_bounds__(256) void k_wgemm_g(GemmArgs G0, GStride S)
{
    const GemmArgs G = gemm_at(G0, S, blockIdx.z);
#include "wgemm_body.h"
}

// The vector step's layer 2 (M = tens of thousands of envs, N = l2, K = l1: 98 % of its FLOPs): 128 x 128 tile, each wave a 64 x 64
// quarter as 2 x 2 MFMA blocks, so a k-step's four operand reads feed four MFMAs (the 64 x 64 kernel above: two reads per MFMA).
// HEAD: the output layer (l2 -> 2) is folded into the epilogue -- every wave reduces its 64 columns of relu(C) against W3 and leaves one
// partial per (row, output); relu(layer 2), 157 MB at 65 536 envs x 600, is never written or read back, and the N = 2 product, which
// a 64-wide tile pads 32-fold, disappears.  k_act_tail adds the partials in index order.
constexpr int BT = 128, BLD = BT + 4, BR = BT * GK / 256;
// V4: both operands are contiguous along the index that runs across a stage (A along k, B along j), 16-byte aligned, with row strides, K
// and N multiples of 4 (the host checks): a stage is staged with two 16-byte loads per operand and thread instead of eight predicated
// 4-byte ones -- a quarter of the load / address / bounds instructions next to the MFMAs.
typedef float wf32x4 __attribute__((ext_vector_type(4)));
template <bool HEAD, bool V4>
__global__ __launch_bounds__(256) void k_wgemm128(GemmArgs G)
{
#include "wgemm128_body.h"
}
// grid z = learner
template <bool HEAD, bool V4>
__global__ __launch_bounds__(256) void k_wgemm128_g(GemmArgs G0, GStride S)
{
    const GemmArgs G = gemm_at(G0, S, blockIdx.z);
#include "wgemm128_body.h"
}

// The minibatch-sized products (M <= a few hundred rows): few tiles and a long K.  One wave's chain of 32x32x2 MFMAs costs 32 cycles
// per k whatever the memory system does (K = 600: 9 us), and a 64 x 64 tile per workgroup leaves most CUs idle (N = 600: 20
// workgroups).  So here a workgroup owns a 32 x 32 tile and its four waves split every 64-deep K stage four ways (16 k each); the
// four partial tiles meet in LDS at the end and are added in wave order (a fixed order).  Same operands, strides and epilogue.
// Up to four INDEPENDENT products ride in one launch (grid z): the update is a chain of small dependent launches, and e.g. the layer-1
// products of three forward passes, or a layer's weight gradient, bias gradient and back-propagated error, need nothing from each other.
constexpr int SK = 64, SKB = 6, SLD = 32 + 4, SR = 32 * SK / 256, GMAX = 4;
struct GemmBatch { GemmArgs g[GMAX]; };
__global__ __launch_bounds__(256) void k_wgemm_sk(GemmBatch B)
{
    const GemmArgs &G = B.g[blockIdx.z];
#include "wgemm_sk_body.h"
}
// A learner group's products: grid z = learner * n + product, learner l's operands at the learner-0 pointers + l * its stride.  Each
// output element is summed in the same order as k_wgemm_sk's.
struct GemmBatchG { GemmArgs g[GMAX]; GStride s[GMAX]; int n; };
__global__ __launch_bounds__(256) void k_wgemm_sk_g(GemmBatchG B)
{
    const int q = (int)(blockIdx.z % (unsigned)B.n);
    const GemmArgs G = gemm_at(B.g[q], B.s[q], blockIdx.z / (unsigned)B.n);
#include "wgemm_sk_body.h"
}

static GemmArgs prod(const float *A, int64_t sai, int64_t sak, const float *B, int64_t sbk, int64_t sbj, float *C, int64_t ldc,
                     int64_t M, int N, int K, const float *bias = nullptr, int relu = 0, const float *gate = nullptr, int64_t ldg = 0)
{
    return GemmArgs{A, B, C, (int)M, N, K, sai, sak, sbk, sbj, ldc, bias, gate, ldg, relu};
}
// A learner group's replay(): `count` learners whose every buffer (networks, workspace, ring) is learner 0's + l * `stride` floats.
// null: one learner, the single-learner launches.
struct WGrp { int count; int64_t stride; };
// independent minibatch-sized products (one of M, N, K is the minibatch) in one launch; a group: the same products of every learner
static int gemm_multi(hipStream_t st, std::initializer_list<GemmArgs> list, const WGrp *grp = nullptr)
{
    GemmBatch b;
    std::memset(&b, 0, sizeof b);
    unsigned gx = 1, gy = 1, n = 0;
    for (const GemmArgs &g : list) {
        if (n >= GMAX) return set_error(SHEMS_ERR_ARG, "gemm_multi: at most %d products per launch", GMAX);
        b.g[n++] = g;
        gx = std::max(gx, (unsigned)((g.M + 31) / 32));
        gy = std::max(gy, (unsigned)((g.N + 31) / 32));
    }
    if (grp) {
        GemmBatchG bg;
        std::memset(&bg, 0, sizeof bg);
        const int64_t s = grp->stride;
        for (unsigned q = 0; q < n; ++q) { bg.g[q] = b.g[q]; bg.s[q] = GStride{s, s, s, s, s, 0, 0}; }
        bg.n = (int)n;
        hipLaunchKernelGGL(k_wgemm_sk_g, dim3(gx, gy, n * (unsigned)grp->count), dim3(256), 0, st, bg);
        return hip_ok(hipGetLastError(), "k_wgemm_sk_g launch");
    }
    hipLaunchKernelGGL(k_wgemm_sk, dim3(gx, gy, n), dim3(256), 0, st, b);
    return hip_ok(hipGetLastError(), "k_wgemm_sk launch");
}
static int gemm(hipStream_t st, const float *A, int64_t sai, int64_t sak, const float *B, int64_t sbk, int64_t sbj, float *C, int64_t ldc,
                int64_t M, int N, int K, const float *bias = nullptr, int relu = 0, const float *gate = nullptr, int64_t ldg = 0,
                const WGrp *grp = nullptr)
{
    GemmArgs g{A, B, C, (int)M, N, K, sai, sak, sbk, sbj, ldc, bias, gate, ldg, relu};
    if (M <= 512 || grp) return gemm_multi(st, {g}, grp);
    hipLaunchKernelGGL(k_wgemm, dim3((unsigned)((M + GT - 1) / GT), (unsigned)((N + GT - 1) / GT)), dim3(256), 0, st, g);
    return hip_ok(hipGetLastError(), "k_wgemm launch");
}

// A network (in -> l1 -> l2 -> out) in the flat Flux layout.
struct WNet {
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    int in, l1, l2, out;
};
static WNet wnet(const float *P, int in, int l1, int l2, int out)
{
    const float *W1 = P, *b1 = W1 + (int64_t)in * l1, *W2 = b1 + l1, *b2 = W2 + (int64_t)l1 * l2, *W3 = b2 + l2, *b3 = W3 + (int64_t)l2 * out;
    return WNet{W1, b1, W2, b2, W3, b3, in, l1, l2, out};
}
static int64_t wnet_size(int in, int l1, int l2, int out) { return (int64_t)in * l1 + l1 + (int64_t)l1 * l2 + l2 + (int64_t)l2 * out + out; }

// The three layer products of a forward pass over `rows` (the pass width: WBP, or a group's P) rows, as values: independent passes are
// launched layer by layer together.
struct Fwd { GemmArgs l1, l2, l3; };
static Fwd fwd_of(const WNet &n, const float *X, float *H1, float *H2, float *P, int rows = WBP)
{
    return Fwd{prod(X, n.in, 1, n.W1, n.l1, 1, H1, n.l1, rows, n.l1, n.in, n.b1, 1), prod(H1, n.l1, 1, n.W2, n.l2, 1, H2, n.l2, rows, n.l2, n.l1, n.b2, 1),
               prod(H2, n.l2, 1, n.W3, n.out, 1, P, n.out, rows, n.out, n.l2, n.b3, 0)};
}

// X [m][in] -> H1 [m][l1], H2 [m][l2] (post-relu), P [m][out] (pre-activation of the last layer, b3 included)
static int net_forward(hipStream_t st, const WNet &n, const float *X, int64_t m, float *H1, float *H2, float *P, const WGrp *grp = nullptr)
{
    if (int rc = gemm(st, X, n.in, 1, n.W1, n.l1, 1, H1, n.l1, m, n.l1, n.in, n.b1, 1, nullptr, 0, grp)) return rc;
    if (int rc = gemm(st, H1, n.l1, 1, n.W2, n.l2, 1, H2, n.l2, m, n.l2, n.l1, n.b2, 1, nullptr, 0, grp)) return rc;
    return gemm(st, H2, n.l2, 1, n.W3, n.out, 1, P, n.out, m, n.out, n.l2, n.b3, 0, nullptr, 0, grp);
}

// obs [m][9] -> (obs - s_min) / ((s_max - s_min) + 1f-8)  (normalize, MPS:55-57)
__global__ __launch_bounds__(256) void k_wnorm(const float *__restrict__ obs, const float *__restrict__ lo, const float *__restrict__ hi,
                                               float *__restrict__ out, int64_t count)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) {
        const int k = (int)(e % WSIN);
        out[e] = (obs[e] - lo[k]) / ((hi[k] - lo[k]) + 1e-8f);
    }
}

// ---- update workspace (floats; sample-major, WBP rows -- a group's pass width P rows) ----------------------------------------
struct WWs {
    float *XS, *XS2, *XC, *XC2, *XQ;          // [WBP][9] normalize(s), normalize(s'); [WBP][11] [s; a], [s'; actor_target(s')], [s; actor(s)]
    float *R, *DONE, *Y, *Q, *Q2, *DQ, *DQA;  // [WBP]
    int32_t *IDX;                             // [WBP] sampled ring slots
    float *PA, *PT, *API, *DA, *D3;           // [WBP][2] actor pre-activation, target actor's, a_pi; [WBP][11] d loss / d [s; a_pi]; [WBP][2]
    float *T1, *T2, *H1c, *H2c, *H1a, *H2a, *H1q, *H2q, *G1, *G2;
    float *ONES;                              // [WBP] ones: a bias gradient sum_m dY[m][n] is the product ones' dY, one more tile in a launch that runs anyway
    int64_t total;
};
// (host and device: a group's kernels carve learner l's workspace themselves)
__host__ __device__ static inline WWs wws(float *base, int l1, int l2, int P = WBP)
{
    WWs w;
    int64_t o = 0;
    auto take = [&](int64_t n) { float *p = base ? base + o : nullptr; o += (n + 3) / 4 * 4; return p; };
    w.XS = take(P * WSIN); w.XS2 = take(P * WSIN); w.XC = take(P * WCIN); w.XC2 = take(P * WCIN); w.XQ = take(P * WCIN);
    w.R = take(P); w.DONE = take(P); w.Y = take(P); w.Q = take(P); w.Q2 = take(P); w.DQ = take(P); w.DQA = take(P);
    w.IDX = reinterpret_cast<int32_t *>(take(P));
    w.PA = take(P * WAIN); w.PT = take(P * WAIN); w.API = take(P * WAIN); w.DA = take(P * WCIN); w.D3 = take(P * WAIN);
    w.T1 = take((int64_t)P * l1); w.T2 = take((int64_t)P * l2);
    w.H1c = take((int64_t)P * l1); w.H2c = take((int64_t)P * l2);
    w.H1a = take((int64_t)P * l1); w.H2a = take((int64_t)P * l2);
    w.H1q = take((int64_t)P * l1); w.H2q = take((int64_t)P * l2);
    w.G1 = take((int64_t)P * l1); w.G2 = take((int64_t)P * l2);
    w.ONES = take(P);
    w.total = o;
    return w;
}
// A group's pass width: P = max(128, max_batch rounded up to 32)
static int pass_width(int max_batch) { return std::max(WBP, (max_batch + 31) / 32 * 32); }
constexpr int WPMAX = 256;               // the widest pass a group runs (batch <= 256)

struct WPrep {
    shems_replay ring;
    int64_t ring_len, excl_pos, excl_count;
    uint64_t seed;
    uint32_t tick;
    int batch;
    const float *lo, *hi;
    WWs w;
};
// getData (MPS:31-42) + normalize: thread m = minibatch row m.  The sampler is shems_ddpg.hip's prep_load.
__device__ __forceinline__ void wprep_row(const WPrep &A, int m)
{
    const bool live = m < A.batch;
    const u32x4 x = philox4x32_10((uint32_t)(m >> 2), 0u, A.tick, kStreamSample, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
    const uint32_t wd = (m & 3) == 0 ? x.x : (m & 3) == 1 ? x.y : (m & 3) == 2 ? x.z : x.w;
    int64_t j = (int64_t)(wd % (uint32_t)(A.ring_len - A.excl_count));
    if (A.excl_count > 0) j = (A.excl_pos + A.excl_count + j) % A.ring.capacity;
    const WWs &w = A.w;
#pragma unroll
    for (int k = 0; k < WSIN; ++k) {
        const float lo = A.lo[k], den = (A.hi[k] - lo) + 1e-8f;
        const float x1 = live ? (A.ring.s[j * WSIN + k] - lo) / den : 0.0f;
        const float x2 = live ? (A.ring.s2[j * WSIN + k] - lo) / den : 0.0f;
        w.XS[m * WSIN + k] = x1; w.XS2[m * WSIN + k] = x2;
        w.XC[m * WCIN + k] = x1; w.XC2[m * WCIN + k] = x2; w.XQ[m * WCIN + k] = x1;
    }
    w.XC[m * WCIN + 9] = live ? A.ring.a[j * 2] : 0.0f;
    w.XC[m * WCIN + 10] = live ? A.ring.a[j * 2 + 1] : 0.0f;
    w.R[m] = live ? A.ring.r[j] : 0.0f;
    w.DONE[m] = live && A.ring.done[j] ? 1.0f : 0.0f;
    w.DQA[m] = live ? -1.0f / (float)A.batch : 0.0f;                 // d(-mean q) / dq
    w.IDX[m] = live ? (int32_t)j : -1;
    w.ONES[m] = 1.0f;
}
__global__ __launch_bounds__(WBP) void k_wprep(WPrep A) { wprep_row(A, threadIdx.x); }

// ---- a learner group (shems_wide_group_update): workgroup = learner, thread m = row m of the pass width P ----------------------------
struct WGroupArgs {
    shems_ddpg d0;                       // learner 0's blocks (learner l: + l * stride floats)
    shems_replay ring0;
    int64_t stride;                      // floats
    int64_t ring_len;
    uint64_t seed;
    uint32_t tick;
    int l1, l2, P, max_batch;
    const shems_group_hparams *hp;       // null: d0's batch / gamma
};
__device__ __forceinline__ int wg_batch(const WGroupArgs &A, int l) { return min(max(A.hp ? (int)A.hp[l].batch : A.d0.batch, 1), A.max_batch); }
__device__ __forceinline__ WWs wg_ws(const WGroupArgs &A, int l) { return wws(A.d0.ws + l * A.stride, A.l1, A.l2, A.P); }
__global__ __launch_bounds__(WPMAX) void k_wprep_g(WGroupArgs A)
{
    const int l = blockIdx.x;
    const int64_t off = (int64_t)l * A.stride * 4;
    shems_replay r = A.ring0;
    r.s = gsh(r.s, off); r.a = gsh(r.a, off); r.r = gsh(r.r, off); r.s2 = gsh(r.s2, off); r.done = gsh(r.done, off);
    const WPrep p{r, A.ring_len, 0, 0, A.seed + (uint64_t)l, A.tick, wg_batch(A, l), A.d0.s_min + l * A.stride, A.d0.s_max + l * A.stride, wg_ws(A, l)};
    wprep_row(p, threadIdx.x);
}
// shems_wide_group_update_x: learner l's ring length is min(pushed[l], xp[l].mem_size) in place of A.ring_len (a kernel of its own, so
// that k_wprep_g stays the code it was)
__global__ __launch_bounds__(WPMAX) void k_wprep_gx(WGroupArgs A, const shems_group_xparams *xp, const int64_t *pushed)
{
    const int l = blockIdx.x;
    const int64_t off = (int64_t)l * A.stride * 4;
    shems_replay r = A.ring0;
    r.s = gsh(r.s, off); r.a = gsh(r.a, off); r.r = gsh(r.r, off); r.s2 = gsh(r.s2, off); r.done = gsh(r.done, off);
    // clamped to 1..capacity: no division by zero, no slot outside the arrays
    const int64_t ring_len = min(max(min(pushed[l], (int64_t)xp[l].mem_size), (int64_t)1), r.capacity);
    const WPrep p{r, ring_len, 0, 0, A.seed + (uint64_t)l, A.tick, wg_batch(A, l), A.d0.s_min + l * A.stride, A.d0.s_max + l * A.stride, wg_ws(A, l)};
    wprep_row(p, threadIdx.x);
}
// a = tanh(P) for the live rows -> a_out [WBP][2] (may be null) and the action columns of a [WBP][11] critic input; workgroup 0: the
// target actor's head into [s'; a'], workgroup 1: the actor's into a_pi and [s; a_pi]
__device__ __forceinline__ void wtanh_cat_row(const float *__restrict__ P0, float *__restrict__ a0_out, float *__restrict__ cat0,
                                              const float *__restrict__ P1, float *__restrict__ a1_out, float *__restrict__ cat1, int batch, int m)
{
    const float *P = blockIdx.x == 0 ? P0 : P1;
    float *a_out = blockIdx.x == 0 ? a0_out : a1_out, *cat = blockIdx.x == 0 ? cat0 : cat1;
    const float a0 = m < batch ? tanhf(P[2 * m]) : 0.0f, a1 = m < batch ? tanhf(P[2 * m + 1]) : 0.0f;
    if (a_out) { a_out[2 * m] = a0; a_out[2 * m + 1] = a1; }
    cat[m * WCIN + 9] = a0;
    cat[m * WCIN + 10] = a1;
}
__global__ __launch_bounds__(WBP) void k_wtanh_cat(const float *__restrict__ P0, float *__restrict__ a0_out, float *__restrict__ cat0,
                                                   const float *__restrict__ P1, float *__restrict__ a1_out, float *__restrict__ cat1, int batch)
{
    wtanh_cat_row(P0, a0_out, cat0, P1, a1_out, cat1, batch, threadIdx.x);
}
// grid (2, learners)
__global__ __launch_bounds__(WPMAX) void k_wtanh_cat_g(WGroupArgs A)
{
    const int l = blockIdx.y;
    const WWs w = wg_ws(A, l);
    wtanh_cat_row(w.PT, nullptr, w.XC2, w.PA, w.API, w.XQ, wg_batch(A, l), threadIdx.x);
}

// critic loss head (DDPG.jl:131-135): y = r + gamma (1 - done) q', dq = 2 (q - y) / B, loss = mean((q - y)^2)
// rows: the pass width; red: [rows] of LDS
__device__ __forceinline__ void wloss_body(const WWs &w, float gamma, int batch, float *loss, int rows, float *red)
{
    const int m = threadIdx.x;
    const float y = w.R[m] + gamma * (1.0f - w.DONE[m]) * w.Q2[m];
    const float diff = m < batch ? w.Q[m] - y : 0.0f;
    w.Y[m] = y;
    w.DQ[m] = 2.0f * diff / (float)batch;
    red[m] = diff * diff;
    __syncthreads();
    if (m == 0) {
        float s = 0.0f;
        for (int i = 0; i < rows; ++i) s += red[i];
        loss[0] = s / (float)batch;
    }
}
__global__ __launch_bounds__(WBP) void k_wloss(WWs w, float gamma, int batch, float *loss)
{
    __shared__ float red[WBP];
    wloss_body(w, gamma, batch, loss, WBP, red);
}
__global__ __launch_bounds__(WPMAX) void k_wloss_g(WGroupArgs A)
{
    __shared__ float red[WPMAX];
    const int l = blockIdx.x;
    wloss_body(wg_ws(A, l), A.hp ? A.hp[l].gamma : A.d0.gamma, wg_batch(A, l), A.d0.losses + l * A.stride, A.P, red);
}

// actor loss head (DDPG.jl:137-140): loss = -mean(q); error at the actor's pre-tanh output = d loss / d a_pi * (1 - a_pi^2)
__device__ __forceinline__ void wactor_head_body(const WWs &w, int batch, float *loss, int rows, float *red)
{
    const int m = threadIdx.x;
    const bool live = m < batch;
#pragma unroll
    for (int o = 0; o < WAIN; ++o) {
        const float a = w.API[2 * m + o];
        w.D3[2 * m + o] = live ? w.DA[m * WCIN + 9 + o] * (1.0f - a * a) : 0.0f;
    }
    red[m] = live ? w.Q[m] : 0.0f;
    __syncthreads();
    if (m == 0) {
        float s = 0.0f;
        for (int i = 0; i < rows; ++i) s += red[i];
        loss[1] = -s / (float)batch;
    }
}
__global__ __launch_bounds__(WBP) void k_wactor_head(WWs w, int batch, float *loss)
{
    __shared__ float red[WBP];
    wactor_head_body(w, batch, loss, WBP, red);
}
__global__ __launch_bounds__(WPMAX) void k_wactor_head_g(WGroupArgs A)
{
    __shared__ float red[WPMAX];
    const int l = blockIdx.x;
    wactor_head_body(wg_ws(A, l), wg_batch(A, l), A.d0.losses + l * A.stride, A.P, red);
}

// Zygote's pullback of Chain(Dense, Dense, Dense) for the error d3 [WBP][out] at the last layer's pre-activation: parameter
// gradients into `grad` (flat Flux layout; null = input gradient only); dX [WBP][in] = d loss / d input if asked for.  X, H1, H2: what
// the forward pass kept.  Three launches: {gW3, gb3, G2}, {gW2, gb2, G1}, {gW1, gb1, dX} -- within one, nothing depends on anything.
// rows: the pass width (WBP; a group's P); grp: a learner group (every product of every learner in the same three launches).
static int net_backward(hipStream_t st, const WNet &n, const float *X, const float *H1, const float *H2, const float *d3, float *grad,
                        float *G1, float *G2, float *dX, const float *ones, int rows = WBP, const WGrp *grp = nullptr)
{
    const int R = rows;
    const GemmArgs g2 = prod(d3, n.out, 1, n.W3, 1, n.out, G2, n.l2, R, n.l2, n.out, nullptr, 0, H2, n.l2);       // (d3 W3') .* relu'
    const GemmArgs g1 = prod(G2, n.l2, 1, n.W2, 1, n.l2, G1, n.l1, R, n.l1, n.l2, nullptr, 0, H1, n.l1);          // (G2 W2') .* relu'
    if (!grad) {
        if (int rc = gemm_multi(st, {g2}, grp)) return rc;
        if (int rc = gemm_multi(st, {g1}, grp)) return rc;
        return dX ? gemm_multi(st, {prod(G1, n.l1, 1, n.W1, 1, n.l1, dX, n.in, R, n.in, n.l1)}, grp) : SHEMS_OK;      // G1 W1'
    }
    float *gW1 = grad, *gb1 = gW1 + (int64_t)n.in * n.l1, *gW2 = gb1 + n.l1, *gb2 = gW2 + (int64_t)n.l1 * n.l2, *gW3 = gb2 + n.l2,
          *gb3 = gW3 + (int64_t)n.l2 * n.out;
    auto colsum = [&](const float *D, int cols, float *out) { return prod(ones, R, 1, D, cols, 1, out, cols, 1, cols, R); };   // ones' D
    if (int rc = gemm_multi(st, {prod(H2, 1, n.l2, d3, n.out, 1, gW3, n.out, n.l2, n.out, R), colsum(d3, n.out, gb3), g2}, grp)) return rc;       // gW3 = H2' d3
    if (int rc = gemm_multi(st, {prod(H1, 1, n.l1, G2, n.l2, 1, gW2, n.l2, n.l1, n.l2, R), colsum(G2, n.l2, gb2), g1}, grp)) return rc;           // gW2 = H1' G2
    if (dX)
        return gemm_multi(st, {prod(X, 1, n.in, G1, n.l1, 1, gW1, n.l1, n.in, n.l1, R), colsum(G1, n.l1, gb1),                             // gW1 = X' G1
                               prod(G1, n.l1, 1, n.W1, 1, n.l1, dX, n.in, R, n.in, n.l1)}, grp);
    return gemm_multi(st, {prod(X, 1, n.in, G1, n.l1, 1, gW1, n.l1, n.in, n.l1, R), colsum(G1, n.l1, gb1)}, grp);
}

static int check_shape(int l1, int l2, const char *fn)
{
    if (l1 < 1 || l2 < 1 || l1 > 4096 || l2 > 4096) return set_error(SHEMS_ERR_ARG, "%s: hidden sizes must be in 1..4096 (got %d, %d)", fn, l1, l2);
    return SHEMS_OK;
}
static int check_wide(const shems_ddpg *d, int l1, int l2, const char *fn)
{
    if (int rc = check_shape(l1, l2, fn)) return rc;
    if (!d || !d->actor || !d->critic || !d->actor_t || !d->critic_t || !d->m_actor || !d->v_actor || !d->m_critic ||
        !d->v_critic || !d->grad_actor || !d->grad_critic || !d->s_min || !d->s_max || !d->ws || !d->losses)
        return set_error(SHEMS_ERR_ARG, "%s: shems_ddpg has a NULL buffer", fn);
    if (d->batch < 1 || d->batch > WBP) return set_error(SHEMS_ERR_ARG, "%s: batch must be in 1..128 (got %d)", fn, d->batch);
    for (const float *p : {d->actor, d->critic, d->actor_t, d->critic_t, d->m_actor, d->v_actor, d->m_critic, d->v_critic})
        if (int rc = w2t_flux_guard(p, fn)) return rc;
    return SHEMS_OK;
}

// used by shems_policy.hip's wide act entry points: the vector step's forward pass.  Outputs `n_partials` partial pre-activation sums
// [p][m][2] into d_part (b3 NOT included: k_act_tail adds b3 and the partials in index order).
int wide_actor_pre(const float *actor, const float *s_min, const float *s_max, int l1, int l2, const float *d_obs, int64_t m, float *d_ws,
                   float *d_part, int *n_partials, hipStream_t st)
{
    if (int rc = check_shape(l1, l2, "shems_wide_act")) return rc;
    float *xn = d_ws, *H1 = xn + (m * WSIN + 3) / 4 * 4;
    const int64_t cnt = m * WSIN;
    const WNet n = wnet(actor, WSIN, l1, l2, WAIN);
    hipLaunchKernelGGL(k_wnorm, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, d_obs, s_min, s_max, xn, cnt);
    if (int rc = gemm(st, xn, n.in, 1, n.W1, n.l1, 1, H1, n.l1, m, n.l1, n.in, n.b1, 1)) return rc;
    // layer 2 with the output layer in its epilogue: relu(layer 2) stays in registers
    GemmArgs g = prod(H1, n.l1, 1, n.W2, n.l2, 1, nullptr, 0, m, n.l2, n.l1, n.b2, 1);
    g.head_w = n.W3; g.head_out = d_part; g.head_n = WAIN;
    const unsigned ty = (unsigned)((l2 + BT - 1) / BT);
    *n_partials = 2 * (int)ty;
    const bool v4 = (l1 % 4) == 0 && (l2 % 4) == 0 && ((uintptr_t)H1 & 15) == 0 && ((uintptr_t)n.W2 & 15) == 0;     // (300, 600): yes
    if (v4) hipLaunchKernelGGL((k_wgemm128<true, true>), dim3((unsigned)((m + BT - 1) / BT), ty), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((k_wgemm128<true, false>), dim3((unsigned)((m + BT - 1) / BT), ty), dim3(256), 0, st, g);
    return hip_ok(hipGetLastError(), "k_wgemm128 launch");
}
// A learner group's fused step (shems_wide_act_step_group_dev): env i = l * epl + r is learner l's; its actor and normalisation are
// learner 0's + l * stride floats.  Three launches for every learner: normalise, layer 1 (grid z = learner), layer 2 with the head
// (grid z = learner).  d_part holds learner l's partials at [l][p][epl][2].
__global__ __launch_bounds__(256) void k_wnorm_g(const float *__restrict__ obs, const float *__restrict__ lo0, const float *__restrict__ hi0,
                                                 float *__restrict__ out, int64_t count, int64_t per_learner, int64_t stride)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) {
        const int k = (int)(e % WSIN);
        const int64_t off = (e / per_learner) * stride;
        const float lo = lo0[off + k], hi = hi0[off + k];
        out[e] = (obs[e] - lo) / ((hi - lo) + 1e-8f);
    }
}
int wide_actor_pre_group(const float *actor0, const float *s_min0, const float *s_max0, int64_t stride, int count, int64_t epl, int l1, int l2,
                         const float *d_obs, float *d_ws, float *d_part, int *n_partials, hipStream_t st)
{
    if (int rc = check_shape(l1, l2, "shems_wide_act_step_group_dev")) return rc;
    const int64_t m = epl * count, cnt = m * WSIN;
    float *xn = d_ws, *H1 = xn + (m * WSIN + 3) / 4 * 4;
    const WNet n = wnet(actor0, WSIN, l1, l2, WAIN);
    hipLaunchKernelGGL(k_wnorm_g, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, d_obs, s_min0, s_max0, xn, cnt, epl * WSIN, stride);
    const GemmArgs g1 = prod(xn, n.in, 1, n.W1, n.l1, 1, H1, n.l1, epl, n.l1, n.in, n.b1, 1);
    hipLaunchKernelGGL(k_wgemm_g, dim3((unsigned)((epl + GT - 1) / GT), (unsigned)((l1 + GT - 1) / GT), (unsigned)count), dim3(256), 0, st, g1,
                       GStride{epl * WSIN, stride, epl * l1, stride, 0, 0, 0});
    if (int rc = hip_ok(hipGetLastError(), "k_wgemm_g launch")) return rc;
    GemmArgs g = prod(H1, n.l1, 1, n.W2, n.l2, 1, nullptr, 0, epl, n.l2, n.l1, n.b2, 1);
    g.head_w = n.W3; g.head_out = d_part; g.head_n = WAIN;
    const unsigned ty = (unsigned)((l2 + BT - 1) / BT);
    *n_partials = 2 * (int)ty;
    const GStride s2{epl * l1, stride, 0, stride, 0, stride, 2 * (int64_t)ty * epl * WAIN};
    const dim3 grid((unsigned)((epl + BT - 1) / BT), ty, (unsigned)count);
    // learner l's H1 / W2 keep learner 0's 16-byte alignment: epl is a multiple of 32, the stride of 16 bytes
    const bool v4 = (l1 % 4) == 0 && (l2 % 4) == 0 && ((uintptr_t)H1 & 15) == 0 && ((uintptr_t)n.W2 & 15) == 0 && (stride % 4) == 0;
    if (v4) hipLaunchKernelGGL((k_wgemm128_g<true, true>), grid, dim3(256), 0, st, g, s2);
    else hipLaunchKernelGGL((k_wgemm128_g<true, false>), grid, dim3(256), 0, st, g, s2);
    return hip_ok(hipGetLastError(), "k_wgemm128_g launch");
}
// floats of d_ws: normalised observations, layer 1, and the partial sums of the output layer
int64_t wide_act_part_offset(int l1, int64_t m) { return (m * WSIN + 3) / 4 * 4 + (m * (int64_t)l1 + 3) / 4 * 4; }      // 16-byte aligned
int64_t wide_act_ws_floats(int l1, int l2, int64_t m) { return wide_act_part_offset(l1, m) + 2 * ((l2 + BT - 1) / BT) * m * WAIN; }

}  // namespace shems

using namespace shems;

extern "C" {

int shems_wide_params(int32_t l1, int32_t l2, int64_t *n_actor, int64_t *n_critic)
{
    if (int rc = check_shape(l1, l2, "shems_wide_params")) return rc;
    if (n_actor) *n_actor = wnet_size(WSIN, l1, l2, WAIN);
    if (n_critic) *n_critic = wnet_size(WCIN, l1, l2, 1);
    return SHEMS_OK;
}

int shems_wide_workspace_floats(int32_t l1, int32_t l2, int64_t *out)
{
    if (int rc = check_shape(l1, l2, "shems_wide_workspace_floats")) return rc;
    if (!out) return set_error(SHEMS_ERR_ARG, "shems_wide_workspace_floats: NULL");
    *out = wws(nullptr, l1, l2).total;
    return SHEMS_OK;
}

int shems_wide_act_workspace_floats(int32_t l1, int32_t l2, int64_t m, int64_t *out)
{
    if (int rc = check_shape(l1, l2, "shems_wide_act_workspace_floats")) return rc;
    if (!out || m <= 0) return set_error(SHEMS_ERR_ARG, "shems_wide_act_workspace_floats: bad arguments");
    *out = wide_act_ws_floats(l1, l2, m);
    return SHEMS_OK;
}

int shems_wide_group_workspace_floats(int32_t l1, int32_t l2, int32_t max_batch, int64_t *out)
{
    if (int rc = check_shape(l1, l2, "shems_wide_group_workspace_floats")) return rc;
    if (!out) return set_error(SHEMS_ERR_ARG, "shems_wide_group_workspace_floats: NULL");
    if (max_batch < 1 || max_batch > WPMAX)
        return set_error(SHEMS_ERR_ARG, "shems_wide_group_workspace_floats: max_batch must be in 1..%d (got %d)", WPMAX, max_batch);
    *out = wws(nullptr, l1, l2, pass_width(max_batch)).total;
    return SHEMS_OK;
}

int shems_wide_critic_grad_ex(const shems_ddpg *d, int32_t l1, int32_t l2, const shems_replay *ring, int64_t ring_len, uint64_t seed,
                              uint32_t tick, int64_t excl_pos, int64_t excl_count, void *stream)
{
    if (int rc = check_wide(d, l1, l2, "shems_wide_critic_grad_ex")) return rc;
    if (!ring || !ring->s || !ring->a || !ring->r || !ring->s2 || !ring->done || ring_len < 1 || ring_len > ring->capacity)
        return set_error(SHEMS_ERR_ARG, "shems_wide_critic_grad_ex: bad replay ring / length");
    if (excl_count < 0 || excl_pos < 0 || (excl_count > 0 && (ring_len != ring->capacity || excl_count >= ring_len)))
        return set_error(SHEMS_ERR_ARG, "shems_wide_critic_grad_ex: an exclusion window needs a full ring and 0 <= count < capacity");
    hipStream_t st = (hipStream_t)stream;
    const WWs w = wws(d->ws, l1, l2);
    WPrep p{*ring, ring_len, excl_pos, excl_count, seed, tick, d->batch, d->s_min, d->s_max, w};
    hipLaunchKernelGGL(k_wprep, dim3(1), dim3(WBP), 0, st, p);
    // Three forward passes need only the minibatch: a' = actor_target(s') (DDPG.jl:131), q = critic([s; a]) (:134) and a_pi = actor(s)
    // (:138; the actor does not change before shems_wide_actor_apply_pub) -- launched together, layer by layer.
    const WNet c = wnet(d->critic, WCIN, l1, l2, 1);
    const Fwd ft = fwd_of(wnet(d->actor_t, WSIN, l1, l2, WAIN), w.XS2, w.T1, w.T2, w.PT), fc = fwd_of(c, w.XC, w.H1c, w.H2c, w.Q),
              fa = fwd_of(wnet(d->actor, WSIN, l1, l2, WAIN), w.XS, w.H1a, w.H2a, w.PA);
    if (int rc = gemm_multi(st, {ft.l1, fc.l1, fa.l1})) return rc;
    if (int rc = gemm_multi(st, {ft.l2, fc.l2, fa.l2})) return rc;
    if (int rc = gemm_multi(st, {ft.l3, fc.l3, fa.l3})) return rc;
    hipLaunchKernelGGL(k_wtanh_cat, dim3(2), dim3(WBP), 0, st, w.PT, (float *)nullptr, w.XC2, w.PA, w.API, w.XQ, d->batch);
    // q' = critic_target([s'; a'])  (DDPG.jl:132); T1 / T2 are free again
    if (int rc = net_forward(st, wnet(d->critic_t, WCIN, l1, l2, 1), w.XC2, WBP, w.T1, w.T2, w.Q2)) return rc;
    // loss_crit = mse(q, y) and its pullback (DDPG.jl:133-135)
    hipLaunchKernelGGL(k_wloss, dim3(1), dim3(WBP), 0, st, w, d->gamma, d->batch, d->losses);
    return net_backward(st, c, w.XC, w.H1c, w.H2c, w.DQ, d->grad_critic, w.G1, w.G2, nullptr, w.ONES);
}

int shems_wide_actor_grad(const shems_ddpg *d, int32_t l1, int32_t l2, void *stream)
{
    if (int rc = check_wide(d, l1, l2, "shems_wide_actor_grad")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const WWs w = wws(d->ws, l1, l2);
    // loss_act = -mean(critic([s; actor(s)])) through the critic as it stands now (already updated, DDPG.jl:137-140); a_pi = actor(s) and
    // the actor's hidden layers were laid down by shems_wide_critic_grad_ex
    const WNet a = wnet(d->actor, WSIN, l1, l2, WAIN), c = wnet(d->critic, WCIN, l1, l2, 1);
    if (int rc = net_forward(st, c, w.XQ, WBP, w.H1q, w.H2q, w.Q)) return rc;
    if (int rc = net_backward(st, c, w.XQ, w.H1q, w.H2q, w.DQA, nullptr, w.G1, w.G2, w.DA, w.ONES)) return rc;
    hipLaunchKernelGGL(k_wactor_head, dim3(1), dim3(WBP), 0, st, w, d->batch, d->losses);
    return net_backward(st, a, w.XS, w.H1a, w.H2a, w.D3, d->grad_actor, w.G1, w.G2, nullptr, w.ONES);
}

int shems_wide_critic_apply(const shems_ddpg *d, int32_t l1, int32_t l2, double eta, double bp1, double bp2, double grad_scale, void *stream)
{
    if (int rc = check_wide(d, l1, l2, "shems_wide_critic_apply")) return rc;
    return adam_soft_sweep(d->critic, d->grad_critic, d->m_critic, d->v_critic, d->critic_t, nullptr, (int)wnet_size(WCIN, l1, l2, 1), eta, bp1,
                           bp2, grad_scale, d->tau, (hipStream_t)stream);
}

int shems_wide_actor_apply_pub(const shems_ddpg *d, int32_t l1, int32_t l2, double eta, double bp1, double bp2, double grad_scale,
                               float *d_publish, void *stream)
{
    if (int rc = check_wide(d, l1, l2, "shems_wide_actor_apply_pub")) return rc;
    return adam_soft_sweep(d->actor, d->grad_actor, d->m_actor, d->v_actor, d->actor_t, d_publish, (int)wnet_size(WSIN, l1, l2, WAIN), eta, bp1,
                           bp2, grad_scale, d->tau, (hipStream_t)stream);
}

/* replay() for every learner of a group on the wide path: the launches of shems_wide_critic_grad_ex, _critic_apply, _actor_grad and
   _actor_apply_pub, each once for all learners (grid z / x = learner). */
// shems_wide_group_update (d_xp == null) and shems_wide_group_update_x (per-learner ring lengths on the device; ring_len is not used)
static int wide_group_update(const char *fn, const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, int32_t l1, int32_t l2,
                             const shems_group_hparams *d_hp, const shems_group_xparams *d_xp, const int64_t *d_pushed, int32_t max_batch,
                             int64_t ring_len, uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit, double eta_act,
                             double bp1_act, double bp2_act, void *stream)
{
    if (int rc = check_shape(l1, l2, fn)) return rc;
    if (!d0 || !d0->actor || !d0->critic || !d0->actor_t || !d0->critic_t || !d0->m_actor || !d0->v_actor || !d0->m_critic ||
        !d0->v_critic || !d0->grad_actor || !d0->grad_critic || !d0->s_min || !d0->s_max || !d0->ws || !d0->losses)
        return set_error(SHEMS_ERR_ARG, "%s: shems_ddpg has a NULL buffer", fn);
    if (!g || g->count < 1 || g->count > 65535 / GMAX || g->stride_bytes < 0 || (g->stride_bytes & 15) != 0 || (g->count > 1 && g->stride_bytes == 0))
        return set_error(SHEMS_ERR_ARG, "%s: shems_group needs 1 <= count <= %d and a 16-byte-multiple stride", fn, 65535 / GMAX);
    if (max_batch < 1 || max_batch > WPMAX) return set_error(SHEMS_ERR_ARG, "%s: max_batch must be in 1..%d (got %d)", fn, WPMAX, max_batch);
    if (d_hp && ((uintptr_t)d_hp & 7) != 0) return set_error(SHEMS_ERR_ARG, "%s: d_hp must be an 8-byte aligned device array of count records", fn);
    if (!d_hp && (d0->batch < 1 || d0->batch > max_batch))
        return set_error(SHEMS_ERR_ARG, "%s: batch must be in 1..max_batch = %d (got %d)", fn, max_batch, d0->batch);
    if (!ring0 || !ring0->s || !ring0->a || !ring0->r || !ring0->s2 || !ring0->done || ring_len < 1 || ring_len > ring0->capacity)
        return set_error(SHEMS_ERR_ARG, "%s: bad replay ring / length", fn);
    for (const void *q : {(const void *)d0->actor, (const void *)d0->critic, (const void *)d0->actor_t, (const void *)d0->critic_t,
                          (const void *)d0->m_actor, (const void *)d0->v_actor, (const void *)d0->m_critic, (const void *)d0->v_critic,
                          (const void *)d0->grad_actor, (const void *)d0->grad_critic})
        if (((uintptr_t)q & 15) != 0) return set_error(SHEMS_ERR_ARG, "%s: parameter, moment and gradient blocks must be 16-byte aligned", fn);
    if (int rc = w2t_flux_guard(d0->actor, fn)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int L = g->count, P = pass_width(max_batch);
    const int64_t stride = g->count > 1 ? g->stride_bytes / 4 : 0;
    const WGrp grp{L, stride};
    const WGroupArgs A{*d0, *ring0, stride, ring_len, seed, tick, l1, l2, P, max_batch, d_hp};
    const WWs w = wws(d0->ws, l1, l2, P);                     // learner 0's carve; learner l's is the same + l * stride
    // critic gradient (shems_wide_critic_grad_ex)
    if (d_xp) hipLaunchKernelGGL(k_wprep_gx, dim3((unsigned)L), dim3((unsigned)P), 0, st, A, d_xp, d_pushed);
    else hipLaunchKernelGGL(k_wprep_g, dim3((unsigned)L), dim3((unsigned)P), 0, st, A);
    const WNet c = wnet(d0->critic, WCIN, l1, l2, 1), a = wnet(d0->actor, WSIN, l1, l2, WAIN);
    const Fwd ft = fwd_of(wnet(d0->actor_t, WSIN, l1, l2, WAIN), w.XS2, w.T1, w.T2, w.PT, P), fc = fwd_of(c, w.XC, w.H1c, w.H2c, w.Q, P),
              fa = fwd_of(a, w.XS, w.H1a, w.H2a, w.PA, P);
    if (int rc = gemm_multi(st, {ft.l1, fc.l1, fa.l1}, &grp)) return rc;
    if (int rc = gemm_multi(st, {ft.l2, fc.l2, fa.l2}, &grp)) return rc;
    if (int rc = gemm_multi(st, {ft.l3, fc.l3, fa.l3}, &grp)) return rc;
    hipLaunchKernelGGL(k_wtanh_cat_g, dim3(2, (unsigned)L), dim3((unsigned)P), 0, st, A);
    if (int rc = net_forward(st, wnet(d0->critic_t, WCIN, l1, l2, 1), w.XC2, P, w.T1, w.T2, w.Q2, &grp)) return rc;
    hipLaunchKernelGGL(k_wloss_g, dim3((unsigned)L), dim3((unsigned)P), 0, st, A);
    if (int rc = net_backward(st, c, w.XC, w.H1c, w.H2c, w.DQ, d0->grad_critic, w.G1, w.G2, nullptr, w.ONES, P, &grp)) return rc;
    // ADAM + soft update of every critic (shems_wide_critic_apply)
    if (int rc = adam_soft_sweep_group(d0->critic, d0->grad_critic, d0->m_critic, d0->v_critic, d0->critic_t, (int)wnet_size(WCIN, l1, l2, 1), eta_crit,
                                       bp1_crit, bp2_crit, d0->tau, L, stride * 4, d_hp, true, st)) return rc;
    // actor gradient through the updated critic (shems_wide_actor_grad)
    if (int rc = net_forward(st, c, w.XQ, P, w.H1q, w.H2q, w.Q, &grp)) return rc;
    if (int rc = net_backward(st, c, w.XQ, w.H1q, w.H2q, w.DQA, nullptr, w.G1, w.G2, w.DA, w.ONES, P, &grp)) return rc;
    hipLaunchKernelGGL(k_wactor_head_g, dim3((unsigned)L), dim3((unsigned)P), 0, st, A);
    if (int rc = net_backward(st, a, w.XS, w.H1a, w.H2a, w.D3, d0->grad_actor, w.G1, w.G2, nullptr, w.ONES, P, &grp)) return rc;
    return adam_soft_sweep_group(d0->actor, d0->grad_actor, d0->m_actor, d0->v_actor, d0->actor_t, (int)wnet_size(WSIN, l1, l2, WAIN), eta_act,
                                 bp1_act, bp2_act, d0->tau, L, stride * 4, d_hp, false, st);
}

int shems_wide_group_update(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, int32_t l1, int32_t l2,
                            const shems_group_hparams *d_hp, int32_t max_batch, int64_t ring_len, uint64_t seed, uint32_t tick,
                            double eta_crit, double bp1_crit, double bp2_crit, double eta_act, double bp1_act, double bp2_act, void *stream)
{
    return wide_group_update("shems_wide_group_update", d0, ring0, g, l1, l2, d_hp, nullptr, nullptr, max_batch, ring_len, seed, tick, eta_crit,
                             bp1_crit, bp2_crit, eta_act, bp1_act, bp2_act, stream);
}

int shems_wide_group_update_x(const shems_ddpg *d0, const shems_replay *ring0, const shems_group *g, int32_t l1, int32_t l2,
                              const shems_group_hparams *d_hp, const shems_group_xparams *d_xp, const int64_t *d_pushed, int32_t max_batch,
                              uint64_t seed, uint32_t tick, double eta_crit, double bp1_crit, double bp2_crit, double eta_act,
                              double bp1_act, double bp2_act, void *stream)
{
    const char *fn = "shems_wide_group_update_x";
    if (!d_hp || !d_xp || !d_pushed) return set_error(SHEMS_ERR_ARG, "%s: d_hp, d_xp and d_pushed are all required", fn);
    if ((((uintptr_t)d_xp | (uintptr_t)d_pushed) & 7) != 0)
        return set_error(SHEMS_ERR_ARG, "%s: d_xp and d_pushed must be 8-byte aligned device arrays of count records", fn);
    return wide_group_update(fn, d0, ring0, g, l1, l2, d_hp, d_xp, d_pushed, max_batch, 1, seed, tick, eta_crit, bp1_crit, bp2_crit, eta_act,
                             bp1_act, bp2_act, stream);
}

/* the s rows of the minibatch the last shems_wide_critic_grad_ex sampled (adapt_param_noise!, DDPG.jl:74-87) */
int shems_wide_batch_slots(const shems_ddpg *d, int32_t l1, int32_t l2, int32_t *out_slots, void *stream)
{
    if (int rc = check_wide(d, l1, l2, "shems_wide_batch_slots")) return rc;
    if (!out_slots) return set_error(SHEMS_ERR_ARG, "shems_wide_batch_slots: NULL");
    const WWs w = wws(d->ws, l1, l2);
    if (int rc = hip_ok(hipMemcpyAsync(out_slots, w.IDX, sizeof(int32_t) * d->batch, hipMemcpyDeviceToHost, (hipStream_t)stream), "memcpy slots")) return rc;
    return hip_ok(hipStreamSynchronize((hipStream_t)stream), "sync");
}

}  // extern "C"

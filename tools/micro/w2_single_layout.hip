// The single learner's three access shapes on the 250 x 500 layer-2 state, WITHOUT their matrix work, in Flux order and in the
// tiled layout of shems_group_w2t ([4 k-tiles][8 n-tiles][m | v | p | target][64][64] floats, zero padded to 256 x 512).  Sibling of
// adam_stream.hip (which has the learner groups' 64 x 64 shape); the question here is whether the line-aligned layout is worth
// carrying to the five-launch replay() and to k_act2 at ONE learner, where the passes are short and partly latency.
//
//   grad   k_grad's W workgroups (csrc/shems_ddpg.hip, grad_body): 207 workgroups of which 128 own a 32 x 32 tile; wave w the 16 x 16
//          block (k half w >> 1, n half w & 1), lane (g, c) the elements (4 g + r, c), r < 4: scalar loads of m, v, p, target up front,
//          adam_math, scalar stores.  `grad+wait`: the same with ~2.5 us of spinning between the loads and the arithmetic (the real
//          kernel requests its ADAM state with its first burst and consumes it after the tile: the load latency is hidden there).
//   fwd    k_fwd's W2 panel: 64 workgroups (16 n-tiles x 4 column tiles), each W2[0..255][32 nt .. +32) as 8 float4 per thread.
//   act    k_act2's W2 stream: 1 024 workgroups of four waves, two per CU (80 KB of LDS each), wave w moves columns [128 w, +128) of
//          all 250 rows through LDS-DMA, 16 chunks of 16 rows, a piece = rows 2 q, 2 q + 1 (512 B each in Flux order, 2 x 256 B per
//          row on tiles), a two-chunk ring per wave.  No MFMAs: this is the stream's own ceiling, not the kernel's time.
//   replay fwd, fwd, grad, fwd, grad as dependent launches on one stream (the order of replay()'s K1..K5).
//
// Every shape runs (a) hot: 20 dependent launches back to back, time / 20, seven rounds; (b) behind the act stream: one act launch
// (512 MB through L2), then the measured launch between two events, eleven times -- how a replay() finds its state in the train loop.
// Flux order is run at the actor's and at the critic's W2 offset (byte 10 000 / 12 000 of the parameter vector).
//
// Build + run (from the repo root):
//   hipcc -O3 --offload-arch=gfx950 -I <package>/csrc -o abl/w2_single_layout tools/micro/w2_single_layout.hip && abl/w2_single_layout
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "shems_adam.h"

using namespace shems;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int K = 250, N = 500;
constexpr int64_t VEC = 129004;                 // floats of a parameter vector (critic: 11 x 250 + 250 + 125 000 + 500 + 500 + 1, padded to 4)
constexpr int64_t TILE = 64 * 64, TBLK = 4 * TILE, TILED_FLOATS = 32 * TBLK;      // 2 MB per network

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

struct Lay {
    float *m, *v, *p, *t;  // Flux order: the four parameter-vector-shaped arrays; tiled: all four = the region's base
    int woff;              // Flux order: off_w2 in floats
    float *out;            // [1 024 x 256] sink
    AdamCtx c;
};

// element (k, n), k < 256, n < 512, of array a (0 m, 1 v, 2 p, 3 target) in the tiled region
__device__ __forceinline__ int64_t tl(int a, int k, int n) { return ((int64_t)((k >> 6) * 8 + (n >> 6)) * 4 + a) * TILE + (k & 63) * 64 + (n & 63); }

template <bool TILED, int SPIN>
__global__ __launch_bounds__(256) void k_grad_shape(Lay A)
{
    const int bx = blockIdx.x;
    if (bx >= 8 * 16) return;                                   // (the G and R workgroups touch no layer-2 state)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kt = bx / 16, nt = bx % 16;
    int64_t im[4], iv[4], ip[4], it[4];
    bool ok[4];
    float m[4], v[4], p[4], t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = kt * 32 + 16 * (wave >> 1) + 4 * (lane >> 4) + r, n = nt * 32 + 16 * (wave & 1) + (lane & 15);
        ok[r] = k < K && n < N;
        if (TILED) { im[r] = tl(0, k, n); iv[r] = tl(1, k, n); ip[r] = tl(2, k, n); it[r] = tl(3, k, n); }
        else { const int64_t e = ok[r] ? A.woff + (int64_t)k * N + n : 0; im[r] = iv[r] = ip[r] = it[r] = e; }
        m[r] = A.m[im[r]]; v[r] = A.v[iv[r]]; p[r] = A.p[ip[r]]; t[r] = A.t[it[r]];
    }
    if (SPIN) {
        const uint64_t t0 = wall_clock64();                     // 100 MHz
        while (wall_clock64() - t0 < SPIN) __builtin_amdgcn_s_sleep(8);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 4; ++r) adam_math(A.c, 1e-3f * (float)((tid + r) & 31) - 0.015f, m[r], v[r], p[r], t[r]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (ok[r]) { A.m[im[r]] = m[r]; A.v[iv[r]] = v[r]; A.p[ip[r]] = p[r]; A.t[it[r]] = t[r]; }
}

template <bool TILED>
__global__ __launch_bounds__(256) void k_fwd_shape(Lay A)
{
    const int tid = threadIdx.x, n0 = 32 * (blockIdx.x >> 2);
    f32x4 wv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int e = i * 256 + tid, k = e >> 3, c = e & 7;
        const int64_t a = TILED ? tl(2, k, n0 + 4 * c) : A.woff + (int64_t)min(k, K - 1) * N + n0 + 4 * c;     // (Flux order: the last tile's columns >= 500
        wv[i] = *reinterpret_cast<const f32x4 *>(A.p + a);                                                     //  read the next row / b2, in bounds)
    }
    f32x4 s = wv[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += wv[i];
    A.out[(int64_t)blockIdx.x * 256 + tid] = (s[0] + s[1]) + (s[2] + s[3]);
}

__device__ __forceinline__ void glds16(const char *sbase, uint32_t voff, uint32_t lds_base)
{
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(sbase), "s"(lds_base) : "memory");
}

template <bool TILED>
__global__ __launch_bounds__(256) void k_act_shape(Lay A)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];            // [4 waves][2 chunks][8 pieces][256 floats] = 64 KB (80 KB requested: two per CU)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *Wf = smem + wave * (2 * 2048);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)Wf;
    const char *base = TILED ? reinterpret_cast<const char *>(A.p) + 2 * TILE * 4 + (size_t)wave * (2 * TBLK * 4)
                             : reinterpret_cast<const char *>(A.p + A.woff) + wave * 512;
    // lane part of piece q of a chunk: Flux order row 2 q + (lane >> 5), 16 B x (lane & 31); tiled: tile 2 w + ((lane & 31) >> 4), row likewise
    const uint32_t vlane = TILED ? (uint32_t)(((lane & 31) >> 4) * (TBLK * 4) + (lane >> 5) * 256 + (lane & 15) * 16)
                                 : (uint32_t)((lane >> 5) * (N * 4) + (lane & 31) * 16);
    float acc = 0.0f;
#pragma unroll 1
    for (int c = 0; c < 16; ++c) {
        const char *cb = base + (TILED ? (size_t)(c >> 2) * (8 * TBLK * 4) + (size_t)(c & 3) * (16 * 256) : (size_t)c * (16 * N * 4));
        const int np = c == 15 ? 5 : 8;                                     // rows >= 250 are never fetched
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < np) glds16(cb, vlane + q * (TILED ? 512 : 2 * N * 4), lds0 + (c & 1) * 8192 + q * 1024);
        if (c > 0) {
            if (c == 15) asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            acc += Wf[((c - 1) & 1) * 2048 + lane * 4];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    acc += Wf[2048 + lane * 4];
    A.out[(int64_t)blockIdx.x * 256 + tid] = acc;
}

enum Shape { GRAD, GRADW, FWD, ACT, REPLAY };
constexpr int ACT_LDS = 80 * 1024;
constexpr int SPIN_TICKS = 250;                 // 2.5 us at 100 MHz

template <bool TILED>
static void launch(Shape s, const Lay &A, const Lay &B, hipStream_t st)
{
    switch (s) {
    case GRAD: hipLaunchKernelGGL((k_grad_shape<TILED, 0>), dim3(207), dim3(256), 0, st, A); break;
    case GRADW: hipLaunchKernelGGL((k_grad_shape<TILED, SPIN_TICKS>), dim3(207), dim3(256), 0, st, A); break;
    case FWD: hipLaunchKernelGGL((k_fwd_shape<TILED>), dim3(64), dim3(256), 0, st, A); break;
    case ACT: hipLaunchKernelGGL((k_act_shape<TILED>), dim3(1024), dim3(256), ACT_LDS, st, A); break;
    case REPLAY:                                 // K1 critic target forward, K2 critic forward (k_mid), K3 critic gradient, K4 actor-side forward, K5 actor gradient
        hipLaunchKernelGGL((k_fwd_shape<TILED>), dim3(64), dim3(256), 0, st, B);
        hipLaunchKernelGGL((k_fwd_shape<TILED>), dim3(64), dim3(256), 0, st, B);
        hipLaunchKernelGGL((k_grad_shape<TILED, 0>), dim3(207), dim3(256), 0, st, B);
        hipLaunchKernelGGL((k_fwd_shape<TILED>), dim3(64), dim3(256), 0, st, A);
        hipLaunchKernelGGL((k_grad_shape<TILED, 0>), dim3(207), dim3(256), 0, st, A);
        break;
    }
}

template <bool TILED>
static void run(const char *what, Shape s, const Lay &A, const Lay &B)
{
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int w = 0; w < 3; ++w) launch<TILED>(s, A, B, 0);
    CHECK(hipDeviceSynchronize());
    std::vector<float> hot, cold;
    constexpr int reps = 20;
    for (int round = 0; round < 7; ++round) {
        CHECK(hipEventRecord(e0, 0));
        for (int r = 0; r < reps; ++r) launch<TILED>(s, A, B, 0);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        hot.push_back(ms * 1e3f / reps);
    }
    if (s != ACT) {
        for (int round = 0; round < 11; ++round) {
            launch<TILED>(ACT, A, B, 0);
            CHECK(hipEventRecord(e0, 0));
            launch<TILED>(s, A, B, 0);
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
            cold.push_back(ms * 1e3f);
        }
    }
    std::sort(hot.begin(), hot.end()); std::sort(cold.begin(), cold.end());
    printf("%-44s hot  min %7.2f  med %7.2f  max %7.2f us", what, hot.front(), hot[hot.size() / 2], hot.back());
    if (!cold.empty()) printf("   behind act  min %7.2f  med %7.2f  max %7.2f us", cold.front(), cold[cold.size() / 2], cold.back());
    printf("\n");
    fflush(stdout);
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

int main()
{
    // Flux order: p, target, m, v as four parameter-vector-shaped arrays per network, back to back (the agent's carve); tiled: one 2 MB
    // region per network.  Everything zero: ADAM on zeros with a small gradient stays finite.
    float *flux, *tiled, *out;
    const size_t fluxN = 8 * VEC, tiledN = 2 * TILED_FLOATS, outN = 1024 * 256;
    CHECK(hipMalloc(&flux, fluxN * 4)); CHECK(hipMalloc(&tiled, tiledN * 4)); CHECK(hipMalloc(&out, outN * 4));
    CHECK(hipMemset(flux, 0, fluxN * 4)); CHECK(hipMemset(tiled, 0, tiledN * 4)); CHECK(hipMemset(out, 0, outN * 4));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_act_shape<false>), hipFuncAttributeMaxDynamicSharedMemorySize, ACT_LDS));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_act_shape<true>), hipFuncAttributeMaxDynamicSharedMemorySize, ACT_LDS));
    AdamCtx c{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 9, 1e-4, 0.9, 0.999, 1.0, 1e-4 / (1.0 - 0.9), 1.0 / (1.0 - 0.999), 1e-3f};
    auto fl = [&](int net, int woff) { float *b = flux + net * 4 * VEC; return Lay{b + 2 * VEC, b + 3 * VEC, b, b + VEC, woff, out, c}; };
    auto tlay = [&](int net) { float *b = tiled + net * TILED_FLOATS; return Lay{b, b, b, b, 0, out, c}; };
    const Lay fa = fl(0, 2500), fc = fl(1, 3000), ta = tlay(0), tc = tlay(1);
    int wg = 0;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, k_act_shape<true>, 256, ACT_LDS));
    printf("single learner, 250 x 500 layer-2 state: Flux order (row pitch 2 000 B, W2 at byte 10 000 / 12 000) against 64 x 64 tiles; act shape: %d workgroups per CU\n", wg);
    struct { Shape s; const char *name; } shapes[] = {{GRAD, "grad"}, {GRADW, "grad+wait"}, {FWD, "fwd"}, {ACT, "act"}, {REPLAY, "replay"}};
    for (int pass = 0; pass < 2; ++pass)           // the whole table twice: the second pass shows the spread between runs of one process
        for (auto &sh : shapes) {
            char b[96];
            snprintf(b, sizeof b, "%-10s Flux order, actor offset", sh.name); run<false>(b, sh.s, fa, fc);
            if (sh.s != REPLAY) { snprintf(b, sizeof b, "%-10s Flux order, critic offset", sh.name); run<false>(b, sh.s, fc, fa); }
            snprintf(b, sizeof b, "%-10s tiled", sh.name); run<true>(b, sh.s, ta, tc);
        }
    CHECK(hipFree(flux)); CHECK(hipFree(tiled)); CHECK(hipFree(out));
    return 0;
}

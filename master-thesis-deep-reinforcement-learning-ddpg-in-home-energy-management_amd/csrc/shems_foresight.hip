// shems_foresight.hip -- the perfect-foresight controller: shems_foresight_solve_dev (backward sweep) and shems_foresight_track_dev
// (greedy forward pass on the exact env).  The recursion itself is csrc/shems_foresight_core.h; this file only spreads it over the GPU.
//
// Backward sweep: one launch per hour t = T - 1 .. 0 (an hour needs the whole V_{t+1} plane of its problem, so hours are separated by
// launch boundaries and by nothing else), grid = (node tiles, problems), 256 threads.  The workgroup stages its problem's V_{t+1} plane
// (65 x 33 nodes: 17 KB) and the two table rows of the hour in LDS; a wave takes `npw` nodes one after the other, the actions of a node
// spread over its 64 lanes (lane l: actions l, l + 64, ... in ascending order, so a strict > keeps the smallest index), and the
// (value, index) maximum is a butterfly over the wave with fs_better -- every lane ends with the same pair, lane 0 stores it.
// Forward pass: one workgroup per env, all T hours inside the kernel (as k_track); the 256 threads evaluate the actions from the env's
// true state against V_{t+1} in L2, the maximum goes wave -> LDS -> thread 0, which steps the env with the ordinary DRL step.
// Receding horizon (shems_foresight_solve_horizon_dev, the schedule: shems_foresight_core.h): one launch, grid = (windows, problems).
// The sweeps of a window depend only on each other, so its workgroup keeps them in LDS: two planes, hour t reads one and writes the
// other, a workgroup barrier between sweeps and nothing else; no workgroup waits on another.  Nodes and actions are spread as in the
// backward sweep (wave w: nodes w, w + waves, ...), and only the planes the forward pass will read leave the CU.
// Planning on a forecast (shems_foresight_solve_forecast_dev / _track_forecast_dev, the belief: shems_foresight_core.h): the same two
// kernels, k_fs_window and k_fs_track, with their rows taken where fs_belief_off says.  The entry point sets the launch-uniform `fc` of
// the kernel's arguments: 0 on the true rows (forecast_off is then not used, whatever the records hold), 1 under a forecast.
// The audit of tracked passes (shems_foresight_audit_dev, the definition: shems_foresight_core.h): k_fs_audit, one launch over
// passes x hours x actions, a wave per hour, V planes read from global memory, no LDS and no barrier.
// Hedging over a forecast ensemble (shems_foresight_track_ensemble_dev, the definition: shems_foresight_core.h): the K scenario sweeps
// are K records of solve_forecast_dev; k_fs_track_ens is the forward pass that weighs every action against all K planes.
// One kernel per role.  What the kernels share exists once: the wave maximum (fs_wave_best, all five reductions) and, for the two forward
// kernels, the block maximum, thread 0's step-and-record and the final stores (fs_block_best, fs_step_record, fs_track_store).
//
// Compiled with -ffp-contract=off (shems_core.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "shems_env_dev.h"
#include "shems_foresight_core.h"
#include "shems_internal.h"

namespace shems {

constexpr int kFsThreads = 256, kFsWaves = kFsThreads / 64;
constexpr int kFsMaxPlaneBytes = 150000;           // of the 160 KB of LDS a gfx950 workgroup can hold
// k_fs_window: 16 waves, all a CU holds at the kernel's registers, in ONE workgroup -- whatever its two planes take of the CU's LDS
// (34 KB at the default grid, 134 KB at 129 x 65), the CU is full.  A measuring build may set another size (_build.build(defines=...)).
#ifndef SHEMS_FS_WINDOW_THREADS
#define SHEMS_FS_WINDOW_THREADS 1024
#endif
constexpr int kFsWindowThreads = SHEMS_FS_WINDOW_THREADS;
static_assert(kFsWindowThreads % 64 == 0 && kFsWindowThreads >= 64 && kFsWindowThreads <= 1024, "whole waves, at most 16");

// The (value, index) maximum over a wave: a butterfly with fs_better, so every lane ends with the same pair -- the first maximum,
// whatever lane held it.
__device__ __forceinline__ void fs_wave_best(double &best_v, int &best_a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best_v, off, 64);
        const int oa = __shfl_xor(best_a, off, 64);
        if (fs_better(ov, oa, best_v, best_a)) { best_v = ov; best_a = oa; }
    }
}

struct FsSolveArgs {
    const float *tables;
    const shems_foresight_problem *prob;
    FsParams g;
    int T, t, npw;                                 // npw: nodes per wave (a tile = kFsWaves * npw nodes)
    double *V;
    int32_t *arg;
};

__global__ __launch_bounds__(kFsThreads) void k_fs_zero(double *V, int64_t plane, int64_t stride, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;       // V_T = 0: the last plane of every problem
    if (i < total) V[(i / plane) * stride + (stride - plane) + i % plane] = 0.0;
}

// 4 waves per SIMD: left alone the compiler takes 129 VGPRs, one past the step from 4 resident waves to 3; held to 4 it takes 127, no scratch.
__global__ __launch_bounds__(kFsThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_fs_backward(FsSolveArgs A)
{
    extern __shared__ __attribute__((aligned(16))) double s_v[];            // V_{t+1} [nb * ne]
    __shared__ float s_row[2 * SHEMS_NCOL];                                 // rows idx0 + t and idx0 + t + 1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.y;
    const FsParams &g = A.g;
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    const shems_foresight_problem P = A.prob[p];
    double *Vt = A.V + ((int64_t)p * (A.T + 1) + A.t) * N;
    const double *Vn = Vt + N;
    for (int i = tid; i < N; i += kFsThreads) s_v[i] = Vn[i];
    if (tid < 2 * SHEMS_NCOL) s_row[tid] = A.tables[((int64_t)P.cfg.table_row0 + P.idx0 + A.t - 1) * SHEMS_NCOL + tid];
    __syncthreads();
    const float h_cur = s_row[0], h_next = s_row[SHEMS_NCOL], soc_ev_next = s_row[SHEMS_NCOL + 1];
    for (int k = 0; k < A.npw; ++k) {
        const int node = ((int)blockIdx.x * kFsWaves + wave) * A.npw + k;   // wave-uniform
        if (node >= N) break;
        const int ib = node / g.ne, ie = node - ib * g.ne;
        const EnvIn s{fs_soc_b_node(P, g.nb, ib), fs_soc_ev_node(g, ie), h_cur, s_row[2], s_row[3], s_row[4]};
        double best_v = -__builtin_inf();
        int best_a = kFsNoAction;
        for (int a = lane; a < NA; a += 64) {
            const int ab = a / g.nae, ae = a - ab * g.nae;
            const double q = fs_q(P.cfg, s, h_cur, h_next, soc_ev_next, fs_target(ab, g.nab), fs_target(ae, g.nae), s_v, g, P.scale_b);
            if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
        }
        fs_wave_best(best_v, best_a);
        if (lane == 0) {
            Vt[node] = best_v;
            if (A.arg) A.arg[((int64_t)p * A.T + A.t) * N + node] = best_a;
        }
    }
}

struct FsWindowArgs {
    const float *tables;
    const shems_foresight_problem *prob;
    FsParams g;
    int T, H, c;                                   // hours of the pass, horizon, control
    int fc;                                        // launch-uniform: 1 = the plans read a forecast (the belief: shems_foresight_core.h)
    double *V;
    int32_t *arg;
};

// One workgroup = one plan: window j = blockIdx.x * c of problem blockIdx.y, hours hi - 1 down to fs_plan_first.  Sweep k stages its
// two table rows in s_row[k & 1], reads plane k & 1 and writes the other; the one barrier per sweep orders all three (a wave that is
// one sweep ahead writes what the sweep before the slower waves' current one read).  Registers as k_fs_backward: held to 4 waves per
// SIMD (128 VGPRs), no scratch.
// A.fc: the plan's belief (shems_foresight_core.h): the two rows of a sweep no longer sit next to each other in memory, so lanes 0-7 of
// wave 0 load the current row and lanes 8-15 the next, each from its own wave-uniform base formed inside the sweep.
__global__ __launch_bounds__(kFsWindowThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_fs_window(FsWindowArgs A)
{
    extern __shared__ __attribute__((aligned(16))) double s_v[];            // [2][nb * ne]
    __shared__ float s_row[2][2 * SHEMS_NCOL];                              // rows idx0 + t and idx0 + t + 1 of the sweep's hour
    constexpr int threads = kFsWindowThreads, waves = threads / 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);              // the same in every lane: node indices stay in scalar registers
    const int p = blockIdx.y, j = (int)blockIdx.x * A.c;
    const FsParams &g = A.g;
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    const shems_foresight_problem P = A.prob[p];
    const int hi = fs_plan_end(j, A.H, A.T), lo = fs_plan_first(j, A.arg != nullptr);
    double *Vp = A.V + (int64_t)p * (A.T + 1) * N;
    int32_t *argp = A.arg ? A.arg + (int64_t)p * A.T * N : nullptr;
    const bool zeros_out = fs_plan_keeps_plane(j, A.c, A.T, hi);            // U_hi = 0: the plane the forward pass reads at hour hi - 1
    for (int i = tid; i < N; i += threads) {
        s_v[i] = 0.0;
        if (zeros_out) Vp[(int64_t)hi * N + i] = 0.0;
    }
    int cur = 0;
    for (int t = hi - 1; t >= lo; --t, cur ^= 1) {
        const float *rows = A.tables + ((int64_t)P.cfg.table_row0 + P.idx0 + t - 1) * SHEMS_NCOL;      // the same address in every lane
        if (wave == 0) {
            int l = lane;
            asm volatile("" : "+v"(l));                                      // formed here: no per-lane address lives across the sweeps
            if (A.fc) {
                const float *r0 = rows + (int64_t)fs_belief_off(t, j, P.forecast_off) * SHEMS_NCOL;                  // hour t
                const float *r1 = rows + ((int64_t)fs_belief_off(t + 1, j, P.forecast_off) + 1) * SHEMS_NCOL;        // hour t + 1
                if (l < 2 * SHEMS_NCOL) s_row[cur][l] = (l < SHEMS_NCOL ? r0 : r1)[l & (SHEMS_NCOL - 1)];
            } else {
                if (l < 2 * SHEMS_NCOL) s_row[cur][l] = rows[l];
            }
        }
        __syncthreads();
        const float *row = s_row[cur];
        const double *Vn = s_v + cur * N;
        double *Vt = s_v + (cur ^ 1) * N;
        const bool v_out = fs_plan_keeps_plane(j, A.c, A.T, t), a_out = argp && fs_plan_keeps_argmax(j, A.c, A.T, t);
        const float h_cur = row[0], h_next = row[SHEMS_NCOL], soc_ev_next = row[SHEMS_NCOL + 1];
        for (int node = wave; node < N; node += waves) {                    // wave-uniform
            const int ib = node / g.ne, ie = node - ib * g.ne;
            const EnvIn s{fs_soc_b_node(P, g.nb, ib), fs_soc_ev_node(g, ie), h_cur, row[2], row[3], row[4]};
            double best_v = -__builtin_inf();
            int best_a = kFsNoAction;
            for (int a = lane; a < NA; a += 64) {
                const int ab = a / g.nae, ae = a - ab * g.nae;
                const double q = fs_q(P.cfg, s, h_cur, h_next, soc_ev_next, fs_target(ab, g.nab), fs_target(ae, g.nae), Vn, g, P.scale_b);
                if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
            }
            fs_wave_best(best_v, best_a);
            if (lane == 0) {
                Vt[node] = best_v;
                if (v_out) Vp[(int64_t)t * N + node] = best_v;
                if (a_out) argp[(int64_t)t * N + node] = best_a;
            }
        }
    }
}

struct FsTrackArgs {
    shems_view v;
    const shems_foresight_problem *prob;
    int n_prob;
    int fc;                                        // launch-uniform: 1 = the next row comes from the record's forecast table
    const int32_t *problem_of_env;
    FsParams g;
    int T;
    const double *V;
    double *results;                               // [n or 1][T][23] or null
    int64_t results_env;
    double *returns;                               // [n] or null
    float *targets;                                // [n][T][2] or null
};

// ---- what the two forward kernels (k_fs_track, k_fs_track_ens) share: one workgroup of kFsThreads per env ----
struct FsTrackLds {
    float obs[SHEMS_NSTATE];                       // the env's state, published by thread 0 after every step
    double bv[kFsWaves];                           // the waves' maxima
    int ba[kFsWaves];
};

// The block maximum: wave -> LDS -> thread 0, which alone ends with the workgroup's pair.  Holds the one barrier between the two.
__device__ __forceinline__ void fs_block_best(FsTrackLds &S, double &best_v, int &best_a)
{
    const int tid = threadIdx.x;
    fs_wave_best(best_v, best_a);
    if ((tid & 63) == 0) { S.bv[tid >> 6] = best_v; S.ba[tid >> 6] = best_a; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kFsWaves; ++w)
            if (fs_better(S.bv[w], S.ba[w], best_v, best_a)) { best_v = S.bv[w]; best_a = S.ba[w]; }
    }
}

// Thread 0's step-and-record of hour t: the winning action steps env e with the ordinary DRL step, the results and targets rows are
// written and the new state is published in S.obs.  The caller has checked that row idx + 1 exists.
__device__ __forceinline__ void fs_step_record(const FsTrackArgs &A, const shems_config &cfg, int64_t e, int t, int best_a, FsTrackLds &S,
                                               float (&obs)[SHEMS_NSTATE], int32_t &idx, int32_t &step, double &total)
{
    const FsParams &g = A.g;
    const int a = best_a == kFsNoAction ? 0 : best_a;                       // every Q a NaN: cannot happen on finite tables
    const int ab = a / g.nae, ae = a - ab * g.nae;
    const float a0 = fs_target(ab, g.nab), a1 = fs_target(ae, g.nae);
    float pre[SHEMS_NSTATE];
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) pre[k] = obs[k];
    double reward;
    StepFlows f;
    float B, EV, Bt, EVt;
    env_advance(cfg, A.v.tables, obs, idx, step, a0, a1, SHEMS_TRACK_DRL, reward, f, B, EV, Bt, EVt);
    total += reward;
    if (A.results && (A.results_env < 0 || A.results_env == e)) {
        double *r = A.results + ((A.results_env < 0 ? e : 0) * (int64_t)A.T + t) * SHEMS_NRESULT;
        write_results(r, idx, pre, EVt, EV, reward, f, B, Bt);
    }
    if (A.targets) {
        float *tg = A.targets + (e * (int64_t)A.T + t) * 2;
        tg[0] = a0; tg[1] = a1;
    }
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) S.obs[k] = obs[k];
}

// Thread 0's final stores: the env where the pass left it, and its total.
__device__ __forceinline__ void fs_track_store(const FsTrackArgs &A, int64_t e, const float (&obs)[SHEMS_NSTATE], int32_t idx, int32_t step,
                                               double total)
{
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) A.v.obs[e * SHEMS_NSTATE + k] = obs[k];
    A.v.idx[e] = idx;
    A.v.step[e] = step;
    if (A.returns) A.returns[e] = total;
}

// The forward pass on one value function.  A.fc: the controller does not know row t + 1 yet: h_countdown / soc_ev of the next row come
// from the forecast table, which must lie inside the row array (checked here, against the view's total_rows: the records may come from
// a solve on another array).  Without it forecast_off is not used and that check is skipped.
__global__ __launch_bounds__(kFsThreads) void k_fs_track(FsTrackArgs A)
{
    __shared__ FsTrackLds S;
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    const shems_view &v = A.v;
    const FsParams &g = A.g;
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    // ---- entry checks, the same answer in every thread ----
    const int p = A.problem_of_env ? A.problem_of_env[e] : 0;
    int32_t idx = v.idx[e], step = v.step[e];
    if (p < 0 || p >= A.n_prob || A.prob[p].idx0 != idx) {
        if (tid == 0) raise(v.err, SHEMS_ERR_INDEX);
        return;
    }
    const shems_foresight_problem P = A.prob[p];
    if (A.fc && ((int64_t)P.cfg.table_row0 + P.forecast_off < 0 || (int64_t)P.cfg.table_row0 + P.forecast_off + P.cfg.nrow > v.total_rows)) {
        if (tid == 0) raise(v.err, SHEMS_ERR_INDEX);
        return;
    }
    const int forecast_off = A.fc ? P.forecast_off : 0;                     // fc == 0: the member is ignored, whatever the record holds
    const shems_config cfg = load_cfg(v, e);                                // the env's own config steps the env
    float obs[SHEMS_NSTATE];
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) obs[k] = v.obs[e * SHEMS_NSTATE + k];
    if (tid < SHEMS_NSTATE) S.obs[tid] = v.obs[e * SHEMS_NSTATE + tid];
    __syncthreads();
    double total = 0.0;
    for (int t = 0; t < A.T; ++t) {
        if (idx < 1 || idx + 1 > cfg.nrow || idx + 1 > P.cfg.nrow) {       // row idx + 1 does not exist (Julia: BoundsError)
            if (tid == 0) raise(v.err, SHEMS_ERR_INDEX);
            break;
        }
        const double *Vn = A.V + ((int64_t)p * (A.T + 1) + t + 1) * N;
        const float h_cur = load_h(v.tables, P.cfg.table_row0, idx);
        const int64_t next0 = (int64_t)P.cfg.table_row0 + fs_belief_off(t + 1, t, forecast_off);
        const float h_next = load_h(v.tables, next0, idx + 1);
        const float soc_ev_next = v.tables[(next0 + idx) * SHEMS_NCOL + 1];
        const EnvIn s{S.obs[0], S.obs[1], S.obs[2], S.obs[3], S.obs[4], S.obs[5]};
        double best_v = -__builtin_inf();
        int best_a = kFsNoAction;
        for (int a = tid; a < NA; a += kFsThreads) {
            const int ab = a / g.nae, ae = a - ab * g.nae;
            const double q = fs_q(P.cfg, s, h_cur, h_next, soc_ev_next, fs_target(ab, g.nab), fs_target(ae, g.nae), Vn, g, P.scale_b);
            if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
        }
        fs_block_best(S, best_v, best_a);
        if (tid == 0) fs_step_record(A, cfg, e, t, best_a, S, obs, idx, step, total);
        else idx += 1;                                                       // every thread follows the row index
        __syncthreads();
    }
    if (tid == 0) fs_track_store(A, e, obs, idx, step, total);
}

struct FsTrackEnsArgs {
    FsTrackArgs t;                                 // prob: n_prob * K records, problem-major, scenario-minor; V: their planes
    int K;                                         // scenarios per problem, 1 .. kFsMaxScen
    const double *w;                               // [n_prob][K] weights, device memory
};

// The forward pass hedging over K scenarios (the definition: shems_foresight_core.h).  Shaped like k_fs_track under a forecast: one
// workgroup per env, all T hours in the launch.  The K weights and row offsets of the workgroup's problem go to LDS once; per hour
// threads 0 .. K - 1 stage (h_countdown, soc_ev) of every scenario's row t + 1 there, then thread `tid` takes actions tid, tid + 256,
// ...: the DRL step once (fs_step), then the K lookups against the K planes in global memory (every env of a problem reads the same
// planes: L2), added in scenario order inside the thread (fs_q_ens) -- no partial sum crosses a lane.  The maximum, the step and the
// stores are k_fs_track's (fs_block_best, fs_step_record, fs_track_store).
__global__ __launch_bounds__(kFsThreads) void k_fs_track_ens(FsTrackEnsArgs E)
{
    __shared__ FsTrackLds S;
    __shared__ double s_w[kFsMaxScen];
    __shared__ int s_off[kFsMaxScen];
    __shared__ float s_hn[kFsMaxScen], s_sn[kFsMaxScen];
    const FsTrackArgs &A = E.t;
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    const shems_view &v = A.v;
    const FsParams &g = A.g;
    const int K = E.K;
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    // ---- entry checks, the same answer in every thread ----
    const int p = A.problem_of_env ? A.problem_of_env[e] : 0;
    int32_t idx = v.idx[e], step = v.step[e];
    bool ok = K >= 1 && K <= kFsMaxScen && p >= 0 && p < A.n_prob && A.prob[(int64_t)p * K].idx0 == idx;
    if (ok) {
        const shems_foresight_problem *R = A.prob + (int64_t)p * K;
        const int32_t row0 = R[0].cfg.table_row0, nrow = R[0].cfg.nrow;
        ok = row0 >= 0 && nrow >= 2 && (int64_t)row0 + nrow <= v.total_rows;
        for (int k = 0; k < K; ++k) {
            const int64_t f0 = (int64_t)row0 + R[k].forecast_off;
            ok = ok && R[k].idx0 == idx && R[k].cfg.table_row0 == row0 && R[k].cfg.nrow == nrow && f0 >= 0 && f0 + nrow <= v.total_rows;
        }
    }
    if (!ok) {
        if (tid == 0) raise(v.err, SHEMS_ERR_INDEX);
        return;
    }
    const shems_foresight_problem P = A.prob[(int64_t)p * K];              // the truth: scenario 0's record without its offset
    if (tid < K) {
        s_w[tid] = E.w[(int64_t)p * K + tid];
        s_off[tid] = A.prob[(int64_t)p * K + tid].forecast_off;
    }
    const shems_config cfg = load_cfg(v, e);                                // the env's own config steps the env
    float obs[SHEMS_NSTATE];
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) obs[k] = v.obs[e * SHEMS_NSTATE + k];
    if (tid < SHEMS_NSTATE) S.obs[tid] = v.obs[e * SHEMS_NSTATE + tid];
    __syncthreads();
    const int64_t v_stride = (int64_t)(A.T + 1) * N;
    double total = 0.0;
    for (int t = 0; t < A.T; ++t) {
        if (idx < 1 || idx + 1 > cfg.nrow || idx + 1 > P.cfg.nrow) {       // row idx + 1 does not exist (Julia: BoundsError)
            if (tid == 0) raise(v.err, SHEMS_ERR_INDEX);
            break;
        }
        if (tid < K) {                                                      // scenario tid's row t + 1 (inside the array: entry checks)
            const int64_t next0 = (int64_t)P.cfg.table_row0 + fs_belief_off(t + 1, t, s_off[tid]);
            s_hn[tid] = load_h(v.tables, next0, idx + 1);
            s_sn[tid] = v.tables[(next0 + idx) * SHEMS_NCOL + 1];
        }
        __syncthreads();
        const double *Vn = A.V + ((int64_t)p * K * (A.T + 1) + t + 1) * N;  // plane t + 1 of scenario 0
        const float h_cur = load_h(v.tables, P.cfg.table_row0, idx);
        const EnvIn s{S.obs[0], S.obs[1], S.obs[2], S.obs[3], S.obs[4], S.obs[5]};
        double best_v = -__builtin_inf();
        int best_a = kFsNoAction;
        for (int a = tid; a < NA; a += kFsThreads) {
            const int ab = a / g.nae, ae = a - ab * g.nae;
            const FsStep st = fs_step(P.cfg, s, fs_target(ab, g.nab), fs_target(ae, g.nae));
            const double q = fs_q_ens(st, h_cur, K, s_w, s_hn, s_sn, Vn, v_stride, g, P.scale_b);
            if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
        }
        fs_block_best(S, best_v, best_a);
        if (tid == 0) fs_step_record(A, cfg, e, t, best_a, S, obs, idx, step, total);
        else idx += 1;                                                       // every thread follows the row index
        __syncthreads();
    }
    if (tid == 0) fs_track_store(A, e, obs, idx, step, total);
}

struct FsAuditArgs {
    const float *tables;
    int64_t total_rows;
    const shems_foresight_problem *prob;
    int n_prob;
    const int32_t *problem_of_pass;                // [n] or null: problem 0
    FsParams g;
    int T;
    const double *V;
    const double *results;                         // [n][T][23]
    double *out;                                   // [n][T][3]: best_q, achieved_q, v_state
    int32_t *best_action;                          // [n][T]
    int32_t *status;                               // [n], zeroed on the stream before the launch
};

// The audit of tracked passes (the definition: shems_foresight_core.h).  Hours are independent: grid = (tiles of kFsWaves hours,
// passes), a wave owns one hour, lane l takes actions l, l + 64, ... against the V_{t+1} plane in global memory (every pass of a
// problem reads the same plane at the same hour: L2), the fs_better butterfly finishes the maximum, lane 0 adds achieved_q and v_state
// and stores.  No LDS, no barrier: a wave past the last hour, or one whose row is refused, simply leaves.
__global__ __launch_bounds__(kFsThreads) void k_fs_audit(FsAuditArgs A)
{
    const int lane = threadIdx.x & 63;
    const int t = (int)blockIdx.x * kFsWaves + (int)(threadIdx.x >> 6);     // wave-uniform
    if (t >= A.T) return;
    const int64_t e = blockIdx.y;
    const FsParams &g = A.g;
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    const int p = A.problem_of_pass ? A.problem_of_pass[e] : 0;
    const double *r = A.results + (e * A.T + t) * SHEMS_NRESULT;
    double *o = A.out + (e * A.T + t) * 3;
    shems_foresight_problem P;
    FsAuditHour h;
    bool ok = p >= 0 && p < A.n_prob;
    if (ok) {
        P = A.prob[p];
        ok = fs_audit_hour(P, A.tables, A.total_rows, r, t, h);
    }
    if (!ok) {                                                              // every writer of status[e] stores the same value
        if (lane == 0) {
            o[0] = o[1] = o[2] = __builtin_nan("");
            A.best_action[e * A.T + t] = -1;
            A.status[e] = SHEMS_ERR_INDEX;
        }
        return;
    }
    const double *Vt = A.V + ((int64_t)p * (A.T + 1) + t) * N, *Vn = Vt + N;
    double best_v = -__builtin_inf();
    int best_a = kFsNoAction;
    for (int a = lane; a < NA; a += 64) {
        const double q = fs_audit_q(P, h, a, Vn, g);
        if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
    }
    fs_wave_best(best_v, best_a);
    if (lane == 0) {
        o[0] = best_v;
        o[1] = fs_audit_achieved(P, r, t + 1 < A.T ? r + SHEMS_NRESULT : nullptr, Vn, g);
        o[2] = fs_audit_v_state(P, h, Vt, g);
        A.best_action[e * A.T + t] = best_a == kFsNoAction ? -1 : best_a;   // every Q a NaN: cannot happen on finite tables
    }
}

// ---- demonstrations: result rows + labels -> (observation, action) pairs in a replay ring (fs_demo_hour, csrc/shems_foresight_core.h) ----
struct FsDemosArgs {
    const float *tables;
    int64_t total_rows;
    const shems_foresight_problem *prob;
    int n_prob;
    const int32_t *problem_of_pass;
    FsParams g;
    int T;
    const double *results;
    const float *targets;              // [n_pass][T][2], or null
    const int32_t *best_action;        // [n_pass][T], or null (exactly one of the two is given)
    float *s, *a;                      // the ring's observation and action arrays
    int64_t capacity, pos;
    int32_t *status;
};

// Grid = (tiles of kFsThreads hours, passes), one thread per hour: a few hundred bytes in, eleven floats out, nothing shared.  The
// entry point has held n_pass * T to the capacity, so no two threads write one slot; a refused hour leaves its slot alone.
__global__ __launch_bounds__(kFsThreads) void k_fs_demos(FsDemosArgs A)
{
    const int t = (int)blockIdx.x * kFsThreads + (int)threadIdx.x;
    if (t >= A.T) return;
    const int64_t e = blockIdx.y;
    const int p = A.problem_of_pass ? A.problem_of_pass[e] : 0;
    const int64_t at = e * A.T + t;
    FsDemo d;
    bool ok = p >= 0 && p < A.n_prob;
    if (ok) {
        const shems_foresight_problem P = A.prob[p];
        ok = fs_demo_hour(P, A.tables, A.total_rows, A.results + at * SHEMS_NRESULT, t, A.targets ? A.targets + at * 2 : nullptr,
                          A.best_action ? A.best_action[at] : -1, A.g, d);
    }
    if (!ok) {                                                              // every writer of status[e] stores the same value
        A.status[e] = SHEMS_ERR_INDEX;
        return;
    }
    const int64_t slot = fs_demo_slot(A.pos, e, A.T, t, A.capacity);
    float *ps = A.s + slot * SHEMS_NSTATE;
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) ps[k] = d.s[k];
    A.a[slot * 2] = d.a[0];
    A.a[slot * 2 + 1] = d.a[1];
}

// ---- transitions: result rows -> (s, a, r, s', done) in a replay ring, and the returns-to-go of the passes (fs_transition_hour,
// fs_returns, csrc/shems_foresight_core.h) ----
struct FsTransArgs {
    const float *tables;
    int64_t total_rows;
    const shems_foresight_problem *prob;
    int n_prob;
    const int32_t *problem_of_pass;
    int T, tail, mode;
    float gamma;
    const double *results;
    double *returns;                   // [n_pass][T], or null (TD only)
    float *s, *a, *r, *s2;             // the ring's arrays
    uint8_t *done;
    int64_t capacity, pos;
    int32_t *status;
};

__device__ __forceinline__ double fs_wave_lane(double x, int lane)         // lane: uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// One wave per pass.  The recurrence is one dependent chain per pass: the wave takes the pass in chunks of 64 hours from the end, every
// lane loads and checks ITS hour (the next chunk's loads are issued before this chunk's chain), then all lanes walk the chunk's 64
// steps together on rewards read out of each other's registers -- the chain never waits for memory -- and lane j keeps step j's value.
// G[T - 1] is read before the loop and only the last chunk, which may be short, is walked with a bound: a step of a full chunk is the
// product, the sum and six instructions beside them.  The order of fs_returns, whatever T.  A refused pass (MC's verdict, core
// header) gets fs_returns_refused() in every hour, which is what k_fs_transitions reads of it; status[e] is written in MC mode only.
__global__ __launch_bounds__(64) void k_fs_returns(FsTransArgs A)
{
    const int lane = (int)threadIdx.x;
    const int64_t e = blockIdx.x;
    const int p = A.problem_of_pass ? A.problem_of_pass[e] : 0;
    const bool known = p >= 0 && p < A.n_prob;
    const shems_foresight_problem P = A.prob[known ? p : 0];
    const double *res = A.results + e * A.T * SHEMS_NRESULT;
    double *out = A.returns + e * A.T;
    const double g = (double)A.gamma;
    auto load = [&](int c, double &rew, bool &ok) {
        const int t = c * 64 + lane;
        rew = 0.0; ok = true;
        if (t < A.T) {
            const double *r = res + (int64_t)t * SHEMS_NRESULT;
            rew = r[5];
            ok = fs_returns_hour_ok(P, A.tables, A.total_rows, r, t);
        }
    };
    const int last = A.T - 1, nchunk = last / 64 + 1;
    bool bad = !known, ok, ok_next = true;
    double rew, rew_next = 0.0;
    load(nchunk - 1, rew, ok);
    double G = fs_wave_lane(rew, last & 63);                                // G[T - 1] = r[T - 1][5]: the chain starts at hour T - 2
    auto step = [&](int j, double &mine) {                                  // j: uniform
        G = fs_return_step(fs_wave_lane(rew, j), g, G);
        if (lane == j) mine = G;
    };
    for (int c = nchunk - 1; c >= 0; --c) {
        if (c > 0) load(c - 1, rew_next, ok_next);
        bad = bad || !ok;
        double mine = G;                                                    // the lane of hour T - 1 keeps this; every other lane that stores takes a step's
        if (c == nchunk - 1) {                                              // the one chunk that may be short: hours T - 2 down to its first
#pragma unroll 1
            for (int j = (last & 63) - 1; j >= 0; --j) step(j, mine);
        } else {
#pragma unroll 1
            for (int q = 3; q >= 0; --q) {                                  // 16 rewards in scalar registers at a time, no branch inside
#pragma unroll
                for (int u = 15; u >= 0; --u) step(q * 16 + u, mine);
            }
        }
        if (c * 64 + lane < A.T) out[c * 64 + lane] = mine;
        rew = rew_next; ok = ok_next;
    }
    if (__any(bad)) {
        for (int t = lane; t < A.T; t += 64) out[t] = fs_returns_refused();     // the same lane stored hour t above
        if (A.mode == SHEMS_FS_TRANS_MC && lane == 0) A.status[e] = SHEMS_ERR_INDEX;
    }
}

// Grid = (tiles of kFsThreads hours, passes), one thread per hour with a successor, as k_fs_demos.  The entry point has held
// n_pass * (T - tail) to the capacity, so no two threads write one slot.  MC: the verdict of the pass is the NaN k_fs_returns left in
// its first return (not the status word, which the host reads); every writer of status[e] stores the same value.
__global__ __launch_bounds__(kFsThreads) void k_fs_transitions(FsTransArgs A)
{
    const int t = (int)blockIdx.x * kFsThreads + (int)threadIdx.x;
    const int keep = A.T - A.tail;
    if (t >= keep) return;
    const int64_t e = blockIdx.y;
    const bool mc = A.mode == SHEMS_FS_TRANS_MC;
    float ret = 0.0f;
    if (mc) {
        const double G0 = A.returns[e * A.T];
        if (G0 != G0) return;
        ret = (float)A.returns[e * A.T + t];
    }
    const int p = A.problem_of_pass ? A.problem_of_pass[e] : 0;
    FsTransition x;
    bool ok = p >= 0 && p < A.n_prob;
    if (ok) {
        const shems_foresight_problem P = A.prob[p];
        ok = fs_transition_hour(P, A.tables, A.total_rows, A.results + (e * A.T + t) * SHEMS_NRESULT, t, x);
    }
    if (!ok) {
        A.status[e] = SHEMS_ERR_INDEX;
        return;
    }
    const int64_t slot = fs_demo_slot(A.pos, e, keep, t, A.capacity);
    float *ps = A.s + slot * SHEMS_NSTATE, *ps2 = A.s2 + slot * SHEMS_NSTATE;
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) { ps[k] = x.d.s[k]; ps2[k] = x.s2[k]; }
    A.a[slot * 2] = x.d.a[0];
    A.a[slot * 2 + 1] = x.d.a[1];
    A.r[slot] = mc ? ret : x.rew;
    A.done[slot] = mc ? 1 : 0;
}

static int fs_params(const shems_foresight_grid *grid, const char *fn, FsParams &g)
{
    if (!grid) return set_error(SHEMS_ERR_ARG, "%s: grid is NULL", fn);
    if (grid->nb < 2 || grid->ne < 2)
        return set_error(SHEMS_ERR_ARG, "%s: the state grid is %d x %d nodes; each axis needs at least 2", fn, (int)grid->nb, (int)grid->ne);
    if (grid->nab < 1 || grid->nae < 1)
        return set_error(SHEMS_ERR_ARG, "%s: the action grid is %d x %d targets; each axis needs at least 1", fn, (int)grid->nab, (int)grid->nae);
    if ((int64_t)grid->nb * grid->ne * 8 > kFsMaxPlaneBytes)
        return set_error(SHEMS_ERR_ARG, "%s: a V plane of %d x %d nodes does not fit the %d bytes of LDS a workgroup stages", fn, (int)grid->nb,
                         (int)grid->ne, kFsMaxPlaneBytes);
    if ((int64_t)grid->nab * grid->nae > (1 << 24))
        return set_error(SHEMS_ERR_ARG, "%s: %d x %d action targets are more than 2^24", fn, (int)grid->nab, (int)grid->nae);
    g.nb = grid->nb; g.ne = grid->ne; g.nab = grid->nab; g.nae = grid->nae;
    g.scale_e = (double)(grid->ne - 1);
    g.he = 1.0 / (double)(grid->ne - 1);
    return SHEMS_OK;
}

// What both backward entry points check before any HIP call: the grid, T, the buffers and every problem record (`recs` receives the
// records completed with scale_b / hb, as the kernels read them; forecast_off is kept and its table held to the row array with
// `forecast`, written 0 otherwise); fs_check_v: the size of the V buffer.
static int fs_check_solve(const char *fn, const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                          const shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid, int32_t T,
                          const double *d_V, FsParams &g, std::vector<shems_foresight_problem> &recs, bool forecast = false)
{
    if (int rc = fs_params(grid, fn, g)) return rc;
    if (T < 1) return set_error(SHEMS_ERR_ARG, "%s: T = %d; the horizon must be at least 1 hour", fn, (int)T);
    if (!d_tables || total_rows < 2 || !problems || !d_problems || n_problems < 1 || n_problems > 65535 || !d_V)
        return set_error(SHEMS_ERR_ARG, "%s: NULL buffer, fewer than 2 table rows, or a problem count outside 1 .. 65535", fn);
    recs.assign(problems, problems + n_problems);                            // validated and completed here, then uploaded
    for (int32_t p = 0; p < n_problems; ++p) {
        shems_foresight_problem &P = recs[p];
        if (P.cfg.table_row0 < 0 || P.cfg.nrow < 2 || (int64_t)P.cfg.table_row0 + P.cfg.nrow > total_rows)
            return set_error(SHEMS_ERR_ARG, "%s: problem %d names table rows %d .. %lld of %lld", fn, (int)p, (int)P.cfg.table_row0,
                             (long long)P.cfg.table_row0 + P.cfg.nrow, (long long)total_rows);
        if (P.idx0 < 1 || (int64_t)P.idx0 + T > P.cfg.nrow)
            return set_error(SHEMS_ERR_ARG, "%s: problem %d: the window of rows %d .. %lld runs off its table of %d rows (a pass of T steps reads row idx0 + T)",
                             fn, (int)p, (int)P.idx0, (long long)P.idx0 + T, (int)P.cfg.nrow);
        if (!(P.cfg.soc_max > 0.0f)) return set_error(SHEMS_ERR_ARG, "%s: problem %d: soc_max = %g must be positive", fn, (int)p, (double)P.cfg.soc_max);
        if (!forecast) P.forecast_off = 0;
        const int64_t f0 = (int64_t)P.cfg.table_row0 + P.forecast_off;
        if (f0 < 0 || f0 + P.cfg.nrow > total_rows)
            return set_error(SHEMS_ERR_ARG, "%s: problem %d: its forecast table (forecast_off = %d) names rows %lld .. %lld of %lld", fn, (int)p,
                             (int)P.forecast_off, (long long)f0, (long long)(f0 + P.cfg.nrow), (long long)total_rows);
        P.scale_b = (double)(g.nb - 1) / (double)P.cfg.soc_max;             // the only divisions of the sweep: float64, on the host
        P.hb = (double)P.cfg.soc_max / (double)(g.nb - 1);
    }
    return SHEMS_OK;
}

static int fs_check_v(const char *fn, int32_t n_problems, int32_t T, int64_t N, int64_t v_doubles)
{
    if (v_doubles < (int64_t)n_problems * (T + 1) * N)
        return set_error(SHEMS_ERR_ARG, "%s: the V buffer holds %lld float64; %d problems x %d planes x %lld nodes need %lld", fn, (long long)v_doubles,
                         (int)n_problems, (int)T + 1, (long long)N, (long long)n_problems * (T + 1) * N);
    return SHEMS_OK;
}

// the records the kernels (and the forward pass) read: ordered on the stream; the runtime has staged a pageable source on return
static int fs_upload(const std::vector<shems_foresight_problem> &recs, shems_foresight_problem *d_problems, hipStream_t st)
{
    return hip_ok(hipMemcpyAsync(d_problems, recs.data(), recs.size() * sizeof(shems_foresight_problem), hipMemcpyHostToDevice, st),
                  "upload of the problem records");
}

}  // namespace shems

using namespace shems;

extern "C" int shems_foresight_solve_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                                         shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid,
                                         int32_t T, double *d_V, int64_t v_doubles, int32_t *d_argmax, void *stream)
{
    const char *fn = "shems_foresight_solve_dev";
    FsParams g;
    std::vector<shems_foresight_problem> recs;
    if (int rc = fs_check_solve(fn, d_tables, total_rows, problems, d_problems, n_problems, grid, T, d_V, g, recs)) return rc;
    const int64_t N = (int64_t)g.nb * g.ne;
    if (int rc = fs_check_v(fn, n_problems, T, N, v_doubles)) return rc;
    const int lds = (int)(N * 8);
    static std::atomic<uint64_t> optin{0};                                  // per device, once: the largest plane fs_params admits
    if (int rc = lds_optin(optin, (const void *)k_fs_backward, kFsMaxPlaneBytes, "hipFuncSetAttribute(k_fs_backward)")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = fs_upload(recs, d_problems, st)) return rc;
    const int64_t total = (int64_t)n_problems * N;
    hipLaunchKernelGGL(k_fs_zero, dim3((unsigned)((total + kFsThreads - 1) / kFsThreads)), dim3(kFsThreads), 0, st, d_V, N, (int64_t)(T + 1) * N, total);
    if (int rc = hip_ok(hipGetLastError(), "k_fs_zero launch")) return rc;
    // nodes per wave: the fewest workgroups that still give every CU several (a wave's nodes run one after the other)
    int npw = 8;
    while (npw > 1 && ((N + kFsWaves * npw - 1) / (kFsWaves * npw)) * n_problems < 1024) npw >>= 1;
    FsSolveArgs a;
    std::memset(&a, 0, sizeof a);
    a.tables = d_tables; a.prob = d_problems; a.g = g; a.T = T; a.npw = npw; a.V = d_V; a.arg = d_argmax;
    const dim3 gridDim((unsigned)((N + kFsWaves * npw - 1) / (kFsWaves * npw)), (unsigned)n_problems);
    for (int t = T - 1; t >= 0; --t) {
        a.t = t;
        hipLaunchKernelGGL(k_fs_backward, gridDim, dim3(kFsThreads), lds, st, a);
    }
    return hip_ok(hipGetLastError(), "k_fs_backward launch");
}

// Both window entry points: the checks, the kernel's LDS opt-in, the upload and the one launch.
static int fs_solve_window(const char *fn, bool forecast, const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                           shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid, int32_t T,
                           int32_t horizon, int32_t control, double *d_V, int64_t v_doubles, int32_t *d_argmax, void *stream)
{
    FsParams g;
    std::vector<shems_foresight_problem> recs;
    if (int rc = fs_check_solve(fn, d_tables, total_rows, problems, d_problems, n_problems, grid, T, d_V, g, recs, forecast)) return rc;
    if (horizon < 1) return set_error(SHEMS_ERR_ARG, "%s: horizon = %d; a plan sees at least the current hour", fn, (int)horizon);
    if (control < 1 || control > horizon)
        return set_error(SHEMS_ERR_ARG, "%s: control = %d; a fresh plan every 1 .. horizon = %d hours", fn, (int)control, (int)horizon);
    const int64_t N = (int64_t)g.nb * g.ne;
    if (2 * N * 8 > kFsMaxPlaneBytes)
        return set_error(SHEMS_ERR_ARG, "%s: the two V planes of %d x %d nodes a window keeps take %lld bytes of LDS; a workgroup has %d for them", fn,
                         (int)g.nb, (int)g.ne, (long long)(2 * N * 8), kFsMaxPlaneBytes);
    if (int rc = fs_check_v(fn, n_problems, T, N, v_doubles)) return rc;
    const int lds = (int)(2 * N * 8);
    static std::atomic<uint64_t> optin{0};                                  // per device, once (129 x 65 fails at launch without it)
    if (int rc = lds_optin(optin, (const void *)k_fs_window, kFsMaxPlaneBytes, "hipFuncSetAttribute(k_fs_window)")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = fs_upload(recs, d_problems, st)) return rc;
    FsWindowArgs a;
    std::memset(&a, 0, sizeof a);
    a.tables = d_tables; a.prob = d_problems; a.g = g; a.T = T; a.H = horizon; a.c = control; a.fc = forecast; a.V = d_V; a.arg = d_argmax;
    const dim3 gridDim((unsigned)fs_plan_windows(T, control), (unsigned)n_problems);
    hipLaunchKernelGGL(k_fs_window, gridDim, dim3(kFsWindowThreads), lds, st, a);
    return hip_ok(hipGetLastError(), "k_fs_window launch");
}

extern "C" int shems_foresight_solve_horizon_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                                                 shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid,
                                                 int32_t T, int32_t horizon, int32_t control, double *d_V, int64_t v_doubles,
                                                 int32_t *d_argmax, void *stream)
{
    return fs_solve_window("shems_foresight_solve_horizon_dev", false, d_tables, total_rows, problems, d_problems, n_problems, grid, T, horizon,
                           control, d_V, v_doubles, d_argmax, stream);
}

extern "C" int shems_foresight_solve_forecast_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *problems,
                                                  shems_foresight_problem *d_problems, int32_t n_problems, const shems_foresight_grid *grid,
                                                  int32_t T, int32_t horizon, int32_t control, double *d_V, int64_t v_doubles,
                                                  int32_t *d_argmax, void *stream)
{
    return fs_solve_window("shems_foresight_solve_forecast_dev", true, d_tables, total_rows, problems, d_problems, n_problems, grid, T, horizon,
                           control, d_V, v_doubles, d_argmax, stream);
}

// What the three forward entry points check before any HIP call, in the order the refusals are reported: the view, the grid, T, the
// buffers, then `check_v(N)` -- the caller's check of the V buffer against its record count (the ensemble's also holds its scenario count
// and weights, which have this place in the order) --, then results_env.  Fills `a`.
template <class CheckV>
static int fs_check_track(const char *fn, int fc, const shems_view *v, const shems_foresight_problem *d_problems, int32_t n_problems,
                          const int32_t *d_problem_of_env, const shems_foresight_grid *grid, int32_t T, const double *d_V, double *d_results,
                          int64_t results_env, double *d_returns, float *d_targets, FsTrackArgs &a, CheckV check_v)
{
    if (int rc = check_view(v, fn)) return rc;
    FsParams g;
    if (int rc = fs_params(grid, fn, g)) return rc;
    if (T < 1) return set_error(SHEMS_ERR_ARG, "%s: T = %d; the horizon must be at least 1 hour", fn, (int)T);
    if (!d_problems || n_problems < 1 || !d_V) return set_error(SHEMS_ERR_ARG, "%s: NULL buffer or no problem", fn);
    if (int rc = check_v((int64_t)g.nb * g.ne)) return rc;
    if (results_env >= v->n_envs) return set_error(SHEMS_ERR_ARG, "%s: results_env %lld outside the batch", fn, (long long)results_env);
    std::memset(&a, 0, sizeof a);
    a.v = *v; a.prob = d_problems; a.n_prob = n_problems; a.fc = fc; a.problem_of_env = d_problem_of_env; a.g = g; a.T = T; a.V = d_V;
    a.results = d_results; a.results_env = results_env; a.returns = d_returns; a.targets = d_targets;
    return SHEMS_OK;
}

static int fs_track(const char *fn, bool forecast, const shems_view *v, const shems_foresight_problem *d_problems, int32_t n_problems,
                    const int32_t *d_problem_of_env, const shems_foresight_grid *grid, int32_t T, const double *d_V, int64_t v_doubles,
                    double *d_results, int64_t results_env, double *d_returns, float *d_targets, void *stream)
{
    FsTrackArgs a;
    if (int rc = fs_check_track(fn, forecast, v, d_problems, n_problems, d_problem_of_env, grid, T, d_V, d_results, results_env, d_returns,
                                d_targets, a, [&](int64_t N) { return fs_check_v(fn, n_problems, T, N, v_doubles); }))
        return rc;
    hipLaunchKernelGGL(k_fs_track, dim3((unsigned)v->n_envs), dim3(kFsThreads), 0, (hipStream_t)stream, a);
    return hip_ok(hipGetLastError(), "k_fs_track launch");
}

extern "C" int shems_foresight_track_dev(const shems_view *v, const shems_foresight_problem *d_problems, int32_t n_problems,
                                         const int32_t *d_problem_of_env, const shems_foresight_grid *grid, int32_t T, const double *d_V,
                                         int64_t v_doubles, double *d_results, int64_t results_env, double *d_returns, float *d_targets, void *stream)
{
    return fs_track("shems_foresight_track_dev", false, v, d_problems, n_problems, d_problem_of_env, grid, T, d_V, v_doubles, d_results,
                    results_env, d_returns, d_targets, stream);
}

extern "C" int shems_foresight_track_forecast_dev(const shems_view *v, const shems_foresight_problem *d_problems, int32_t n_problems,
                                                  const int32_t *d_problem_of_env, const shems_foresight_grid *grid, int32_t T,
                                                  const double *d_V, int64_t v_doubles, double *d_results, int64_t results_env,
                                                  double *d_returns, float *d_targets, void *stream)
{
    return fs_track("shems_foresight_track_forecast_dev", true, v, d_problems, n_problems, d_problem_of_env, grid, T, d_V, v_doubles, d_results,
                    results_env, d_returns, d_targets, stream);
}

extern "C" int shems_foresight_track_ensemble_dev(const shems_view *v, const shems_foresight_problem *d_problems, int32_t n_problems,
                                                  int32_t n_scen, const double *weights, double *d_weights, const int32_t *d_problem_of_env,
                                                  const shems_foresight_grid *grid, int32_t T, const double *d_V, int64_t v_doubles,
                                                  double *d_results, int64_t results_env, double *d_returns, float *d_targets, void *stream)
{
    const char *fn = "shems_foresight_track_ensemble_dev";
    const int64_t recs = (int64_t)n_problems * n_scen;
    const auto check_ens = [&](int64_t N) {                                 // the ensemble's own checks
        if (n_scen < 1 || n_scen > kFsMaxScen)
            return set_error(SHEMS_ERR_ARG, "%s: n_scen = %d; an ensemble holds 1 .. %d scenarios", fn, (int)n_scen, kFsMaxScen);
        if (!weights || !d_weights) return set_error(SHEMS_ERR_ARG, "%s: NULL weight buffer (host weights or their device copy)", fn);
        for (int32_t p = 0; p < n_problems; ++p)
            for (int32_t k = 0; k < n_scen; ++k) {
                const double w = weights[(int64_t)p * n_scen + k];
                if (!(w > 0.0) || !(w <= 1.7976931348623157e308))            // also a NaN
                    return set_error(SHEMS_ERR_ARG, "%s: problem %d, scenario %d: weight %g; a weight is finite and > 0", fn, (int)p, (int)k, w);
            }
        if (v_doubles < recs * (T + 1) * N)
            return set_error(SHEMS_ERR_ARG, "%s: the V buffer holds %lld float64; %d problems x %d scenarios x %d planes x %lld nodes need %lld", fn,
                             (long long)v_doubles, (int)n_problems, (int)n_scen, (int)T + 1, (long long)N, (long long)(recs * (T + 1) * N));
        return (int)SHEMS_OK;
    };
    FsTrackEnsArgs a;
    std::memset(&a, 0, sizeof a);
    if (int rc = fs_check_track(fn, 1, v, d_problems, n_problems, d_problem_of_env, grid, T, d_V, d_results, results_env, d_returns, d_targets,
                                a.t, check_ens))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // the weights the kernel reads: ordered on the stream; the runtime has staged a pageable source on return
    if (int rc = hip_ok(hipMemcpyAsync(d_weights, weights, (size_t)recs * sizeof(double), hipMemcpyHostToDevice, st), "upload of the scenario weights"))
        return rc;
    a.K = n_scen; a.w = d_weights;
    hipLaunchKernelGGL(k_fs_track_ens, dim3((unsigned)v->n_envs), dim3(kFsThreads), 0, st, a);
    return hip_ok(hipGetLastError(), "k_fs_track_ens launch");
}

extern "C" int shems_foresight_audit_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *d_problems, int32_t n_problems,
                                         const shems_foresight_grid *grid, int32_t T, const double *d_V, int64_t v_doubles,
                                         const double *d_results, int32_t n_pass, const int32_t *d_problem_of_pass, double *d_out,
                                         int32_t *d_best_action, int32_t *d_status, void *stream)
{
    const char *fn = "shems_foresight_audit_dev";
    FsParams g;
    if (int rc = fs_params(grid, fn, g)) return rc;
    if (T < 1) return set_error(SHEMS_ERR_ARG, "%s: T = %d; a pass is at least 1 hour", fn, (int)T);
    if (!d_tables || total_rows < 2 || !d_problems || n_problems < 1 || !d_V)
        return set_error(SHEMS_ERR_ARG, "%s: NULL buffer, fewer than 2 table rows, or no problem", fn);
    if (n_pass < 1 || n_pass > 65535) return set_error(SHEMS_ERR_ARG, "%s: n_pass = %d; one call audits 1 .. 65535 passes", fn, (int)n_pass);
    if (!d_results || !d_out || !d_best_action || !d_status)
        return set_error(SHEMS_ERR_ARG, "%s: NULL results, out, best_action or status buffer", fn);
    if (int rc = fs_check_v(fn, n_problems, T, (int64_t)g.nb * g.ne, v_doubles)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = hip_ok(hipMemsetAsync(d_status, 0, (size_t)n_pass * sizeof(int32_t), st), "hipMemsetAsync(status)")) return rc;
    FsAuditArgs a;
    std::memset(&a, 0, sizeof a);
    a.tables = d_tables; a.total_rows = total_rows; a.prob = d_problems; a.n_prob = n_problems; a.problem_of_pass = d_problem_of_pass;
    a.g = g; a.T = T; a.V = d_V; a.results = d_results; a.out = d_out; a.best_action = d_best_action; a.status = d_status;
    hipLaunchKernelGGL(k_fs_audit, dim3((unsigned)((T + kFsWaves - 1) / kFsWaves), (unsigned)n_pass), dim3(kFsThreads), 0, st, a);
    return hip_ok(hipGetLastError(), "k_fs_audit launch");
}

extern "C" int shems_foresight_demos_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *d_problems, int32_t n_problems,
                                         const shems_foresight_grid *grid, int32_t T, const double *d_results, int32_t n_pass,
                                         const int32_t *d_problem_of_pass, const float *d_targets, const int32_t *d_best_action,
                                         const shems_replay *ring, int64_t pos, int32_t *d_status, void *stream)
{
    const char *fn = "shems_foresight_demos_dev";
    FsParams g;
    if (int rc = fs_params(grid, fn, g)) return rc;
    if (T < 1) return set_error(SHEMS_ERR_ARG, "%s: T = %d; a pass is at least 1 hour", fn, (int)T);
    if (!d_tables || total_rows < 2 || !d_problems || n_problems < 1)
        return set_error(SHEMS_ERR_ARG, "%s: NULL buffer, fewer than 2 table rows, or no problem", fn);
    if (n_pass < 1 || n_pass > 65535) return set_error(SHEMS_ERR_ARG, "%s: n_pass = %d; one call converts 1 .. 65535 passes", fn, (int)n_pass);
    if (!d_results || !d_status) return set_error(SHEMS_ERR_ARG, "%s: NULL results or status buffer", fn);
    if ((d_targets != nullptr) == (d_best_action != nullptr))
        return set_error(SHEMS_ERR_ARG, "%s: exactly one label source: %s", fn, d_targets ? "both d_targets and d_best_action are given" : "neither d_targets nor d_best_action is given");
    if (!ring || !ring->s || !ring->a) return set_error(SHEMS_ERR_ARG, "%s: NULL ring, or a ring without s or a", fn);
    switch (fs_demo_check_ring(ring->capacity, pos, n_pass, T)) {
    case 1: return set_error(SHEMS_ERR_ARG, "%s: the ring's capacity is %lld", fn, (long long)ring->capacity);
    case 2: return set_error(SHEMS_ERR_ARG, "%s: %d passes x %d hours are %lld pairs; the ring's capacity is %lld", fn, (int)n_pass, (int)T,
                             (long long)n_pass * T, (long long)ring->capacity);
    case 3: return set_error(SHEMS_ERR_ARG, "%s: pos = %lld lies outside the ring of %lld slots", fn, (long long)pos, (long long)ring->capacity);
    default: break;
    }
    hipStream_t st = (hipStream_t)stream;
    if (int rc = hip_ok(hipMemsetAsync(d_status, 0, (size_t)n_pass * sizeof(int32_t), st), "hipMemsetAsync(status)")) return rc;
    FsDemosArgs a;
    std::memset(&a, 0, sizeof a);
    a.tables = d_tables; a.total_rows = total_rows; a.prob = d_problems; a.n_prob = n_problems; a.problem_of_pass = d_problem_of_pass;
    a.g = g; a.T = T; a.results = d_results; a.targets = d_targets; a.best_action = d_best_action; a.s = ring->s; a.a = ring->a;
    a.capacity = ring->capacity; a.pos = pos; a.status = d_status;
    hipLaunchKernelGGL(k_fs_demos, dim3((unsigned)((T + kFsThreads - 1) / kFsThreads), (unsigned)n_pass), dim3(kFsThreads), 0, st, a);
    return hip_ok(hipGetLastError(), "k_fs_demos launch");
}

extern "C" int shems_foresight_transitions_dev(const float *d_tables, int64_t total_rows, const shems_foresight_problem *d_problems,
                                               int32_t n_problems, int32_t T, const double *d_results, int32_t n_pass,
                                               const int32_t *d_problem_of_pass, int32_t mode, float gamma, int32_t tail, double *d_returns,
                                               const shems_replay *ring, int64_t pos, int32_t *d_status, void *stream)
{
    const char *fn = "shems_foresight_transitions_dev";
    if (T < 2) return set_error(SHEMS_ERR_ARG, "%s: T = %d; a transition needs a successor hour, so a pass is at least 2 hours", fn, (int)T);
    if (tail < 1 || tail >= T) return set_error(SHEMS_ERR_ARG, "%s: tail = %d lies outside 1 .. T - 1 = %d", fn, (int)tail, (int)T - 1);
    if (mode != SHEMS_FS_TRANS_TD && mode != SHEMS_FS_TRANS_MC) return set_error(SHEMS_ERR_ARG, "%s: mode = %d is neither TD (0) nor MC (1)", fn, (int)mode);
    if (mode == SHEMS_FS_TRANS_MC && !d_returns) return set_error(SHEMS_ERR_ARG, "%s: MC mode needs d_returns", fn);
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return set_error(SHEMS_ERR_ARG, "%s: gamma = %g lies outside [0, 1]", fn, (double)gamma);
    if (!d_tables || total_rows < 2 || !d_problems || n_problems < 1)
        return set_error(SHEMS_ERR_ARG, "%s: NULL buffer, fewer than 2 table rows, or no problem", fn);
    if (n_pass < 1 || n_pass > 65535) return set_error(SHEMS_ERR_ARG, "%s: n_pass = %d; one call converts 1 .. 65535 passes", fn, (int)n_pass);
    if (!d_results || !d_status) return set_error(SHEMS_ERR_ARG, "%s: NULL results or status buffer", fn);
    if (!ring || !ring->s || !ring->a || !ring->r || !ring->s2 || !ring->done)
        return set_error(SHEMS_ERR_ARG, "%s: NULL ring, or a ring without all of s, a, r, s2 and done", fn);
    const int keep = T - tail;
    switch (fs_demo_check_ring(ring->capacity, pos, n_pass, keep)) {
    case 1: return set_error(SHEMS_ERR_ARG, "%s: the ring's capacity is %lld", fn, (long long)ring->capacity);
    case 2: return set_error(SHEMS_ERR_ARG, "%s: %d passes x %d hours are %lld transitions; the ring's capacity is %lld", fn, (int)n_pass, keep,
                             (long long)n_pass * keep, (long long)ring->capacity);
    case 3: return set_error(SHEMS_ERR_ARG, "%s: pos = %lld lies outside the ring of %lld slots", fn, (long long)pos, (long long)ring->capacity);
    default: break;
    }
    hipStream_t st = (hipStream_t)stream;
    if (int rc = hip_ok(hipMemsetAsync(d_status, 0, (size_t)n_pass * sizeof(int32_t), st), "hipMemsetAsync(status)")) return rc;
    FsTransArgs a;
    std::memset(&a, 0, sizeof a);
    a.tables = d_tables; a.total_rows = total_rows; a.prob = d_problems; a.n_prob = n_problems; a.problem_of_pass = d_problem_of_pass;
    a.T = T; a.tail = tail; a.mode = mode; a.gamma = gamma; a.results = d_results; a.returns = d_returns;
    a.s = ring->s; a.a = ring->a; a.r = ring->r; a.s2 = ring->s2; a.done = ring->done;
    a.capacity = ring->capacity; a.pos = pos; a.status = d_status;
    if (d_returns) {
        hipLaunchKernelGGL(k_fs_returns, dim3((unsigned)n_pass), dim3(64), 0, st, a);
        if (int rc = hip_ok(hipGetLastError(), "k_fs_returns launch")) return rc;
    }
    hipLaunchKernelGGL(k_fs_transitions, dim3((unsigned)((keep + kFsThreads - 1) / kFsThreads), (unsigned)n_pass), dim3(kFsThreads), 0, st, a);
    return hip_ok(hipGetLastError(), "k_fs_transitions launch");
}

// shems_nstep.hip -- multi-step (n-step) returns: the kernels that build an n-step replay ring on the GPU (include/shems_hip.h,
// DESIGN.md 4r; the arithmetic and the slot rules are csrc/shems_nstep_core.h's).  Built with -ffp-contract=off.
//
//   k_nstep_fold           behind every fused vector step of an n-step learner: the step has written the one-step transitions of the
//                          stationary window [0, window) into a staging ring; the fold stores hour h's (s, a, r) in history slot
//                          h mod n and, from hour n - 1 on, emits (s_{h-n+1}, a_{h-n+1}, G, s'_h, done_h) into the ring.  grid y =
//                          learner (a learner group: every block at + l * stride_bytes).
//   k_nstep_from_episodes  populate_memory: whole episodes of one-step transitions (what shems_rollout_dev leaves in a scratch ring)
//                          converted in one launch.
// Both are small streams: threads map flat over the window x 9 (x 2, x 1) elements, so loads and stores are contiguous apart from
// the ring's wrap; no LDS, no atomics.  Each thread reads history slot (h + 1) mod n and writes slot h mod n of its own element
// only, so no thread reads what another writes (n = 1, where the two slots coincide, reads the staging values instead).
#include "shems_internal.h"
#include "shems_nstep_core.h"

namespace shems {

constexpr int kNstepBlock = 256;

template <class T>
__device__ __forceinline__ T *at_learner(T *p, int64_t l, int64_t stride_bytes)
{
    return (T *)((char *)p + l * stride_bytes);
}

__global__ __launch_bounds__(kNstepBlock) void k_nstep_fold(shems_nstep ns, shems_replay stage, shems_replay ring, int64_t stride_bytes,
                                                            const float *__restrict__ d_gamma1, int64_t ring_pos, int32_t hour)
{
    const int64_t l = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kNstepBlock + threadIdx.x;
    const int64_t W = ns.window;
    const int n = ns.n;
    if (i >= W * kNstepState) return;
    const int slot = nstep_slot(hour, n), old = nstep_oldest(hour, n);
    const bool emit = nstep_emits(hour, n);
    float *hist_s = at_learner(ns.hist_s, l, stride_bytes), *hist_a = at_learner(ns.hist_a, l, stride_bytes),
          *hist_r = at_learner(ns.hist_r, l, stride_bytes);
    {                                                   // s and s2: element i = household i / 9, component i % 9
        const float *st_s = at_learner(stage.s, l, stride_bytes), *st_s2 = at_learner(stage.s2, l, stride_bytes);
        const float cur = st_s[i];
        if (emit) {
            const int64_t j = i / kNstepState, c = i - j * kNstepState;
            const int64_t d = nstep_dest(ring_pos, j, ring.capacity);
            at_learner(ring.s, l, stride_bytes)[d * kNstepState + c] = n == 1 ? cur : hist_s[(int64_t)old * W * kNstepState + i];
            at_learner(ring.s2, l, stride_bytes)[d * kNstepState + c] = st_s2[i];
        }
        hist_s[(int64_t)slot * W * kNstepState + i] = cur;
    }
    if (i < W * kNstepAction) {
        const float cur = at_learner(stage.a, l, stride_bytes)[i];
        if (emit) {
            const int64_t j = i / kNstepAction, c = i - j * kNstepAction;
            const int64_t d = nstep_dest(ring_pos, j, ring.capacity);
            at_learner(ring.a, l, stride_bytes)[d * kNstepAction + c] = n == 1 ? cur : hist_a[(int64_t)old * W * kNstepAction + i];
        }
        hist_a[(int64_t)slot * W * kNstepAction + i] = cur;
    }
    if (i < W) {
        const float cur = at_learner(stage.r, l, stride_bytes)[i];
        if (emit) {
            const float g1 = d_gamma1 ? d_gamma1[l] : ns.gamma;
            const int64_t d = nstep_dest(ring_pos, i, ring.capacity);
            at_learner(ring.r, l, stride_bytes)[d] = nstep_return(n, g1, [&](int k) {
                return k == n - 1 ? cur : hist_r[(int64_t)((old + k) % n) * W + i];
            });
            at_learner(ring.done, l, stride_bytes)[d] = at_learner(stage.done, l, stride_bytes)[i];
        }
        hist_r[(int64_t)slot * W + i] = cur;
    }
}

__global__ __launch_bounds__(kNstepBlock) void k_nstep_from_episodes(shems_replay src, int64_t m, int64_t steps, int n, float gamma, int64_t total,
                                                                     shems_replay ring, int64_t ring_pos)
{
    const int64_t i = (int64_t)blockIdx.x * kNstepBlock + threadIdx.x;
    if (i >= total * kNstepState) return;
    {
        const int64_t q = i / kNstepState, c = i - q * kNstepState;
        if (nstep_bulk_kept(q, total, ring.capacity)) {
            const int64_t e = q / m, a0 = e * steps + (q - e * m), d = nstep_dest(ring_pos, q, ring.capacity);
            ring.s[d * kNstepState + c] = src.s[a0 * kNstepState + c];
            ring.s2[d * kNstepState + c] = src.s2[(a0 + n - 1) * kNstepState + c];
        }
    }
    if (i < total * kNstepAction) {
        const int64_t q = i / kNstepAction, c = i - q * kNstepAction;
        if (nstep_bulk_kept(q, total, ring.capacity)) {
            const int64_t e = q / m, a0 = e * steps + (q - e * m), d = nstep_dest(ring_pos, q, ring.capacity);
            ring.a[d * kNstepAction + c] = src.a[a0 * kNstepAction + c];
        }
    }
    if (i < total && nstep_bulk_kept(i, total, ring.capacity)) {
        const int64_t e = i / m, a0 = e * steps + (i - e * m), d = nstep_dest(ring_pos, i, ring.capacity);
        ring.r[d] = nstep_return(n, gamma, [&](int k) { return src.r[a0 + k]; });
        ring.done[d] = src.done[a0 + n - 1];
    }
}

static bool ring_complete(const shems_replay *r) { return r && r->capacity > 0 && r->s && r->a && r->r && r->s2 && r->done; }

static int fold_check(const char *fn, const shems_nstep *ns, const shems_replay *stage, const shems_replay *ring, int64_t ring_pos, int32_t hour)
{
    if (!ns) return set_error(SHEMS_ERR_ARG, "%s: ns is NULL", fn);
    if (ns->n < 1 || ns->n > SHEMS_NSTEP_MAX) return set_error(SHEMS_ERR_ARG, "%s: n = %d outside 1 .. %d", fn, (int)ns->n, (int)SHEMS_NSTEP_MAX);
    if (ns->window < 1 || ns->window > (int64_t)1 << 24)
        return set_error(SHEMS_ERR_ARG, "%s: window = %lld outside 1 .. 2^24", fn, (long long)ns->window);
    if (!ns->hist_s || !ns->hist_a || !ns->hist_r) return set_error(SHEMS_ERR_ARG, "%s: history arrays missing", fn);
    if (hour < 0) return set_error(SHEMS_ERR_ARG, "%s: hour = %d is negative", fn, (int)hour);
    if (!ring_complete(stage)) return set_error(SHEMS_ERR_ARG, "%s: incomplete staging ring", fn);
    if (!ring_complete(ring)) return set_error(SHEMS_ERR_ARG, "%s: incomplete replay ring", fn);
    if (stage->capacity < ns->window)
        return set_error(SHEMS_ERR_ARG, "%s: staging capacity %lld below the window %lld", fn, (long long)stage->capacity, (long long)ns->window);
    if (ring->capacity < ns->window)
        return set_error(SHEMS_ERR_ARG, "%s: ring capacity %lld below the window %lld", fn, (long long)ring->capacity, (long long)ns->window);
    if (ring_pos < 0) return set_error(SHEMS_ERR_ARG, "%s: ring_pos = %lld is negative", fn, (long long)ring_pos);
    return SHEMS_OK;
}

static int fold_launch(const shems_nstep *ns, const shems_replay *stage, const shems_replay *ring, int count, int64_t stride_bytes,
                       const float *d_gamma1, int64_t ring_pos, int32_t hour, void *stream)
{
    const int64_t elems = ns->window * kNstepState;
    const dim3 grid((unsigned)((elems + kNstepBlock - 1) / kNstepBlock), (unsigned)count);
    hipLaunchKernelGGL(k_nstep_fold, grid, dim3(kNstepBlock), 0, (hipStream_t)stream, *ns, *stage, *ring, stride_bytes, d_gamma1,
                       ring_pos % ring->capacity, hour);
    return hip_ok(hipGetLastError(), "k_nstep_fold launch");
}

}  // namespace shems

using namespace shems;

extern "C" {

int shems_nstep_fold_dev(const shems_nstep *ns, const shems_replay *stage, const shems_replay *ring, int64_t ring_pos, int32_t hour,
                         void *stream)
{
    if (int rc = fold_check("shems_nstep_fold_dev", ns, stage, ring, ring_pos, hour)) return rc;
    return fold_launch(ns, stage, ring, 1, 0, nullptr, ring_pos, hour, stream);
}

int shems_nstep_group_fold_dev(const shems_nstep *ns0, const shems_replay *stage0, const shems_replay *ring0, const shems_group *g,
                               const float *d_gamma1, int64_t ring_pos, int32_t hour, void *stream)
{
    if (int rc = fold_check("shems_nstep_group_fold_dev", ns0, stage0, ring0, ring_pos, hour)) return rc;
    if (!g || g->count < 1 || g->count > 65535 || g->stride_bytes < 0 || g->stride_bytes % 4 != 0)
        return set_error(SHEMS_ERR_ARG, "shems_nstep_group_fold_dev: bad group (count 1 .. 65535, stride_bytes a non-negative multiple of 4)");
    return fold_launch(ns0, stage0, ring0, g->count, g->stride_bytes, d_gamma1, ring_pos, hour, stream);
}

int shems_nstep_from_episodes_dev(const shems_replay *src, int64_t episodes, int64_t steps, int32_t n, float gamma, const shems_replay *ring,
                                  int64_t ring_pos, void *stream)
{
    const char *fn = "shems_nstep_from_episodes_dev";
    if (n < 1 || n > SHEMS_NSTEP_MAX) return set_error(SHEMS_ERR_ARG, "%s: n = %d outside 1 .. %d", fn, (int)n, (int)SHEMS_NSTEP_MAX);
    if (steps < n) return set_error(SHEMS_ERR_ARG, "%s: steps = %lld below n = %d", fn, (long long)steps, (int)n);
    if (episodes < 1 || steps > (int64_t)1 << 24 || episodes > (int64_t)1 << 24)
        return set_error(SHEMS_ERR_ARG, "%s: episodes = %lld, steps = %lld outside 1 .. 2^24", fn, (long long)episodes, (long long)steps);
    if (!ring_complete(src)) return set_error(SHEMS_ERR_ARG, "%s: incomplete source ring", fn);
    if (!ring_complete(ring)) return set_error(SHEMS_ERR_ARG, "%s: incomplete replay ring", fn);
    if (src->capacity < episodes * steps)
        return set_error(SHEMS_ERR_ARG, "%s: source capacity %lld below episodes * steps = %lld", fn, (long long)src->capacity,
                         (long long)(episodes * steps));
    if (ring_pos < 0) return set_error(SHEMS_ERR_ARG, "%s: ring_pos = %lld is negative", fn, (long long)ring_pos);
    if (src->s == ring->s || src->r == ring->r) return set_error(SHEMS_ERR_ARG, "%s: source and destination are the same ring", fn);
    const int64_t m = nstep_bulk_m(steps, n), total = episodes * m;
    const int64_t blocks = (total * kNstepState + kNstepBlock - 1) / kNstepBlock;
    if (blocks > 0x7FFFFFFF) return set_error(SHEMS_ERR_ARG, "%s: %lld transitions exceed one launch", fn, (long long)total);
    hipLaunchKernelGGL(k_nstep_from_episodes, dim3((unsigned)blocks), dim3(kNstepBlock), 0, (hipStream_t)stream, *src, m, steps, (int)n, gamma,
                       total, *ring, ring_pos % ring->capacity);
    return hip_ok(hipGetLastError(), "k_nstep_from_episodes launch");
}

}  // extern "C"

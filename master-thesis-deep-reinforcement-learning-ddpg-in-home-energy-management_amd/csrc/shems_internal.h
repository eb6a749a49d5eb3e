// shems_internal.h -- shared by the translation units of libshems_hip.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstdint>
#include "../../include/shems_hip.h"
#include "shems_per_core.h"

namespace shems {
int set_error(int code, const char *fmt, ...);          // records the thread-local message, returns code
int hip_ok(hipError_t e, const char *what);             // SHEMS_OK or SHEMS_ERR_HIP (+ message)
// Kernels with more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize, and the attribute is PER DEVICE: a
// C-ABI caller may drive several GPUs from one process (shems_create(..., device, ...)), so the opt-in is remembered per
// (kernel, current device) -- `mask` is the kernel's own static bit set, bit = device ordinal.
inline int lds_optin(std::atomic<uint64_t> &mask, const void *fn, int bytes, const char *what)
{
    int dev = 0;
    if (int rc = hip_ok(hipGetDevice(&dev), "hipGetDevice")) return rc;
    const uint64_t bit = 1ull << (dev & 63);
    if (mask.load(std::memory_order_acquire) & bit) return SHEMS_OK;
    if (int rc = hip_ok(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), what)) return rc;
    mask.fetch_or(bit, std::memory_order_release);
    return SHEMS_OK;
}
// Floats of shems_ddpg.ws every caller allocates (shems_ddpg_workspace_floats): the latency form's carve (shems_ddpg.hip) defines it, the
// throughput form of the grouped update (shems_gupd.hip) carves its own, smaller, layout out of the same block.
constexpr int64_t kTpWsFloats = 1902568;
int check_view(const shems_view *v, const char *fn);    // every entry point that dereferences a caller-built view (shems_env.hip)
// Single learners on the tiled working layout (shems_ddpg_tiled_enter, shems_ddpg.hip).  w2t_lookup: is `block` one of such a learner's
// eight Flux-order blocks (parameters, targets, moments)?  Its regions go to *out (may be null).  w2t_flux_guard: SHEMS_ERR_STATE if
// so -- what every entry point that reads or writes such a block in Flux order calls before it launches anything.
bool w2t_lookup(const float *block, shems_group_w2t *out);
int w2t_flux_guard(const float *block, const char *fn);
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
// What every entry point that takes a prioritized ring (shems_per_core.h) refuses for the ring's own arguments: a single learner's
// (shems_ddpg.hip) or learner 0's of a group (shems_gupd.hip).  batch null: the batches are per-learner records on the device.
inline int check_per(const shems_per *per, int64_t capacity, int64_t ring_len, int64_t fresh_pos, int64_t fresh_count, const int32_t *batch,
                     const char *fn)
{
    if (!per || !per->prio || !per->pmax || !per->ws) return set_error(SHEMS_ERR_ARG, "%s: shems_per has a NULL buffer", fn);
    if (capacity < 1 || capacity > kPerMaxSlots)
        return set_error(SHEMS_ERR_ARG, "%s: a prioritized ring holds 1..%lld slots (got %lld)", fn, (long long)kPerMaxSlots, (long long)capacity);
    if (ring_len < 1 || ring_len > capacity) return set_error(SHEMS_ERR_ARG, "%s: ring_len must be in 1..capacity", fn);
    if (batch && (*batch < 1 || *batch > kPerCols)) return set_error(SHEMS_ERR_ARG, "%s: batch must be in 1..128 (got %d)", fn, *batch);
    if (((uintptr_t)per->prio & 15) != 0 || ((uintptr_t)per->ws & 15) != 0 || ((uintptr_t)per->pmax & 3) != 0)
        return set_error(SHEMS_ERR_ARG, "%s: prio and the workspace must be 16-byte aligned, pmax 4-byte aligned", fn);
    const size_t np = (size_t)capacity * 4, nw = (size_t)per_ws_floats(capacity) * 4;
    if (ranges_overlap(per->prio, np, per->ws, nw) || ranges_overlap(per->prio, np, per->pmax, 4) || ranges_overlap(per->ws, nw, per->pmax, 4))
        return set_error(SHEMS_ERR_ARG, "%s: prio, pmax and the workspace overlap", fn);
    for (const float v : {per->alpha, per->beta, per->eps_p})
        if (!(v >= 0.0f) || !std::isfinite(v)) return set_error(SHEMS_ERR_ARG, "%s: alpha, beta and eps_p must be finite and >= 0", fn);
    if (per->beta > 1.0f) return set_error(SHEMS_ERR_ARG, "%s: beta must be in [0, 1] (got %g)", fn, (double)per->beta);
    if (fresh_pos < 0 || fresh_pos >= capacity || fresh_count < 0)
        return set_error(SHEMS_ERR_ARG, "%s: the fresh range must start inside the ring and have a count >= 0", fn);
    if (fresh_count > 0 && fresh_count < capacity && ring_len < capacity && fresh_pos + fresh_count > ring_len)
        return set_error(SHEMS_ERR_ARG, "%s: the fresh range [%lld, +%lld) leaves the %lld filled slots", fn, (long long)fresh_pos,
                         (long long)fresh_count, (long long)ring_len);
    return SHEMS_OK;
}
// ADAM (Flux 0.12.1) + soft target update over n consecutive parameters, the data-parallel path's sweep (shems_ddpg.hip: k_adam_soft)
// on any parameter count: the wide-network path (shems_wide.hip) applies its gradients with it.
int adam_soft_sweep(float *p, const float *g, float *m, float *v, float *target, float *publish, int n, double eta, double bp1, double bp2,
                    double gscale, float tau, hipStream_t st);
// The same sweep for `count` learners of a group (learner l: every block + l * gstride_bytes) in one launch, grad_scale 1, no publish
// copy.  hp: learner l's eta and tau from hp[l] (k1 formed on the device); null: eta / tau for every learner.
int adam_soft_sweep_group(float *p, const float *g, float *m, float *v, float *target, int n, double eta, double bp1, double bp2, float tau,
                          int count, int64_t gstride_bytes, const shems_group_hparams *hp, bool critic, hipStream_t st);
// shems_wide.hip: forward pass of an actor (9 -> l1 -> l2 -> 2) of any hidden sizes for m observations, up to the output layer's partial
// sums: d_part [*n_partials][m][2] (b3 not included; the caller adds b3 and the partials in index order).  d_ws holds
// wide_act_ws_floats(l1, l2, m) floats of scratch (normalised observations, layer 1, then -- at wide_act_part_offset -- the partials).
int wide_actor_pre(const float *actor, const float *s_min, const float *s_max, int l1, int l2, const float *d_obs, int64_t m, float *d_ws,
                   float *d_part, int *n_partials, hipStream_t st);
int64_t wide_act_ws_floats(int l1, int l2, int64_t m);
// The same for a learner group (shems_wide_act_step_group_dev): env i = l * epl + r runs learner l's actor and normalisation (learner 0's
// + l * stride floats); d_part holds learner l's partials at [l][*n_partials][epl][2].  The workspace is wide_act_ws_floats(l1, l2, count * epl).
int wide_actor_pre_group(const float *actor0, const float *s_min0, const float *s_max0, int64_t stride, int count, int64_t epl, int l1, int l2,
                         const float *d_obs, float *d_ws, float *d_part, int *n_partials, hipStream_t st);
int64_t wide_act_part_offset(int l1, int64_t m);
}

// shems_nstep_core.h -- multi-step (n-step) returns: the arithmetic and the slot rules of the n-step ring, written once (host + device
// functions).  The reference has no such transitions; the definition is this one (include/shems_hip.h).
//
// An n-step ring holds (s_t, a_t, G_t, s_{t+n}, done_{t+n-1}) with G_t = sum_{k<n} gamma^k r_{t+k}; the update kernels read it as any
// ring and receive gamma_n = gamma^n in their `gamma` field.  Full windows only: an episode of T hours gives the T - n + 1 transitions
// that start at hours 0 .. T - n, and a window never spans a reset.
//   return:    Horner's rule in float64 over the ring's own Float32 rewards, newest first:
//                  acc = (double) r_{t+n-1};   for k = n-2 .. 0: acc = (double) r_{t+k} + (double) gamma32 * acc;   G = (float) acc
//              the product rounds on its own, then the sum (no fma: the pragma below and -ffp-contract=off).
//   discount:  gamma_n = (float)(g * g * ... * g), n factors g = (double) gamma32 multiplied left to right on the HOST (nstep_gamma);
//              the device never forms a power.
//   history:   hour h of an episode is kept in slot h mod n of hist_s / hist_a / hist_r [n][window][9 | 2 | 1]; from hour n - 1 on the
//              fold emits the transition that starts at hour h - n + 1, whose (s, a) lie in slot (h + 1) mod n (for n = 1 that is the
//              hour's own slot: the staging values themselves).  Hours 0 .. n - 2 of an episode emit nothing, so whatever an earlier
//              episode left in the history is overwritten before it can be read.
//   slots:     household j of the window goes to ring slot (ring_pos + j) mod capacity.  Bulk form: with m = steps - n + 1,
//              transition (e, t), t < m, has push order e * m + t and goes to slot (ring_pos + order) mod capacity; orders below
//              episodes * m - capacity would be overwritten by a later push of the same call and are skipped.
// Checked bit for bit against the NumPy twin (tests/nstep_ref.py) by a host build (tests/hostcheck/nstep_hostcheck.cpp, g++
// -ffp-contract=off).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define NSTEP_HD __host__ __device__ __forceinline__
#else
#define NSTEP_HD inline
#endif

namespace shems {

constexpr int kNstepMax = 16;              // SHEMS_NSTEP_MAX
constexpr int kNstepState = 9, kNstepAction = 2;

NSTEP_HD int nstep_slot(int32_t hour, int n) { return (int)(hour % n); }                 // where hour h's (s, a, r) are kept
NSTEP_HD int nstep_oldest(int32_t hour, int n) { return (int)((hour + 1) % n); }         // where hour h - n + 1's are
NSTEP_HD bool nstep_emits(int32_t hour, int n) { return hour >= n - 1; }
NSTEP_HD int64_t nstep_dest(int64_t ring_pos, int64_t j, int64_t capacity) { return (ring_pos + j) % capacity; }
NSTEP_HD int64_t nstep_bulk_m(int64_t steps, int n) { return steps - n + 1; }            // transitions per episode
NSTEP_HD bool nstep_bulk_kept(int64_t order, int64_t total, int64_t capacity) { return order >= total - capacity; }

// G of one window: r_at(k) returns r_{t+k} (a float), k = 0 .. n - 1.
template <class At>
NSTEP_HD float nstep_return(int n, float gamma32, At r_at)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double g = (double)gamma32;
    double acc = (double)r_at(n - 1);
    for (int k = n - 2; k >= 0; --k) {
        const double p = g * acc;
        acc = (double)r_at(k) + p;
    }
    return (float)acc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// gamma_n, host only.
inline float nstep_gamma(float gamma32, int n)
{
    const double g = (double)gamma32;
    double p = g;
    for (int i = 1; i < n; ++i) p = p * g;
    return (float)p;
}

// ---- the fold and the bulk conversion on host arrays (the hostcheck's; any CPU caller's) ----
struct NstepRingHost { int64_t capacity; float *s, *a, *r, *s2; uint8_t *done; };

// One vector step: the staging arrays hold hour `hour`'s one-step transitions of households [0, window).  Returns the pushes made.
inline int64_t nstep_fold_host(int n, int64_t window, float gamma32, float *hist_s, float *hist_a, float *hist_r, const NstepRingHost &stage,
                               const NstepRingHost &ring, int64_t ring_pos, int32_t hour)
{
    const int slot = nstep_slot(hour, n), old = nstep_oldest(hour, n);
    const bool emit = nstep_emits(hour, n);
    for (int64_t j = 0; j < window; ++j) {
        const int64_t d = nstep_dest(ring_pos, j, ring.capacity);
        if (emit) {
            for (int c = 0; c < kNstepState; ++c) {
                ring.s[d * kNstepState + c] = n == 1 ? stage.s[j * kNstepState + c] : hist_s[((int64_t)old * window + j) * kNstepState + c];
                ring.s2[d * kNstepState + c] = stage.s2[j * kNstepState + c];
            }
            for (int c = 0; c < kNstepAction; ++c)
                ring.a[d * kNstepAction + c] = n == 1 ? stage.a[j * kNstepAction + c] : hist_a[((int64_t)old * window + j) * kNstepAction + c];
            ring.r[d] = nstep_return(n, gamma32, [&](int k) {
                return k == n - 1 ? stage.r[j] : hist_r[(int64_t)((old + k) % n) * window + j];
            });
            ring.done[d] = stage.done[j];
        }
        for (int c = 0; c < kNstepState; ++c) hist_s[((int64_t)slot * window + j) * kNstepState + c] = stage.s[j * kNstepState + c];
        for (int c = 0; c < kNstepAction; ++c) hist_a[((int64_t)slot * window + j) * kNstepAction + c] = stage.a[j * kNstepAction + c];
        hist_r[(int64_t)slot * window + j] = stage.r[j];
    }
    return emit ? window : 0;
}

// src holds episode e's hour t at slot e * steps + t.  Returns the pushes (skipped ones included: the push counter's advance).
inline int64_t nstep_from_episodes_host(const NstepRingHost &src, int64_t episodes, int64_t steps, int n, float gamma32, const NstepRingHost &ring,
                                        int64_t ring_pos)
{
    const int64_t m = nstep_bulk_m(steps, n), total = episodes * m;
    for (int64_t q = 0; q < total; ++q) {
        if (!nstep_bulk_kept(q, total, ring.capacity)) continue;
        const int64_t e = q / m, t = q % m, a0 = e * steps + t, a1 = a0 + n - 1, d = nstep_dest(ring_pos, q, ring.capacity);
        for (int c = 0; c < kNstepState; ++c) {
            ring.s[d * kNstepState + c] = src.s[a0 * kNstepState + c];
            ring.s2[d * kNstepState + c] = src.s2[a1 * kNstepState + c];
        }
        for (int c = 0; c < kNstepAction; ++c) ring.a[d * kNstepAction + c] = src.a[a0 * kNstepAction + c];
        ring.r[d] = nstep_return(n, gamma32, [&](int k) { return src.r[a0 + k]; });
        ring.done[d] = src.done[a1];
    }
    return total;
}
#endif

}  // namespace shems

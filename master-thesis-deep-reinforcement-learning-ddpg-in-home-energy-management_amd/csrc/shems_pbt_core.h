// shems_pbt_core.h -- population-based training of a learner group (Jaderberg et al. 2017): the order, the quota, the parent draw and the
// explore arithmetic of one round, written once (host + device functions).  The definition is include/shems_hip.h's and DESIGN.md 4s.
//
//   order:    a is better than b if a's score is finite and b's is not, or both are finite and score_a > score_b; equal scores, or two
//             non-finite ones: the lower learner index is better.  rank[l] = learners of l's population that are better than l.
//   quota:    q = (P * permille) / 1000 in integers, P the population's size, permille in 1 .. 500, so 2 q <= P: the parents (rank < q)
//             and the children (rank >= P - q) are disjoint, and no record or slab is read and written in one round.
//   exploit:  child l draws ONE Philox4x32-10 block, counter (l, round, 0, kStreamPbt), key (seed lo, seed hi); its parent is the learner
//             of rank j = (uint64(x) * q) >> 32 of its population.  A parent whose score is not finite: the child keeps itself.
//   explore:  the child's record is the parent's whole record; then for every field enabled in `fields` (eta_act, eta_crit, tau,
//             noise_sigma = bits 0 .. 3) bit k of the block's word y picks the factor f = up (set) or down (clear):
//                 eta' = (double)(float)(eta * f)            x' = (float)((double) x * f)            then clamp to [lo[k], hi[k]].
//             The bounds are Float32 values (pbt_params_check), so the clamp is exact in either format.
// Checked bit for bit against the NumPy twin (tests/pbt_ref.py) by a host build (tests/hostcheck/pbt_hostcheck.cpp, g++
// -ffp-contract=off).
#pragma once

#include <stdint.h>

#include "../../include/shems_hip.h"
#include "philox.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PBT_HD __host__ __device__ __forceinline__
#else
#define PBT_HD inline
#endif

namespace shems {

constexpr int kPbtFields = 4;              // SHEMS_PBT_FIELDS: eta_act, eta_crit, tau, noise_sigma
constexpr int kPbtMaxRanges = 8;           // SHEMS_PBT_MAX_RANGES
constexpr int kPbtMaxCount = 4096;         // SHEMS_PBT_MAX_COUNT: the counting loops are O(count^2) per child

PBT_HD bool pbt_finite(double s) { return __builtin_fabs(s) <= 1.7976931348623157e308; }      // false for NaN and +-inf

PBT_HD bool pbt_better(double sa, int a, double sb, int b)
{
    const bool fa = pbt_finite(sa), fb = pbt_finite(sb);
    if (fa != fb) return fa;
    if (fa && sa != sb) return sa > sb;
    return a < b;
}

PBT_HD int pbt_quota(int P, int permille) { return (int)(((int64_t)P * permille) / 1000); }

// rank of learner l inside its population, and the population's size
PBT_HD int pbt_rank(int count, const int32_t *pop, const double *score, int l, int *P_out)
{
    const int32_t mine = pop[l];
    const double s = score[l];
    int rank = 0, P = 0;
    for (int m = 0; m < count; ++m) {
        if (pop[m] != mine) continue;
        ++P;
        if (m != l && pbt_better(score[m], m, s, l)) ++rank;
    }
    *P_out = P;
    return rank;
}

PBT_HD double pbt_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

PBT_HD double pbt_explore_eta(double eta, double f, double lo, double hi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return pbt_clamp((double)(float)(eta * f), lo, hi);
}

PBT_HD float pbt_explore_f32(float x, double f, double lo, double hi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (float)pbt_clamp((double)(float)((double)x * f), lo, hi);
}

// One learner of one round.  Returns parent[l] (l itself: kept, *rec untouched) and rank[l]; for a child, *rec receives its new record.
// hp is read at the parent's index only, and a parent is never a child: the caller may store *rec into hp[l] at once.
PBT_HD int pbt_select_one(const shems_pbt_params &p, int count, const int32_t *pop, const double *score, const shems_group_hparams *hp,
                          int l, int *rank_out, shems_group_hparams *rec)
{
    int P = 0;
    const int rank = pbt_rank(count, pop, score, l, &P);
    *rank_out = rank;
    const int q = pbt_quota(P, p.permille);
    if (q == 0 || rank < P - q) return l;
    const u32x4 r = philox4x32_10((uint32_t)l, p.round, 0u, (uint32_t)kStreamPbt, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const int j = (int)(((uint64_t)r.x * (uint64_t)q) >> 32);
    int parent = -1;
    for (int m = 0; m < count && parent < 0; ++m) {
        if (pop[m] != pop[l]) continue;
        int Pm;
        if (pbt_rank(count, pop, score, m, &Pm) == j) parent = m;
    }
    if (parent < 0 || parent == l || !pbt_finite(score[parent])) return l;
    shems_group_hparams h = hp[parent];
    const uint32_t y = r.y;
    if (p.fields & 1u) h.eta_act = pbt_explore_eta(h.eta_act, (y & 1u) ? p.up : p.down, p.lo[0], p.hi[0]);
    if (p.fields & 2u) h.eta_crit = pbt_explore_eta(h.eta_crit, (y & 2u) ? p.up : p.down, p.lo[1], p.hi[1]);
    if (p.fields & 4u) h.tau = pbt_explore_f32(h.tau, (y & 4u) ? p.up : p.down, p.lo[2], p.hi[2]);
    if (p.fields & 8u) h.noise_sigma = pbt_explore_f32(h.noise_sigma, (y & 8u) ? p.up : p.down, p.lo[3], p.hi[3]);
    *rec = h;
    return parent;
}

// ---- host only ----
// The host check of the parameters: 0, or the number of the first bad item with *what naming it (shems_pbt_params_check's message).
// A bound is refused if a value clamped to it could fail shems_group_hparams_check: eta not finite or <= 0, tau outside (0, 1],
// sigma < 0; and if it is not a Float32 value (the clamp must be exact in the record's own format).
inline int pbt_params_check(const shems_pbt_params &p, const char **what)
{
    static const char *const names[kPbtFields] = {"eta_act", "eta_crit", "tau", "noise_sigma"};
    static thread_local char buf[96];
    auto f32 = [](double v) { return (double)(float)v == v; };
    if (p.permille < 1 || p.permille > 500) { *what = "permille outside 1 .. 500"; return 1; }
    if (p.fields & ~15u) { *what = "fields holds unknown bits (eta_act, eta_crit, tau, noise_sigma are bits 0 .. 3)"; return 2; }
    if (p.reserved != 0) { *what = "reserved must be 0"; return 3; }
    if (!pbt_finite(p.down) || !(p.down > 0.0)) { *what = "down must be finite and > 0"; return 4; }
    if (!pbt_finite(p.up) || !(p.up > 0.0)) { *what = "up must be finite and > 0"; return 5; }
    for (int k = 0; k < kPbtFields; ++k) {
        const double lo = p.lo[k], hi = p.hi[k];
        const char *why = nullptr;
        if (!pbt_finite(lo) || !pbt_finite(hi)) why = "bounds must be finite";
        else if (!(lo <= hi)) why = "lo above hi";
        else if (!f32(lo) || !f32(hi)) why = "bounds must be Float32 values";
        else if (k < 2 && !(lo > 0.0)) why = "lo must be > 0 (ADAM's eta)";
        else if (k == 2 && !(lo > 0.0 && hi <= 1.0)) why = "bounds must lie in (0, 1]";
        else if (k == 3 && !(lo >= 0.0)) why = "lo must be >= 0";
        if (why) {
            int n = 0;
            for (const char *s = names[k]; *s && n < 30; ++s) buf[n++] = *s;
            buf[n++] = ':'; buf[n++] = ' ';
            for (const char *s = why; *s && n < 94; ++s) buf[n++] = *s;
            buf[n] = 0;
            *what = buf;
            return 6 + k;
        }
    }
    return 0;
}

// One whole round on host arrays, in place (the hostcheck's; any CPU caller's).
inline void pbt_round_host(const shems_pbt_params &p, int count, const int32_t *pop, const double *score, shems_group_hparams *hp,
                           int32_t *parent, int32_t *rank)
{
    for (int l = 0; l < count; ++l) {
        shems_group_hparams rec;
        int r = 0;
        const int par = pbt_select_one(p, count, pop, score, hp, l, &r, &rec);
        parent[l] = par;
        rank[l] = r;
        if (par != l) hp[l] = rec;
    }
}

}  // namespace shems

// shems_pbt.hip -- population-based training of a learner group: the two launches of one round (include/shems_hip.h; the
// order, the draw and the explore arithmetic are csrc/shems_pbt_core.h's).  Built with -ffp-contract=off.
//
//   k_pbt_select   one thread per learner: its rank inside its population by a counting loop over the group, and for a child the
//                  parent draw and the new record, written in place.  Parents and children are disjoint, so the only record a thread
//                  reads besides its own scores is one nobody writes.  A few hundred threads: the launch is latency, not throughput.
//   k_pbt_copy     the round's stream: every child's slab ranges from its parent's.  grid = (chunks, learner); a workgroup moves
//                  kPbtChunkVecs 16-byte vectors -- kPbtVecs per thread, all loads issued before the first store -- with non-temporal
//                  loads and stores (each byte is touched once; the update kernels that follow should find their own lines in L2, not
//                  this stream's).  A kept learner's workgroups leave on a wave-uniform branch.  No LDS, no atomics.
#include "shems_internal.h"
#include "shems_pbt_core.h"

namespace shems {

constexpr int kPbtBlock = 256;
constexpr int kPbtVecs = 8;                                    // vectors in flight per thread
constexpr int kPbtChunkVecs = kPbtBlock * kPbtVecs;            // SHEMS_PBT_CHUNK_VECS
static_assert(kPbtChunkVecs == SHEMS_PBT_CHUNK_VECS, "the header's chunk size");
static_assert(kPbtMaxRanges == SHEMS_PBT_MAX_RANGES && kPbtFields == SHEMS_PBT_FIELDS && kPbtMaxCount == SHEMS_PBT_MAX_COUNT, "the header's limits");

typedef float pbt_f4 __attribute__((ext_vector_type(4)));

struct PbtRanges {                                             // by value: the ranges in 16-byte vectors
    int64_t off[kPbtMaxRanges];                                // first vector of range k inside a slab
    int64_t len[kPbtMaxRanges];                                // its vectors
    int32_t cend[kPbtMaxRanges];                               // chunks of ranges 0 .. k: a chunk never straddles two ranges
    int32_t n;
};

__global__ __launch_bounds__(kPbtBlock) void k_pbt_select(shems_pbt_params p, int count, const int32_t *__restrict__ pop,
                                                          const double *__restrict__ score, shems_group_hparams *hp,
                                                          int32_t *__restrict__ parent, int32_t *__restrict__ rank)
{
    const int l = (int)(blockIdx.x * kPbtBlock + threadIdx.x);
    if (l >= count) return;
    shems_group_hparams rec;
    int r = 0;
    const int par = pbt_select_one(p, count, pop, score, hp, l, &r, &rec);
    parent[l] = par;
    rank[l] = r;
    if (par != l) hp[l] = rec;
}

__global__ __launch_bounds__(kPbtBlock) void k_pbt_copy(float *slab0, int64_t stride_vecs, int count, PbtRanges rg,
                                                        const int32_t *__restrict__ parent)
{
    const int l = (int)blockIdx.y;
    const int par = parent[l];
    if (par == l || par < 0 || par >= count) return;           // kept (or a bad entry): uniform over the workgroup
    if (parent[par] != par) return;                            // a parent that is itself written this launch is never read
    const pbt_f4 *src = (const pbt_f4 *)slab0 + (int64_t)par * stride_vecs;
    pbt_f4 *dst = (pbt_f4 *)slab0 + (int64_t)l * stride_vecs;
    int64_t off = 0, len = 0;                                  // the chunk's range: a scalar walk, the same for every lane
    int c = (int)blockIdx.x, cbegin = 0;
#pragma unroll
    for (int r = kPbtMaxRanges - 1; r >= 0; --r)
        if (r < rg.n && c < rg.cend[r]) { off = rg.off[r]; len = rg.len[r]; cbegin = r ? rg.cend[r - 1] : 0; }
    const int64_t base = (int64_t)(c - cbegin) * kPbtChunkVecs;            // the chunk's first vector inside its range (scalar)
    const int here = (int)(len - base < kPbtChunkVecs ? len - base : kPbtChunkVecs);
    const pbt_f4 *s = src + off + base;
    pbt_f4 *d = dst + off + base;
    const int i = (int)threadIdx.x;
    pbt_f4 x[kPbtVecs];
    if (here == kPbtChunkVecs) {                                // a full chunk: no lane tests
#pragma unroll
        for (int k = 0; k < kPbtVecs; ++k) x[k] = __builtin_nontemporal_load(s + i + k * kPbtBlock);
#pragma unroll
        for (int k = 0; k < kPbtVecs; ++k) __builtin_nontemporal_store(x[k], d + i + k * kPbtBlock);
    } else {                                                    // a range's tail
#pragma unroll
        for (int k = 0; k < kPbtVecs; ++k)
            if (i + k * kPbtBlock < here) __builtin_nontemporal_store(__builtin_nontemporal_load(s + i + k * kPbtBlock), d + i + k * kPbtBlock);
    }
}

}  // namespace shems

using namespace shems;

extern "C" {

int shems_pbt_params_check(const shems_pbt_params *params)
{
    if (!params) return set_error(SHEMS_ERR_ARG, "shems_pbt_params_check: params is NULL");
    const char *what = nullptr;
    if (pbt_params_check(*params, &what)) return set_error(SHEMS_ERR_ARG, "shems_pbt_params_check: %s", what);
    return SHEMS_OK;
}

int shems_pbt_select_dev(const shems_pbt_params *params, int32_t count, const int32_t *d_pop, const double *d_score,
                         shems_group_hparams *d_hp, int32_t *d_parent, int32_t *d_rank, void *stream)
{
    const char *fn = "shems_pbt_select_dev";
    if (!params || !d_pop || !d_score || !d_hp || !d_parent || !d_rank)
        return set_error(SHEMS_ERR_ARG, "%s: NULL argument (params, d_pop, d_score, d_hp, d_parent and d_rank are all needed)", fn);
    if (count < 1 || count > SHEMS_PBT_MAX_COUNT)
        return set_error(SHEMS_ERR_ARG, "%s: count = %d outside 1 .. %d", fn, (int)count, (int)SHEMS_PBT_MAX_COUNT);
    const char *what = nullptr;
    if (pbt_params_check(*params, &what)) return set_error(SHEMS_ERR_ARG, "%s: %s", fn, what);
    if ((uintptr_t)d_hp % 8 != 0 || (uintptr_t)d_score % 8 != 0)
        return set_error(SHEMS_ERR_ARG, "%s: alignment: d_hp and d_score must be 8-byte aligned", fn);
    if ((uintptr_t)d_pop % 4 != 0 || (uintptr_t)d_parent % 4 != 0 || (uintptr_t)d_rank % 4 != 0)
        return set_error(SHEMS_ERR_ARG, "%s: alignment: d_pop, d_parent and d_rank must be 4-byte aligned", fn);
    const unsigned blocks = (unsigned)((count + kPbtBlock - 1) / kPbtBlock);
    hipLaunchKernelGGL(k_pbt_select, dim3(blocks), dim3(kPbtBlock), 0, (hipStream_t)stream, *params, (int)count, d_pop, d_score, d_hp, d_parent,
                       d_rank);
    return hip_ok(hipGetLastError(), "k_pbt_select launch");
}

int shems_pbt_copy_dev(float *slab0, const shems_group *g, const shems_pbt_range *ranges, int32_t n_ranges, const int32_t *d_parent,
                       void *stream)
{
    const char *fn = "shems_pbt_copy_dev";
    if (!slab0 || !g || !ranges || !d_parent) return set_error(SHEMS_ERR_ARG, "%s: NULL argument (slab0, g, ranges and d_parent are all needed)", fn);
    if (g->count < 1 || g->count > 65535) return set_error(SHEMS_ERR_ARG, "%s: count = %d outside 1 .. 65535", fn, (int)g->count);
    if (g->stride_bytes < 16 || g->stride_bytes % 16 != 0)
        return set_error(SHEMS_ERR_ARG, "%s: stride_bytes = %lld is not a positive multiple of 16", fn, (long long)g->stride_bytes);
    if ((uintptr_t)slab0 % 16 != 0 || (uintptr_t)d_parent % 4 != 0)
        return set_error(SHEMS_ERR_ARG, "%s: alignment: slab0 must be 16-byte aligned, d_parent 4-byte aligned", fn);
    if (n_ranges < 1 || n_ranges > SHEMS_PBT_MAX_RANGES)
        return set_error(SHEMS_ERR_ARG, "%s: n_ranges = %d outside 1 .. %d", fn, (int)n_ranges, (int)SHEMS_PBT_MAX_RANGES);
    PbtRanges rg = {};
    rg.n = n_ranges;
    int64_t total = 0, chunks = 0;
    const int64_t stride_floats = g->stride_bytes / 4;
    for (int k = 0; k < n_ranges; ++k) {
        const int64_t o = ranges[k].offset_floats, n = ranges[k].floats;
        if (o < 0 || n < 0) return set_error(SHEMS_ERR_ARG, "%s: range %d: negative offset or length (%lld, %lld)", fn, k, (long long)o, (long long)n);
        if (o % 4 != 0 || n % 4 != 0)
            return set_error(SHEMS_ERR_ARG, "%s: range %d: alignment: (%lld, %lld) are not both multiples of 4 floats", fn, k, (long long)o,
                             (long long)n);
        if (o > stride_floats || n > stride_floats - o)
            return set_error(SHEMS_ERR_ARG, "%s: range %d: (%lld, %lld) runs past stride_bytes = %lld", fn, k, (long long)o, (long long)n,
                             (long long)g->stride_bytes);
        total += n / 4;
        chunks += (n / 4 + kPbtChunkVecs - 1) / kPbtChunkVecs;
        if (chunks > 0x7FFFFFFF) return set_error(SHEMS_ERR_ARG, "%s: the ranges exceed one launch", fn);
        rg.off[k] = o / 4;
        rg.len[k] = n / 4;
        rg.cend[k] = (int32_t)chunks;
    }
    if (total == 0) return set_error(SHEMS_ERR_ARG, "%s: every range is empty", fn);
    hipLaunchKernelGGL(k_pbt_copy, dim3((unsigned)chunks, (unsigned)g->count), dim3(kPbtBlock), 0, (hipStream_t)stream, slab0, g->stride_bytes / 16,
                       (int)g->count, rg, d_parent);
    return hip_ok(hipGetLastError(), "k_pbt_copy launch");
}

}  // extern "C"

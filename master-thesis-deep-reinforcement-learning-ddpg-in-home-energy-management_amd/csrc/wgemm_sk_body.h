// wgemm_sk_body.h -- the body of k_wgemm_sk and k_wgemm_sk_g (csrc/shems_wide.hip), included inside each kernel so that every kernel compiles
// this text as its own (a body shared through an inlined function changed the existing kernel's register allocation).  In scope: `G`,
// the product's GemmArgs.
    if ((int64_t)blockIdx.x * 32 >= G.M || (int64_t)blockIdx.y * 32 >= G.N) return;      // (the grid is the largest problem's)
    __shared__ float As[2][SK][SLD], Bs[2][SK][SLD];
    __shared__ float red[4][16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * 32, n0 = (int64_t)blockIdx.y * 32;
    const bool a_kfast = G.sak == 1, b_jfast = G.sbj == 1;
    int ai[SR], ak[SR], bj[SR], bk[SR];
#pragma unroll
    for (int r = 0; r < SR; ++r) {
        const int e = tid + 256 * r;
        ai[r] = a_kfast ? e >> SKB : e & 31;  ak[r] = a_kfast ? e & (SK - 1) : e >> 5;
        bj[r] = b_jfast ? e & 31 : e >> SKB;  bk[r] = b_jfast ? e >> 5 : e & (SK - 1);
    }
    // global loads run GP stages ahead in a ring of register slots; every load is unconditional, from a clamped (always valid) address,
    // and the zero of an out-of-range element is selected when the slot is stashed (a load under a lane predicate is sunk into a branch
    // behind s_waitcnt vmcnt(0), which serialises the ring).  One barrier per stage: stash(s) -> barrier -> MFMAs(s); buffer s & 1 was
    // last read in stage s - 2, which every thread left before anyone passed barrier s - 1.
    constexpr int GP = 2;
    float ra[GP][SR], rb[GP][SR];
    unsigned oka[GP], okb[GP];
    auto fetch = [&](int k0, float (&xa)[SR], float (&xb)[SR], unsigned &ma, unsigned &mb) {
        ma = mb = 0u;
#pragma unroll
        for (int r = 0; r < SR; ++r) {
            const int64_t i = m0 + ai[r], j = n0 + bj[r];
            const int ka = k0 + ak[r], kb = k0 + bk[r];
            ma |= (i < G.M && ka < G.K) ? 1u << r : 0u;
            mb |= (j < G.N && kb < G.K) ? 1u << r : 0u;
            xa[r] = G.A[min(i, (int64_t)G.M - 1) * G.sai + min(ka, G.K - 1) * G.sak];
            xb[r] = G.B[min(kb, G.K - 1) * G.sbk + min(j, (int64_t)G.N - 1) * G.sbj];
        }
    };
    auto stash = [&](int buf, const float (&xa)[SR], const float (&xb)[SR], unsigned ma, unsigned mb) {
#pragma unroll
        for (int r = 0; r < SR; ++r) {
            As[buf][ak[r]][ai[r]] = (ma >> r & 1u) ? xa[r] : 0.0f;
            Bs[buf][bk[r]][bj[r]] = (mb >> r & 1u) ? xb[r] : 0.0f;
        }
    };
    wf32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nst = (G.K + SK - 1) / SK;
#pragma unroll
    for (int u = 0; u < GP; ++u) fetch(u * SK, ra[u], rb[u], oka[u], okb[u]);
    for (int s0 = 0; s0 < nst; s0 += GP) {
#pragma unroll
        for (int u = 0; u < GP; ++u) {
            const int s = s0 + u;
            if (s < nst) {
                const int buf = s & 1;
                stash(buf, ra[u], rb[u], oka[u], okb[u]);
                __syncthreads();
                if (s + GP < nst) fetch((s + GP) * SK, ra[u], rb[u], oka[u], okb[u]);
#pragma unroll
                for (int kk = 0; kk < SK / 4; kk += 2)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][wave * (SK / 4) + kk + lh][li], Bs[buf][wave * (SK / 4) + kk + lh][li], acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r * 64 + lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q, r = e >> 6, l2 = e & 63;
        const int64_t i = m0 + (r & 3) + 8 * (r >> 2) + 4 * (l2 >> 5), j = n0 + (l2 & 31);
        if (i < G.M && j < G.N) {
            float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
            if (G.bias) v += G.bias[j];
            if (G.relu) v = fmaxf(v, 0.0f);
            if (G.gate) v = G.gate[i * G.ldg + j] > 0.0f ? v : 0.0f;
            G.C[i * G.ldc + j] = v;
        }
    }

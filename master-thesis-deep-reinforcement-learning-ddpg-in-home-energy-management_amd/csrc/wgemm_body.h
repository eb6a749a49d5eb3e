// wgemm_body.h -- the body of k_wgemm and k_wgemm_g (csrc/shems_wide.hip), included inside each kernel so that every kernel compiles
// this text as its own (a body shared through an inlined function changed the existing kernel's register allocation).  In scope: `G`,
// the product's GemmArgs.
    __shared__ float As[2][GK][GLD], Bs[2][GK][GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.x * GT, n0 = (int64_t)blockIdx.y * GT;
    const bool a_kfast = G.sak == 1, b_jfast = G.sbj == 1;
    // element e = tid + 256 r of a 64 x GK operand tile: (row, k) with the memory-contiguous index fastest across threads
    int ai[GR], ak[GR], bj[GR], bk[GR];
#pragma unroll
    for (int r = 0; r < GR; ++r) {
        const int e = tid + 256 * r;
        ai[r] = a_kfast ? e >> GKB : e & 63;  ak[r] = a_kfast ? e & (GK - 1) : e >> 6;
        bj[r] = b_jfast ? e & 63 : e >> GKB;  bk[r] = b_jfast ? e >> 6 : e & (GK - 1);
    }
    // the global loads of stage s + 1 are in flight while stage s is multiplied; double-buffered LDS, one barrier per stage.  (With
    // thousands of workgroups the latency is hidden by occupancy: a deeper register ring and unpredicated clamped loads, which pay off
    // in the small-M kernel below, measured slower here -- 480-490 against 443 us for the vector step of 65 536 envs.)
    float ra[GR], rb[GR];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            const int64_t i = m0 + ai[r], j = n0 + bj[r];
            const int ka = k0 + ak[r], kb = k0 + bk[r];
            ra[r] = (i < G.M && ka < G.K) ? G.A[i * G.sai + ka * G.sak] : 0.0f;
            rb[r] = (j < G.N && kb < G.K) ? G.B[kb * G.sbk + j * G.sbj] : 0.0f;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int r = 0; r < GR; ++r) { As[buf][ak[r]][ai[r]] = ra[r]; Bs[buf][bk[r]][bj[r]] = rb[r]; }
    };
    wf32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    fetch(0);
    stash(0);
    __syncthreads();
    const int nst = (G.K + GK - 1) / GK;
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        if (s + 1 < nst) fetch((s + 1) * GK);
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][kk + lh][wi * 32 + li], Bs[buf][kk + lh][wj * 32 + li], acc, 0, 0, 0);
        if (s + 1 < nst) stash(buf ^ 1);
        __syncthreads();
    }
    const int64_t j = n0 + wj * 32 + li;
    if (j < G.N) {
        const float bj_ = G.bias ? G.bias[j] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t i = m0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (i < G.M) {
                float v = acc[r] + bj_;
                if (G.relu) v = fmaxf(v, 0.0f);
                if (G.gate) v = G.gate[i * G.ldg + j] > 0.0f ? v : 0.0f;
                G.C[i * G.ldc + j] = v;
            }
        }
    }

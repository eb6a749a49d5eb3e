// wgemm128_body.h -- the body of k_wgemm128 and k_wgemm128_g (csrc/shems_wide.hip), included inside each kernel so that every kernel compiles
// this text as its own (a body shared through an inlined function changed the existing kernel's register allocation).  In scope: `G`,
// the product's GemmArgs; HEAD and V4, the template arguments.
    __shared__ __attribute__((aligned(16))) float As[2][GK][BLD], Bs[2][GK][BLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.x * BT, n0 = (int64_t)blockIdx.y * BT;
    const bool a_kfast = G.sak == 1, b_jfast = G.sbj == 1;
    int ai[BR], ak[BR], bj[BR], bk[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) {
        const int e = tid + 256 * r;
        ai[r] = a_kfast ? e >> GKB : e & (BT - 1);  ak[r] = a_kfast ? e & (GK - 1) : e >> 7;
        bj[r] = b_jfast ? e & (BT - 1) : e >> GKB;  bk[r] = b_jfast ? e >> 7 : e & (GK - 1);
    }
    float ra[BR], rb[BR];
    wf32x4 va[2], vb[2];
    auto fetch = [&](int k0) {
        if constexpr (V4) {
            // quad f = tid + 256 r: A row f >> 2, k = 4 (f & 3) ..; B row k = f >> 5, j = 4 (f & 31) ..
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int f = tid + 256 * r;
                const int64_t i = m0 + (f >> 2), j = n0 + 4 * (f & 31);
                const int ka = k0 + 4 * (f & 3), kb = k0 + (f >> 5);
                const wf32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                va[r] = (i < G.M && ka < G.K) ? *reinterpret_cast<const wf32x4 *>(G.A + i * G.sai + ka) : z;
                vb[r] = (j < G.N && kb < G.K) ? *reinterpret_cast<const wf32x4 *>(G.B + kb * G.sbk + j) : z;
            }
        } else {
#pragma unroll
            for (int r = 0; r < BR; ++r) {
                const int64_t i = m0 + ai[r], j = n0 + bj[r];
                const int ka = k0 + ak[r], kb = k0 + bk[r];
                ra[r] = (i < G.M && ka < G.K) ? G.A[i * G.sai + ka * G.sak] : 0.0f;
                rb[r] = (j < G.N && kb < G.K) ? G.B[kb * G.sbk + j * G.sbj] : 0.0f;
            }
        }
    };
    auto stash = [&](int buf) {
        if constexpr (V4) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int f = tid + 256 * r;
#pragma unroll
                for (int c = 0; c < 4; ++c) As[buf][4 * (f & 3) + c][f >> 2] = va[r][c];
                *reinterpret_cast<wf32x4 *>(&Bs[buf][f >> 5][4 * (f & 31)]) = vb[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < BR; ++r) { As[buf][ak[r]][ai[r]] = ra[r]; Bs[buf][bk[r]][bj[r]] = rb[r]; }
        }
    };
    wf32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
    fetch(0);
    stash(0);
    __syncthreads();
    const int nst = (G.K + GK - 1) / GK;
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        if (s + 1 < nst) fetch((s + 1) * GK);
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            const float a0 = As[buf][kk + lh][wi * 64 + li], a1 = As[buf][kk + lh][wi * 64 + 32 + li];
            const float b0 = Bs[buf][kk + lh][wj * 64 + li], b1 = Bs[buf][kk + lh][wj * 64 + 32 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (s + 1 < nst) stash(buf ^ 1);
        __syncthreads();
    }
    if constexpr (!HEAD) {
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int64_t j = n0 + wj * 64 + y * 32 + li;
            if (j >= G.N) continue;
            const float bj_ = G.bias ? G.bias[j] : 0.0f;
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t i = m0 + wi * 64 + x * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (i < G.M) {
                        float v = acc[x][y][r] + bj_;
                        if (G.relu) v = fmaxf(v, 0.0f);
                        if (G.gate) v = G.gate[i * G.ldg + j] > 0.0f ? v : 0.0f;
                        G.C[i * G.ldc + j] = v;
                    }
                }
        }
    } else {
        // this lane's two columns: bias and the head's weights (zero beyond N, so padded columns add nothing)
        float bb[2], w3[2][2];
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int64_t j = n0 + wj * 64 + y * 32 + li;
            const bool in = j < G.N;
            const int64_t jc = in ? j : 0;
            bb[y] = in && G.bias ? G.bias[jc] : 0.0f;
#pragma unroll
            for (int o = 0; o < 2; ++o) w3[y][o] = in && o < G.head_n ? G.head_w[jc * G.head_n + o] : 0.0f;
        }
        float *out = G.head_out + ((int64_t)blockIdx.y * 2 + wj) * G.M * G.head_n;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v0 = fmaxf(acc[x][0][r] + bb[0], 0.0f), v1 = fmaxf(acc[x][1][r] + bb[1], 0.0f);
                float s0 = v0 * w3[0][0] + v1 * w3[1][0], s1 = v0 * w3[0][1] + v1 * w3[1][1];
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }     // over the half's 32 lanes
                const int64_t i = m0 + wi * 64 + x * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (li == 0 && i < G.M) {
                    out[i * G.head_n] = s0;
                    if (G.head_n > 1) out[i * G.head_n + 1] = s1;
                }
            }
    }

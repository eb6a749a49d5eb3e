// fs_window_body.h -- the body of k_fs_window and k_fs_window_fc (csrc/shems_foresight.hip), included into each kernel after
//   constexpr bool FC = ...;
// and not shared through an inlined template: shared that way, k_fs_window kept its registers but not its instructions, and an
// existing kernel keeps its code (the precedent: DESIGN.md 4d).  `A` is the kernel's FsWindowArgs.
// FC: the plan's belief (shems_foresight_core.h): the two rows of a sweep no longer sit next to each other in memory, so lanes 0-7 of
// wave 0 load the current row and lanes 8-15 the next, each from its own wave-uniform base formed inside the sweep.
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
            if (FC) {
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
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(best_v, off, 64);
                const int oa = __shfl_xor(best_a, off, 64);
                if (fs_better(ov, oa, best_v, best_a)) { best_v = ov; best_a = oa; }
            }
            if (lane == 0) {
                Vt[node] = best_v;
                if (v_out) Vp[(int64_t)t * N + node] = best_v;
                if (a_out) argp[(int64_t)t * N + node] = best_a;
            }
        }
    }

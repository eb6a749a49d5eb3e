// fs_track_body.h -- the body of k_fs_track and k_fs_track_fc (csrc/shems_foresight.hip), included into each kernel after
//   constexpr bool FC = ...;
// and not shared through an inlined template: shared that way, k_fs_track's scalar-register allocation moved (53 instead of 59 spilled
// SGPRs), and an existing kernel keeps its code.  `A` is the kernel's FsTrackArgs.
// FC: the controller does not know row t + 1 yet: h_countdown / soc_ev of the next row come from the forecast table, which must lie
// inside the row array (checked here, against the view's total_rows: the records may come from a solve on another array).
    __shared__ float s_obs[SHEMS_NSTATE];
    __shared__ double s_bv[kFsWaves];
    __shared__ int s_ba[kFsWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    if (FC && ((int64_t)P.cfg.table_row0 + P.forecast_off < 0 || (int64_t)P.cfg.table_row0 + P.forecast_off + P.cfg.nrow > v.total_rows)) {
        if (tid == 0) raise(v.err, SHEMS_ERR_INDEX);
        return;
    }
    const shems_config cfg = load_cfg(v, e);                                // the env's own config steps the env
    float obs[SHEMS_NSTATE];
#pragma unroll
    for (int k = 0; k < SHEMS_NSTATE; ++k) obs[k] = v.obs[e * SHEMS_NSTATE + k];
    if (tid < SHEMS_NSTATE) s_obs[tid] = v.obs[e * SHEMS_NSTATE + tid];
    __syncthreads();
    double total = 0.0;
    for (int t = 0; t < A.T; ++t) {
        if (idx < 1 || idx + 1 > cfg.nrow || idx + 1 > P.cfg.nrow) {       // row idx + 1 does not exist (Julia: BoundsError)
            if (tid == 0) raise(v.err, SHEMS_ERR_INDEX);
            break;
        }
        const double *Vn = A.V + ((int64_t)p * (A.T + 1) + t + 1) * N;
        const float h_cur = load_h(v.tables, P.cfg.table_row0, idx);
        const int64_t next0 = (int64_t)P.cfg.table_row0 + (FC ? fs_belief_off(t + 1, t, P.forecast_off) : 0);
        const float h_next = load_h(v.tables, next0, idx + 1);
        const float soc_ev_next = v.tables[(next0 + idx) * SHEMS_NCOL + 1];
        const EnvIn s{s_obs[0], s_obs[1], s_obs[2], s_obs[3], s_obs[4], s_obs[5]};
        double best_v = -__builtin_inf();
        int best_a = kFsNoAction;
        for (int a = tid; a < NA; a += kFsThreads) {
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
        if (lane == 0) { s_bv[wave] = best_v; s_ba[wave] = best_a; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < kFsWaves; ++w)
                if (fs_better(s_bv[w], s_ba[w], best_v, best_a)) { best_v = s_bv[w]; best_a = s_ba[w]; }
            const int a = best_a == kFsNoAction ? 0 : best_a;               // every Q a NaN: cannot happen on finite tables
            const int ab = a / g.nae, ae = a - ab * g.nae;
            const float a0 = fs_target(ab, g.nab), a1 = fs_target(ae, g.nae);
            float pre[SHEMS_NSTATE];
#pragma unroll
            for (int k = 0; k < SHEMS_NSTATE; ++k) pre[k] = obs[k];
            double reward;
            StepFlows f;
            float B, EV, Bt, EVt;
            env_advance(cfg, v.tables, obs, idx, step, a0, a1, SHEMS_TRACK_DRL, reward, f, B, EV, Bt, EVt);   // bounds checked above
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
            for (int k = 0; k < SHEMS_NSTATE; ++k) s_obs[k] = obs[k];
        } else {
            idx += 1;                                                        // every thread follows the row index
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < SHEMS_NSTATE; ++k) v.obs[e * SHEMS_NSTATE + k] = obs[k];
        v.idx[e] = idx;
        v.step[e] = step;
        if (A.returns) A.returns[e] = total;
    }

// foresight_forecast_hostcheck.cpp -- TEST TOOL, not a product path.  A stand-alone program (g++ -ffp-contract=off) that sweeps one
// problem under the belief of csrc/shems_foresight_core.h -- the plan made at hour j reads the true rows up to j and the forecast
// table's after it, every row offset taken from fs_belief_off -- with a serial loop that does with fs_q what k_fs_window does on
// the GPU, and prints what shems_foresight_solve_forecast_dev would leave, so that a GPU-less container can compare it with the NumPy
// twin on the composite tables.  The GPU tests (-m gpu) remain the authoritative check.
//
//   foresight_forecast_hostcheck INPUT H c
// INPUT (binary, written by the test): int32 total_rows, nb, ne, nab, nae, T; the 72 bytes of one shems_foresight_problem (cfg, idx0,
// forecast_off, scale_b, hb as foresight.make_problems fills them); float32 rows [total_rows][8].
// Output: one line "V t node bits" (the float64 as 16 hex digits) per stored plane entry, one line "A t node index" per arg-max.
#include <cinttypes>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_foresight_core.h"

using namespace shems;

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s INPUT H c\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[6];
    shems_foresight_problem P;
    static_assert(sizeof(shems_foresight_problem) == 72 && offsetof(shems_foresight_problem, forecast_off) == 52, "the record of include/shems_hip.h");
    if (std::fread(head, sizeof head, 1, f) != 1 || std::fread(&P, sizeof P, 1, f) != 1) { std::fprintf(stderr, "short input\n"); return 2; }
    const int64_t total_rows = head[0];
    const int T = head[5], H = std::atoi(argv[2]), c = std::atoi(argv[3]);
    FsParams g;
    g.nb = head[1]; g.ne = head[2]; g.nab = head[3]; g.nae = head[4];
    g.scale_e = (double)(g.ne - 1);
    g.he = 1.0 / (double)(g.ne - 1);
    std::vector<float> tables((size_t)total_rows * SHEMS_NCOL);
    if (std::fread(tables.data(), sizeof(float), tables.size(), f) != tables.size()) { std::fprintf(stderr, "short table\n"); return 2; }
    std::fclose(f);
    // what the entry point refuses
    const int64_t f0 = (int64_t)P.cfg.table_row0 + P.forecast_off;
    if (T < 1 || H < 1 || c < 1 || c > H || P.idx0 < 1 || P.idx0 + T > P.cfg.nrow || P.cfg.table_row0 < 0 ||
        (int64_t)P.cfg.table_row0 + P.cfg.nrow > total_rows || f0 < 0 || f0 + P.cfg.nrow > total_rows) {
        std::fprintf(stderr, "refused\n");
        return 3;
    }
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    std::vector<double> planes(2 * (size_t)N), V((size_t)(T + 1) * N, 0.0);
    std::vector<int32_t> arg((size_t)T * N, -1);
    std::vector<char> have((size_t)T + 1, 0);
    for (int w = 0; w < fs_plan_windows(T, c); ++w) {
        const int j = w * c, hi = fs_plan_end(j, H, T), lo = fs_plan_first(j, true);
        for (int n = 0; n < N; ++n) planes[n] = 0.0;
        if (fs_plan_keeps_plane(j, c, T, hi)) have[hi] = 1;                  // the zero plane
        int cur = 0;
        for (int t = hi - 1; t >= lo; --t, cur ^= 1) {
            const int64_t base = (int64_t)P.cfg.table_row0 + P.idx0 + t - 1;   // the true row of hour t
            const float *row = tables.data() + (base + fs_belief_off(t, j, P.forecast_off)) * SHEMS_NCOL;
            const float *nx = tables.data() + (base + 1 + fs_belief_off(t + 1, j, P.forecast_off)) * SHEMS_NCOL;
            const double *Vn = planes.data() + (size_t)cur * N;
            double *Vt = planes.data() + (size_t)(cur ^ 1) * N;
            for (int node = 0; node < N; ++node) {
                const int ib = node / g.ne, ie = node - ib * g.ne;
                const EnvIn s{fs_soc_b_node(P, g.nb, ib), fs_soc_ev_node(g, ie), row[0], row[2], row[3], row[4]};
                double best_v = -__builtin_inf();
                int best_a = kFsNoAction;
                for (int a = 0; a < NA; ++a) {
                    const int ab = a / g.nae, ae = a - ab * g.nae;
                    const double q = fs_q(P.cfg, s, row[0], nx[0], nx[1], fs_target(ab, g.nab), fs_target(ae, g.nae), Vn, g, P.scale_b);
                    if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
                }
                Vt[node] = best_v;
                if (fs_plan_keeps_plane(j, c, T, t)) { V[(size_t)t * N + node] = best_v; have[t] = 1; }
                if (fs_plan_keeps_argmax(j, c, T, t)) arg[(size_t)t * N + node] = best_a;
            }
        }
    }
    for (int t = 0; t <= T; ++t) {
        if (!have[t]) { std::fprintf(stderr, "no window keeps plane %d\n", t); return 4; }
        for (int n = 0; n < N; ++n) {
            uint64_t bits;
            std::memcpy(&bits, &V[(size_t)t * N + n], 8);
            std::printf("V %d %d %016" PRIx64 "\n", t, n, bits);
        }
    }
    for (int t = 0; t < T; ++t)
        for (int n = 0; n < N; ++n) std::printf("A %d %d %d\n", t, n, (int)arg[(size_t)t * N + n]);
    return 0;
}

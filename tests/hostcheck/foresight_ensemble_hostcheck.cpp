// foresight_ensemble_hostcheck.cpp -- TEST TOOL, not a product path.  A stand-alone program (g++ -ffp-contract=off) that evaluates the
// ensemble controller's Qbar of csrc/shems_foresight_core.h -- fs_step once per action, then fs_q_ens over the K scenario planes, every
// scenario's next row taken where fs_belief_off says -- for every action at every hour of a given trajectory, as k_fs_track_ens does
// on the GPU, so that a GPU-less container can compare the bits with the NumPy twin.  The GPU tests (-m gpu) remain the
// authoritative check.
//
//   foresight_ensemble_hostcheck INPUT
// INPUT (binary, written by the test): int32 total_rows, nb, ne, nab, nae, T, K; K records of 72 bytes (shems_foresight_problem: cfg,
// idx0, forecast_off, scale_b, hb as foresight.make_problems fills them, one per scenario); float64 w[K]; float32 rows
// [total_rows][8]; float64 planes [K][T + 1][nb * ne]; float32 obs [T][9], the state the trajectory is in before each hour.
// Output: one line "t a bits" (Qbar as 16 hex digits) per hour and action.
#include <cinttypes>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_foresight_core.h"

using namespace shems;

template <class T> static bool read_n(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s INPUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[7];
    static_assert(sizeof(shems_foresight_problem) == 72 && offsetof(shems_foresight_problem, forecast_off) == 52, "the record of include/shems_hip.h");
    if (std::fread(head, sizeof head, 1, f) != 1) { std::fprintf(stderr, "short input\n"); return 2; }
    const int64_t total_rows = head[0];
    const int T = head[5], K = head[6];
    FsParams g;
    g.nb = head[1]; g.ne = head[2]; g.nab = head[3]; g.nae = head[4];
    g.scale_e = (double)(g.ne - 1);
    g.he = 1.0 / (double)(g.ne - 1);
    if (T < 1 || K < 1 || K > kFsMaxScen || total_rows < 2 || g.nb < 2 || g.ne < 2 || g.nab < 1 || g.nae < 1) { std::fprintf(stderr, "refused\n"); return 3; }
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    std::vector<shems_foresight_problem> R((size_t)K);
    std::vector<double> w((size_t)K), V((size_t)K * (T + 1) * N);
    std::vector<float> tables((size_t)total_rows * SHEMS_NCOL), obs((size_t)T * SHEMS_NSTATE);
    if (!read_n(f, R) || !read_n(f, w) || !read_n(f, tables) || !read_n(f, V) || !read_n(f, obs)) { std::fprintf(stderr, "short input\n"); return 2; }
    std::fclose(f);
    // what the entry point and the kernel's entry checks refuse
    const shems_foresight_problem &P = R[0];
    if (P.idx0 < 1 || P.idx0 + T > P.cfg.nrow || P.cfg.table_row0 < 0 || (int64_t)P.cfg.table_row0 + P.cfg.nrow > total_rows) { std::fprintf(stderr, "refused\n"); return 3; }
    for (int k = 0; k < K; ++k) {
        const int64_t f0 = (int64_t)P.cfg.table_row0 + R[k].forecast_off;
        if (R[k].idx0 != P.idx0 || R[k].cfg.table_row0 != P.cfg.table_row0 || R[k].cfg.nrow != P.cfg.nrow || f0 < 0 || f0 + P.cfg.nrow > total_rows ||
            !(w[k] > 0.0) || !(w[k] <= 1.7976931348623157e308)) {
            std::fprintf(stderr, "refused\n");
            return 3;
        }
    }
    const int64_t v_stride = (int64_t)(T + 1) * N;
    std::vector<float> h_next((size_t)K), soc_ev_next((size_t)K);
    for (int t = 0; t < T; ++t) {
        const int64_t base = (int64_t)P.cfg.table_row0 + P.idx0 + t - 1;    // the true row of hour t
        const float h_cur = tables[(size_t)base * SHEMS_NCOL];
        for (int k = 0; k < K; ++k) {
            const float *nx = tables.data() + (base + 1 + fs_belief_off(t + 1, t, R[k].forecast_off)) * SHEMS_NCOL;
            h_next[k] = nx[0];
            soc_ev_next[k] = nx[1];
        }
        const float *o = obs.data() + (size_t)t * SHEMS_NSTATE;
        const EnvIn s{o[0], o[1], o[2], o[3], o[4], o[5]};
        const double *Vn = V.data() + (size_t)(t + 1) * N;                   // plane t + 1 of scenario 0
        for (int a = 0; a < NA; ++a) {
            const int ab = a / g.nae, ae = a - ab * g.nae;
            const FsStep st = fs_step(P.cfg, s, fs_target(ab, g.nab), fs_target(ae, g.nae));
            const double q = fs_q_ens(st, h_cur, K, w.data(), h_next.data(), soc_ev_next.data(), Vn, v_stride, g, P.scale_b);
            uint64_t bits;
            std::memcpy(&bits, &q, 8);
            std::printf("%d %d %016" PRIx64 "\n", t, a, bits);
        }
    }
    return 0;
}

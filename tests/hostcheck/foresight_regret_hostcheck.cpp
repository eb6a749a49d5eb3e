// foresight_regret_hostcheck.cpp -- TEST TOOL, not a product path.  A stand-alone program (g++ -ffp-contract=off) that audits tracked
// passes of one problem with the definition at the end of csrc/shems_foresight_core.h -- fs_audit_hour, fs_audit_q, fs_audit_achieved,
// fs_audit_v_state -- in a serial loop over passes, hours and actions that does what k_fs_audit does on the GPU, and prints what
// shems_foresight_audit_dev would leave, so that a GPU-less container can compare it with the oracle twin.  The GPU tests (-m gpu)
// remain the authoritative check.
//
//   foresight_regret_hostcheck INPUT
// INPUT (binary, written by the test): int32 total_rows, nb, ne, nab, nae, T, n_pass; the 72 bytes of one shems_foresight_problem (as
// foresight.make_problems fills them); float32 rows [total_rows][8]; float64 V [T + 1][nb * ne]; float64 results [n_pass][T][23].
// Output: one line "e t best_q achieved_q v_state best_action status" per (pass, hour), the float64 as 16 hex digits.
#include <cinttypes>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_foresight_core.h"

using namespace shems;

static uint64_t bits(double x)
{
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s INPUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[7];
    shems_foresight_problem P;
    static_assert(sizeof(shems_foresight_problem) == 72, "the record of include/shems_hip.h");
    if (std::fread(head, sizeof head, 1, f) != 1 || std::fread(&P, sizeof P, 1, f) != 1) { std::fprintf(stderr, "short input\n"); return 2; }
    const int64_t total_rows = head[0];
    const int T = head[5], n_pass = head[6];
    FsParams g;
    g.nb = head[1]; g.ne = head[2]; g.nab = head[3]; g.nae = head[4];
    g.scale_e = (double)(g.ne - 1);
    g.he = 1.0 / (double)(g.ne - 1);
    if (total_rows < 2 || g.nb < 2 || g.ne < 2 || g.nab < 1 || g.nae < 1 || T < 1 || n_pass < 1) { std::fprintf(stderr, "refused\n"); return 3; }
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    std::vector<float> tables((size_t)total_rows * SHEMS_NCOL);
    std::vector<double> V((size_t)(T + 1) * N), res((size_t)n_pass * T * SHEMS_NRESULT);
    if (std::fread(tables.data(), sizeof(float), tables.size(), f) != tables.size() || std::fread(V.data(), 8, V.size(), f) != V.size() ||
        std::fread(res.data(), 8, res.size(), f) != res.size()) {
        std::fprintf(stderr, "short arrays\n");
        return 2;
    }
    std::fclose(f);
    for (int e = 0; e < n_pass; ++e) {
        for (int t = 0; t < T; ++t) {
            const double *r = res.data() + ((size_t)e * T + t) * SHEMS_NRESULT;
            const double *Vt = V.data() + (size_t)t * N, *Vn = Vt + N;
            FsAuditHour h;
            if (!fs_audit_hour(P, tables.data(), total_rows, r, t, h)) {
                std::printf("%d %d nan nan nan -1 %d\n", e, t, (int)SHEMS_ERR_INDEX);
                continue;
            }
            double best_v = -__builtin_inf();
            int best_a = kFsNoAction;
            for (int a = 0; a < NA; ++a) {
                const double q = fs_audit_q(P, h, a, Vn, g);
                if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
            }
            const double ach = fs_audit_achieved(P, r, t + 1 < T ? r + SHEMS_NRESULT : nullptr, Vn, g);
            const double vs = fs_audit_v_state(P, h, Vt, g);
            std::printf("%d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d 0\n", e, t, bits(best_v), bits(ach), bits(vs), best_a);
        }
    }
    return 0;
}

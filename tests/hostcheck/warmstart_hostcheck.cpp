// warmstart_hostcheck.cpp -- TEST TOOL, not a product path.  A stand-alone program (g++ -ffp-contract=off) that turns tracked passes of
// one problem into transitions and returns-to-go with the definition in csrc/shems_foresight_core.h -- fs_returns, fs_transition_hour,
// fs_demo_slot, fs_demo_check_ring -- in a serial loop over passes and hours that does what k_fs_returns and k_fs_transitions do on
// the GPU, and prints what shems_foresight_transitions_dev would write, so that a GPU-less container can compare it with the NumPy
// twin.  The GPU tests (-m gpu) remain the authoritative check.
//
//   warmstart_hostcheck INPUT
// INPUT (binary, written by the test): int32 total_rows, T, n_pass, mode (0: TD, 1: MC), tail, 0; float32 gamma, 0; int64 capacity,
// pos; the 72 bytes of one shems_foresight_problem (as foresight.make_problems fills them); float32 rows [total_rows][8]; float64
// results [n_pass][T][23].
// Output: "ring K" when fs_demo_check_ring refuses (exit code 3); otherwise per pass "G e" and the T returns as 16 hex digits each,
// "status e v", and one line per (pass, hour < T - tail): "e t slot", the 21 float32 (s[0..8], a[0..1], r, s2[0..8]) as 8 hex digits
// each and done, or "e t -1" for an hour that gives no transition.
#include <cinttypes>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_foresight_core.h"

using namespace shems;

static uint32_t bits(float x)
{
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

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
    int32_t head[6];
    float fl[2];
    int64_t ring[2];
    shems_foresight_problem P;
    static_assert(sizeof(shems_foresight_problem) == 72, "the record of include/shems_hip.h");
    if (std::fread(head, sizeof head, 1, f) != 1 || std::fread(fl, sizeof fl, 1, f) != 1 || std::fread(ring, sizeof ring, 1, f) != 1 ||
        std::fread(&P, sizeof P, 1, f) != 1) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    const int64_t total_rows = head[0], capacity = ring[0], pos = ring[1];
    const int T = head[1], n_pass = head[2], mode = head[3], tail = head[4];
    const float gamma = fl[0];
    if (total_rows < 2 || T < 2 || n_pass < 1 || (mode != SHEMS_FS_TRANS_TD && mode != SHEMS_FS_TRANS_MC) || tail < 1 || tail >= T ||
        !(gamma >= 0.0f && gamma <= 1.0f)) {
        std::fprintf(stderr, "refused\n");
        return 3;
    }
    const int keep = T - tail;
    if (const int k = fs_demo_check_ring(capacity, pos, n_pass, keep)) { std::printf("ring %d\n", k); return 3; }
    std::vector<float> tables((size_t)total_rows * SHEMS_NCOL);
    std::vector<double> res((size_t)n_pass * T * SHEMS_NRESULT), G((size_t)T);
    if (std::fread(tables.data(), sizeof(float), tables.size(), f) != tables.size() || std::fread(res.data(), 8, res.size(), f) != res.size()) {
        std::fprintf(stderr, "short arrays\n");
        return 2;
    }
    std::fclose(f);
    for (int e = 0; e < n_pass; ++e) {
        const double *rows = res.data() + (size_t)e * T * SHEMS_NRESULT;
        const bool pass_ok = fs_returns(P, tables.data(), total_rows, rows, T, gamma, G.data());
        int status = mode == SHEMS_FS_TRANS_MC && !pass_ok ? (int)SHEMS_ERR_INDEX : 0;
        std::printf("G %d", e);
        for (int t = 0; t < T; ++t) std::printf(" %016" PRIx64, bits(G[t]));
        std::printf("\n");
        for (int t = 0; t < keep; ++t) {
            FsTransition x;
            if (mode == SHEMS_FS_TRANS_MC && G[0] != G[0]) { std::printf("%d %d -1\n", e, t); continue; }
            if (!fs_transition_hour(P, tables.data(), total_rows, rows + (size_t)t * SHEMS_NRESULT, t, x)) {
                status = (int)SHEMS_ERR_INDEX;
                std::printf("%d %d -1\n", e, t);
                continue;
            }
            std::printf("%d %d %" PRId64, e, t, fs_demo_slot(pos, e, keep, t, capacity));
            for (int k = 0; k < SHEMS_NSTATE; ++k) std::printf(" %08" PRIx32, bits(x.d.s[k]));
            std::printf(" %08" PRIx32 " %08" PRIx32, bits(x.d.a[0]), bits(x.d.a[1]));
            std::printf(" %08" PRIx32, bits(mode == SHEMS_FS_TRANS_MC ? (float)G[t] : x.rew));
            for (int k = 0; k < SHEMS_NSTATE; ++k) std::printf(" %08" PRIx32, bits(x.s2[k]));
            std::printf(" %d\n", mode == SHEMS_FS_TRANS_MC ? 1 : 0);
        }
        std::printf("status %d %d\n", e, status);
    }
    return 0;
}

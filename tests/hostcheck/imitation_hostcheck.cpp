// imitation_hostcheck.cpp -- TEST TOOL, not a product path.  A stand-alone program (g++ -ffp-contract=off) that turns tracked passes of
// one problem into demonstrations with the definition in csrc/shems_foresight_core.h -- fs_demo_hour, fs_demo_slot,
// fs_demo_check_ring -- in a serial loop over passes and hours that does what k_fs_demos does on the GPU, and prints what
// shems_foresight_demos_dev would write, so that a GPU-less container can compare it with the NumPy twin.  The GPU tests (-m gpu)
// remain the authoritative check.
//
//   imitation_hostcheck INPUT
// INPUT (binary, written by the test): int32 total_rows, nb, ne, nab, nae, T, n_pass, mode (0: target labels, 1: index labels); int64
// capacity, pos; the 72 bytes of one shems_foresight_problem (as foresight.make_problems fills them); float32 rows [total_rows][8];
// float64 results [n_pass][T][23]; the labels: float32 [n_pass][T][2] (mode 0) or int32 [n_pass][T] (mode 1).
// Output: "ring K" when fs_demo_check_ring refuses (exit code 3); otherwise one line per (pass, hour): "e t slot" and the eleven
// float32 (s[0..8], a[0..1]) as 8 hex digits each, or "e t -1 status" for an hour that gives no pair.
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

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s INPUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[8];
    int64_t ring[2];
    shems_foresight_problem P;
    static_assert(sizeof(shems_foresight_problem) == 72, "the record of include/shems_hip.h");
    if (std::fread(head, sizeof head, 1, f) != 1 || std::fread(ring, sizeof ring, 1, f) != 1 || std::fread(&P, sizeof P, 1, f) != 1) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    const int64_t total_rows = head[0], capacity = ring[0], pos = ring[1];
    const int T = head[5], n_pass = head[6], mode = head[7];
    FsParams g;
    g.nb = head[1]; g.ne = head[2]; g.nab = head[3]; g.nae = head[4];
    g.scale_e = (double)(g.ne - 1);
    g.he = 1.0 / (double)(g.ne - 1);
    if (total_rows < 2 || g.nb < 2 || g.ne < 2 || g.nab < 1 || g.nae < 1 || T < 1 || n_pass < 1 || (mode != 0 && mode != 1)) {
        std::fprintf(stderr, "refused\n");
        return 3;
    }
    if (const int k = fs_demo_check_ring(capacity, pos, n_pass, T)) { std::printf("ring %d\n", k); return 3; }
    std::vector<float> tables((size_t)total_rows * SHEMS_NCOL), tgt(mode == 0 ? (size_t)n_pass * T * 2 : 0);
    std::vector<double> res((size_t)n_pass * T * SHEMS_NRESULT);
    std::vector<int32_t> act(mode == 1 ? (size_t)n_pass * T : 0);
    if (std::fread(tables.data(), sizeof(float), tables.size(), f) != tables.size() || std::fread(res.data(), 8, res.size(), f) != res.size() ||
        (mode == 0 ? std::fread(tgt.data(), 4, tgt.size(), f) != tgt.size() : std::fread(act.data(), 4, act.size(), f) != act.size())) {
        std::fprintf(stderr, "short arrays\n");
        return 2;
    }
    std::fclose(f);
    for (int e = 0; e < n_pass; ++e) {
        for (int t = 0; t < T; ++t) {
            const size_t at = (size_t)e * T + t;
            FsDemo d;
            if (!fs_demo_hour(P, tables.data(), total_rows, res.data() + at * SHEMS_NRESULT, t, mode == 0 ? tgt.data() + at * 2 : nullptr,
                              mode == 1 ? act[at] : -1, g, d)) {
                std::printf("%d %d -1 %d\n", e, t, (int)SHEMS_ERR_INDEX);
                continue;
            }
            std::printf("%d %d %" PRId64, e, t, fs_demo_slot(pos, e, T, t, capacity));
            for (int k = 0; k < SHEMS_NSTATE; ++k) std::printf(" %08" PRIx32, bits(d.s[k]));
            std::printf(" %08" PRIx32 " %08" PRIx32 "\n", bits(d.a[0]), bits(d.a[1]));
        }
    }
    return 0;
}

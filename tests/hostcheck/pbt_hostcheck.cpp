// pbt_hostcheck.cpp -- csrc/shems_pbt_core.h on the host (g++ -ffp-contract=off): one round of population-based training over a binary
// input file, the result printed as hex for tests/test_pbt_host.py to compare with the NumPy twin (tests/pbt_ref.py) bit for bit.
//   input:  shems_pbt_params (104 bytes); int32 count; int32 pop[count]; double score[count]; shems_group_hparams hp[count]
//   output: "check <0 | item>", "hp" <hex bytes of the records after the round>, "parent" and "rank" <decimal>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_pbt_core.h"

using namespace shems;

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: pbt_hostcheck <input file>\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    static_assert(sizeof(shems_pbt_params) == 104 && sizeof(shems_group_hparams) == 40 && sizeof(shems_pbt_range) == 16, "the header's sizes");
    shems_pbt_params p;
    int32_t count = 0;
    if (std::fread(&p, sizeof p, 1, f) != 1 || std::fread(&count, 4, 1, f) != 1 || count < 1 || count > kPbtMaxCount) {
        std::fprintf(stderr, "bad header\n");
        std::fclose(f);
        return 2;
    }
    const size_t n = (size_t)count;
    std::vector<int32_t> pop(n), parent(n), rank(n);
    std::vector<double> score(n);
    std::vector<shems_group_hparams> hp(n);
    const bool ok = std::fread(pop.data(), 4, n, f) == n && std::fread(score.data(), 8, n, f) == n && std::fread(hp.data(), sizeof(shems_group_hparams), n, f) == n;
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }
    const char *what = "";
    const int bad = pbt_params_check(p, &what);
    std::printf("check %d %s\n", bad, bad ? what : "");
    if (bad) return 0;
    pbt_round_host(p, count, pop.data(), score.data(), hp.data(), parent.data(), rank.data());
    std::printf("hp");
    const unsigned char *b = (const unsigned char *)hp.data();
    for (size_t i = 0; i < n * sizeof(shems_group_hparams); ++i) std::printf(" %02x", b[i]);
    std::printf("\nparent");
    for (int32_t x : parent) std::printf(" %d", (int)x);
    std::printf("\nrank");
    for (int32_t x : rank) std::printf(" %d", (int)x);
    std::printf("\n");
    return 0;
}

// per_hostcheck.cpp -- csrc/shems_per_core.h on the host (g++ -ffp-contract=off): the prioritized sampler's steps 1-4 and the write-back's
// powers over a binary input file, printed as hex words for tests/test_per_host.py to compare with the NumPy twin bit for bit.
//   input:  int64 capacity, ring_len, fresh_pos, fresh_count; uint64 seed; uint32 tick; int32 batch; float pmax, beta, alpha, eps_p;
//           float prio[capacity]; float diff[128]
//   output: "T <hex>", "S <nb hex>", "C <nb hex>", "u", "t", "idx", "w", "prio <capacity hex>" (after the fresh fill), "pnew <128 hex>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_per_core.h"

using namespace shems;

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
template <class V> static void line(const char *name, const V &v, size_t n)
{
    std::printf("%s", name);
    for (size_t i = 0; i < n; ++i) std::printf(" %08x", bits(v[i]));
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: per_hostcheck <input file>\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int64_t hdr[4]; uint64_t seed; uint32_t tick; int32_t batch; float sc[4];
    bool ok = std::fread(hdr, 8, 4, f) == 4 && std::fread(&seed, 8, 1, f) == 1 && std::fread(&tick, 4, 1, f) == 1 &&
              std::fread(&batch, 4, 1, f) == 1 && std::fread(sc, 4, 4, f) == 4;
    const int64_t capacity = hdr[0], ring_len = hdr[1], fresh_pos = hdr[2], fresh_count = hdr[3];
    if (!ok || capacity < 1 || capacity > kPerMaxSlots || ring_len < 1 || ring_len > capacity || batch < 1 || batch > kPerCols) {
        std::fprintf(stderr, "bad header\n");
        std::fclose(f);
        return 2;
    }
    std::vector<float> prio((size_t)capacity), diff(kPerCols);
    ok = std::fread(prio.data(), 4, (size_t)capacity, f) == (size_t)capacity && std::fread(diff.data(), 4, kPerCols, f) == (size_t)kPerCols;
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }
    const int64_t nb = per_blocks(ring_len);
    std::vector<float> S((size_t)nb), C((size_t)nb), w(kPerCols), u(kPerCols), tm(kPerCols), pnew(kPerCols);
    std::vector<int32_t> idx(kPerCols);
    const PerDrawHost d = per_sample_host(prio.data(), sc[0], capacity, ring_len, fresh_pos, fresh_count, seed, tick, batch, sc[1], S.data(),
                                          C.data(), idx.data(), w.data(), u.data(), tm.data());
    for (int m = 0; m < kPerCols; ++m) pnew[m] = per_priority(diff[m], sc[3], sc[2]);
    std::printf("T %08x\n", bits(d.T));
    line("S", S, (size_t)nb);
    line("C", C, (size_t)nb);
    line("u", u, kPerCols);
    line("t", tm, kPerCols);
    std::printf("idx");
    for (int m = 0; m < kPerCols; ++m) std::printf(" %08x", (uint32_t)idx[m]);
    std::printf("\n");
    line("w", w, kPerCols);
    line("prio", prio, (size_t)capacity);
    line("pnew", pnew, kPerCols);
    return 0;
}

// nstep_hostcheck.cpp -- csrc/shems_nstep_core.h on the host (g++ -ffp-contract=off): the per-step fold and the bulk conversion over a
// binary input file, the resulting ring printed as hex words for tests/test_nstep_host.py to compare with the NumPy twin bit for bit.
//   input:  int64 mode (0 fold, 1 bulk), n, T, episodes, window, capacity, pos0; float gamma; then
//           fold: per hour of every episode  float s[window][9], a[window][2], r[window], s2[window][9]; uint8 done[window]
//           bulk: float s[N][9], a[N][2], r[N], s2[N][9]; uint8 done[N], N = episodes * T  (episode e's hour t at slot e * T + t)
//   the ring starts as the sentinel (-777.25f, 0xAB); pushed starts at pos0.
//   output: "pushed <decimal>", "gamma_n <hex>", "s", "a", "r", "s2" <hex words>, "done" <hex bytes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_nstep_core.h"

using namespace shems;

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static void line(const char *name, const std::vector<float> &v)
{
    std::printf("%s", name);
    for (float x : v) std::printf(" %08x", bits(x));
    std::printf("\n");
}

struct Ring {
    std::vector<float> s, a, r, s2;
    std::vector<uint8_t> done;
    explicit Ring(int64_t cap, float fill = 0.0f, uint8_t b = 0)
        : s((size_t)cap * 9, fill), a((size_t)cap * 2, fill), r((size_t)cap, fill), s2((size_t)cap * 9, fill), done((size_t)cap, b) {}
    NstepRingHost view() { return NstepRingHost{(int64_t)r.size(), s.data(), a.data(), r.data(), s2.data(), done.data()}; }
    bool read(FILE *f, int64_t n)
    {
        const size_t k = (size_t)n;
        return std::fread(s.data(), 4, k * 9, f) == k * 9 && std::fread(a.data(), 4, k * 2, f) == k * 2 && std::fread(r.data(), 4, k, f) == k &&
               std::fread(s2.data(), 4, k * 9, f) == k * 9 && std::fread(done.data(), 1, k, f) == k;
    }
};

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: nstep_hostcheck <input file>\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int64_t h[7];
    float gamma;
    if (std::fread(h, 8, 7, f) != 7 || std::fread(&gamma, 4, 1, f) != 1) { std::fprintf(stderr, "short header\n"); std::fclose(f); return 2; }
    const int64_t mode = h[0], n = h[1], T = h[2], episodes = h[3], window = h[4], capacity = h[5], pos0 = h[6];
    if ((mode != 0 && mode != 1) || n < 1 || n > kNstepMax || T < n || T > 4096 || episodes < 1 || episodes > 4096 || window < 1 || window > 4096 ||
        capacity < 1 || capacity > 65536 || pos0 < 0 || (mode == 0 && window > capacity)) {
        std::fprintf(stderr, "bad header\n");
        std::fclose(f);
        return 2;
    }
    Ring ring(capacity, -777.25f, 0xAB);
    int64_t pushed = pos0;
    bool ok = true;
    if (mode == 0) {
        Ring stage(window);
        std::vector<float> hs((size_t)(n * window * 9)), ha((size_t)(n * window * 2)), hr((size_t)(n * window));
        for (int64_t e = 0; e < episodes && ok; ++e)
            for (int64_t t = 0; t < T && ok; ++t) {
                ok = stage.read(f, window);
                if (ok)
                    pushed += nstep_fold_host((int)n, window, gamma, hs.data(), ha.data(), hr.data(), stage.view(), ring.view(), pushed % capacity,
                                              (int32_t)t);
            }
    } else {
        Ring src(episodes * T);
        ok = src.read(f, episodes * T);
        if (ok) pushed += nstep_from_episodes_host(src.view(), episodes, T, (int)n, gamma, ring.view(), pushed % capacity);
    }
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }
    std::printf("pushed %lld\n", (long long)pushed);
    std::printf("gamma_n %08x\n", bits(nstep_gamma(gamma, (int)n)));
    line("s", ring.s);
    line("a", ring.a);
    line("r", ring.r);
    line("s2", ring.s2);
    std::printf("done");
    for (uint8_t b : ring.done) std::printf(" %02x", b);
    std::printf("\n");
    return 0;
}

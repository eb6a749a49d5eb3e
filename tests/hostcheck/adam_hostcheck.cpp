// adam_hostcheck.cpp -- csrc/shems_adam.h on the host (g++ -ffp-contract=off -Itests/hostcheck/hip_host): adam_math over a binary input
// file, the updated arrays written to a binary output file for tests/test_adam_horizon_host.py to hold to tests/adam_ref.py, and the
// same elements against long-double arithmetic here.  With no input file: the horizon of the beta powers as C doubles advance them.
//   input:  int64 n; double eta, bp1, bp2, gscale; float tau; float p[n], m[n], v[n], target[n], g[n]
//   output file: float p[n], m[n], v[n], target[n] after the update
//   stdout: "longdouble <name> max_ulp <decimal> differing <count>" for p, m, v, target -- the distance between adam_math's value and the
//           long-double evaluation of the reference's statements rounded once to fp32, in fp32 ulp of the larger of |old| and |new|
//   horizon: "bp1 <step> <hex bits>" / "bp2 <step> <hex bits>" at the steps asked for, "subnormal <step>", "settled <step> <hex bits>",
//            "zero <0 | step>"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_adam.h"

using namespace shems;

static uint64_t bits(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

static int horizon(int argc, char **argv)
{
    // the native loop's record (csrc/shems_train.hip): bpc[0] *= 0.9; bpc[1] *= 0.999; after every update
    const long long steps = std::atoll(argv[2]);
    double b1 = 0.9, b2 = 0.999;
    long long subnormal = 0, settled = 0, zero = 0;
    for (long long t = 1; t <= steps; ++t) {                  // (b1, b2) are what update t receives
        for (int a = 3; a < argc; ++a)
            if (std::atoll(argv[a]) == t) std::printf("bp1 %lld %016llx\nbp2 %lld %016llx\n", t, (unsigned long long)bits(b1), t, (unsigned long long)bits(b2));
        if (!(b1 > 0.0 && b1 < 1.0 && b2 > 0.0 && b2 < 1.0) && !zero) zero = t;
        if (!subnormal && std::fpclassify(b1) == FP_SUBNORMAL) subnormal = t;
        const double n1 = b1 * 0.9;
        if (!settled && n1 == b1) settled = t;
        b1 = n1; b2 *= 0.999;
    }
    std::printf("subnormal %lld\nsettled %lld %016llx\nzero %lld\n", subnormal, settled, (unsigned long long)bits(b1), zero);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && std::strcmp(argv[1], "horizon") == 0) return horizon(argc, argv);
    if (argc != 3) { std::fprintf(stderr, "usage: adam_hostcheck <input file> <output file> | adam_hostcheck horizon <steps> [step ...]\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int64_t n = 0;
    double sc[4];
    float tau = 0;
    if (std::fread(&n, 8, 1, f) != 1 || std::fread(sc, 8, 4, f) != 4 || std::fread(&tau, 4, 1, f) != 1 || n < 1 || n > (1 << 24)) {
        std::fprintf(stderr, "bad header\n");
        std::fclose(f);
        return 2;
    }
    const size_t k = (size_t)n;
    std::vector<float> p(k), m(k), v(k), t(k), g(k);
    const bool ok = std::fread(p.data(), 4, k, f) == k && std::fread(m.data(), 4, k, f) == k && std::fread(v.data(), 4, k, f) == k &&
                    std::fread(t.data(), 4, k, f) == k && std::fread(g.data(), 4, k, f) == k;
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }
    const double eta = sc[0], bp1 = sc[1], bp2 = sc[2], gscale = sc[3];
    if (!(bp1 > 0.0 && bp1 < 1.0 && bp2 > 0.0 && bp2 < 1.0)) { std::fprintf(stderr, "beta powers must be in (0,1)\n"); return 2; }   // check_adam's condition
    // the host-side quotients exactly as adam_ctx (csrc/shems_ddpg.hip) forms them
    const AdamCtx c{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (int)n, 0, eta, bp1, bp2, gscale, eta / (1.0 - bp1), 1.0 / (1.0 - bp2), tau};
    double worst[4] = {0, 0, 0, 0};
    int64_t differing[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < k; ++i) {
        const float old[4] = {p[i], m[i], v[i], t[i]};
        adam_math(c, g[i], m[i], v[i], p[i], t[i]);
        // the reference's statements in long double, each array statement rounded once to fp32 (ddpg_oracle.Adam rounds Float64 -> Float32).
        // The step is formed from adam_math's own new moments, which the lines above it hold on their own: where m and g cancel, long
        // double keeps bits of b1 m + (1 - b1) g that the definition's Float64 does not, and a step formed from THAT m would differ.
        const long double gl = (long double)(float)((double)g[i] * gscale);
        const float m_ld = (float)((long double)0.9 * (long double)old[1] + (long double)(1.0 - 0.9) * gl);
        const float g2 = (float)gl * (float)gl;
        const float v_ld = (float)((long double)0.999 * (long double)old[2] + (long double)(1.0 - 0.999) * (long double)g2);
        const long double d_ld = (long double)m[i] / (1.0L - (long double)bp1) / (sqrtl((long double)v[i] / (1.0L - (long double)bp2)) + (long double)1e-8) * (long double)eta;
        const float p_ld = old[0] - (float)d_ld;
        const float t_ld = (1.0f - tau) * old[3] + tau * p_ld;
        const float got[4] = {p[i], m[i], v[i], t[i]}, want[4] = {p_ld, m_ld, v_ld, t_ld};
        for (int a = 0; a < 4; ++a) {
            // in ulp of the larger of |old| and |expected new|: the resolution the operands of the statement were held at
            const float big = std::fmax(std::fabs(old[a]), std::fabs(want[a]));
            const double unit = (double)std::nextafterf(big, INFINITY) - (double)big;
            const double d = std::fabs((double)got[a] - (double)want[a]) / unit;
            if (d != 0) ++differing[a];
            if (d > worst[a]) worst[a] = d;
        }
    }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const bool wrote = std::fwrite(p.data(), 4, k, o) == k && std::fwrite(m.data(), 4, k, o) == k && std::fwrite(v.data(), 4, k, o) == k &&
                       std::fwrite(t.data(), 4, k, o) == k;
    if (std::fclose(o) != 0 || !wrote) { std::fprintf(stderr, "short write\n"); return 2; }
    const char *names[4] = {"p", "m", "v", "target"};
    for (int a = 0; a < 4; ++a) std::printf("longdouble %s max_ulp %.3f differing %lld\n", names[a], worst[a], (long long)differing[a]);
    return 0;
}

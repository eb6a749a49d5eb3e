// bc_hostcheck.cpp -- TEST TOOL, not a product path.  A stand-alone program (g++ -ffp-contract=off) that runs the scalar arithmetic of the
// behaviour-regularised actor loss with the definition in csrc/shems_bc_core.h -- bc_lambda, bc_dloss, bc_loss -- on inputs the test
// writes, in a serial loop, and prints the bit patterns, so that a GPU-less container can compare them with the NumPy twin
// (tests/bc_ref.py).  The GPU tests (-m gpu) remain the authoritative check of the kernel.
//
//   bc_hostcheck INPUT
// INPUT (binary, written by the test): int32 n, int32 normalise; float32 alpha, weight, batch, 0; then float32 arrays qbar [n], da [n],
// diff [n], neg_mean_q [n], mse [n].
// Output, one line per row i: "i", the bits of lambda_i = bc_lambda(alpha, qbar[i], normalise), of bc_dloss(lambda_i, da[i], weight,
// diff[i], batch) and of bc_loss(lambda_i, neg_mean_q[i], weight, mse[i]) (8 hex digits each).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_bc_core.h"

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
    int32_t n = 0, normalise = 0;
    float hp[4];
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&normalise, 4, 1, f) != 1 || std::fread(hp, sizeof hp, 1, f) != 1) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    if (n < 1 || n > (1 << 20) || (normalise != 0 && normalise != 1)) { std::fprintf(stderr, "refused\n"); return 3; }
    const size_t N = (size_t)n;
    std::vector<float> qbar(N), da(N), diff(N), nmq(N), mse(N);
    if (std::fread(qbar.data(), 4, N, f) != N || std::fread(da.data(), 4, N, f) != N || std::fread(diff.data(), 4, N, f) != N ||
        std::fread(nmq.data(), 4, N, f) != N || std::fread(mse.data(), 4, N, f) != N) {
        std::fprintf(stderr, "short arrays\n");
        return 2;
    }
    std::fclose(f);
    const float alpha = hp[0], weight = hp[1], batch = hp[2];
    for (size_t i = 0; i < N; ++i) {
        const float lam = bc_lambda(alpha, qbar[i], normalise);
        std::printf("%zu %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", i, bits(lam), bits(bc_dloss(lam, da[i], weight, diff[i], batch)),
                    bits(bc_loss(lam, nmq[i], weight, mse[i])));
    }
    return 0;
}

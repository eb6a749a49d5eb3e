// foresight_hostcheck.cpp -- TEST TOOL, not a product path.  Compiles csrc/shems_foresight_core.h as ordinary host C++
// (g++ -ffp-contract=off) and runs the backward sweep of ONE problem serially, so that the recursion the GPU threads execute can be
// compared with a NumPy twin on the oracle inside a GPU-less container.  The GPU tests (-m gpu) remain the authoritative check.
#include <cstdint>
#include "../../master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd/csrc/shems_foresight_core.h"

using namespace shems;

static FsParams params(const shems_foresight_grid *grid)
{
    FsParams g;
    g.nb = grid->nb; g.ne = grid->ne; g.nab = grid->nab; g.nae = grid->nae;
    g.scale_e = (double)(grid->ne - 1);
    g.he = 1.0 / (double)(grid->ne - 1);
    return g;
}

extern "C" {

// tables [rows][8]; V [T + 1][nb * ne] float64, arg [T][nb * ne] int32.  Actions in ascending index order with fs_better.
int fhc_solve(const float *tables, const shems_foresight_problem *P, const shems_foresight_grid *grid, int T, double *V, int32_t *arg)
{
    const FsParams g = params(grid);
    const int N = g.nb * g.ne, NA = g.nab * g.nae;
    for (int n = 0; n < N; ++n) V[(int64_t)T * N + n] = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        const float *row = tables + ((int64_t)P->cfg.table_row0 + P->idx0 + t - 1) * SHEMS_NCOL, *nx = row + SHEMS_NCOL;
        const double *Vn = V + (int64_t)(t + 1) * N;
        for (int node = 0; node < N; ++node) {
            const int ib = node / g.ne, ie = node - ib * g.ne;
            const EnvIn s{fs_soc_b_node(*P, g.nb, ib), fs_soc_ev_node(g, ie), row[0], row[2], row[3], row[4]};
            double best_v = -__builtin_inf();
            int best_a = kFsNoAction;
            for (int a = 0; a < NA; ++a) {
                const int ab = a / g.nae, ae = a - ab * g.nae;
                const double q = fs_q(P->cfg, s, row[0], nx[0], nx[1], fs_target(ab, g.nab), fs_target(ae, g.nae), Vn, g, P->scale_b);
                if (fs_better(q, a, best_v, best_a)) { best_v = q; best_a = a; }
            }
            V[(int64_t)t * N + node] = best_v;
            arg[(int64_t)t * N + node] = best_a;
        }
    }
    return 0;
}

// the node and target values and the interpolation, for the host restatements of foresight.py
void fhc_nodes(const shems_foresight_problem *P, const shems_foresight_grid *grid, float *soc_b, float *soc_ev, float *b_t, float *ev_t)
{
    const FsParams g = params(grid);
    for (int i = 0; i < g.nb; ++i) soc_b[i] = fs_soc_b_node(*P, g.nb, i);
    for (int j = 0; j < g.ne; ++j) soc_ev[j] = fs_soc_ev_node(g, j);
    for (int a = 0; a < g.nab; ++a) b_t[a] = fs_target(a, g.nab);
    for (int a = 0; a < g.nae; ++a) ev_t[a] = fs_target(a, g.nae);
}

void fhc_value(const double *plane, const shems_foresight_problem *P, const shems_foresight_grid *grid, const float *soc_b, const float *soc_ev,
               int n, double *out)
{
    const FsParams g = params(grid);
    for (int k = 0; k < n; ++k) out[k] = fs_value(plane, g, P->scale_b, soc_b[k], soc_ev[k]);
}

}

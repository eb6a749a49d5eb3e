// shems_foresight_core.h -- the recursion of the perfect-foresight controller, written once (host + device functions).
//
// With the exogenous series known in advance, the best action sequence of the environment AS WRITTEN is a finite-horizon dynamic
// programme over the two continuous state values (Soc_b, Soc_ev); the rest of the state is the table row.  One evaluation
//   Q_t(state, a) = reward of step!(state, a) + V_{t+1}(Soc_b', Soc_ev')
// runs the env's own arithmetic: action(env, a::ShemsAction) (shems_LU1.jl:283-316), step! (:343-485), the arrival overwrite of
// next_state! (:264-281); there is no discount -- a pass is scored by the plain sum of its rewards (memory_plotting_saving.jl:62-89).
// V lives on an NB x NE grid of nodes and is read off the nodes by bilinear interpolation in float64 with ONE fixed order of operations
// (IEEE add / sub / mul / compare / floor only), so that the device, a host build of this header and a NumPy restatement agree bit for
// bit.  The maximum over the action grid is the SMALLEST index among equal maxima (fs_better), whatever the shape of the reduction.
//
// MUST be compiled with -ffp-contract=off, as shems_core.h.
#pragma once

#include "shems_core.h"

#pragma clang fp contract(off)

namespace shems {

struct FsParams {               // the grid as a kernel needs it; the two float64 scalars are formed on the host
    int    nb, ne, nab, nae;
    double scale_e;             // NE - 1
    double he;                  // 1.0 / (NE - 1)
};

// State nodes: Soc_b[i] = (float)(i * hb), hb = (double)soc_max / (NB - 1); Soc_ev[j] = (float)(j * he); the end nodes are exactly
// soc_max and 1.
SHEMS_HD float fs_soc_b_node(const shems_foresight_problem &p, int nb, int i)
{
    return i == nb - 1 ? p.cfg.soc_max : (float)((double)i * p.hb);
}
SHEMS_HD float fs_soc_ev_node(const FsParams &g, int j) { return j == g.ne - 1 ? 1.0f : (float)((double)j * g.he); }
// Action targets: (float)(a / (double)(n - 1)); the single point of a 1-point axis is 1.
SHEMS_HD float fs_target(int a, int n) { return n == 1 ? 1.0f : (float)((double)a / (double)(n - 1)); }

// One axis of the interpolation: u = x * scale, i = clamp((int)floor(u), 0, n - 2), f = clamp(u - i, 0, 1).
SHEMS_HD void fs_axis(double x, double scale, int n, int &i, double &f)
{
    const double u = x * scale;
    double fl = __builtin_floor(u);
    fl = !(fl > 0.0) ? 0.0 : (fl > (double)(n - 2) ? (double)(n - 2) : fl);      // also catches a NaN
    i = (int)fl;
    const double fr = u - fl;
    f = !(fr > 0.0) ? 0.0 : (fr > 1.0 ? 1.0 : fr);
}

// V off the nodes.  V: one plane [nb][ne] float64 (any address space the caller can read).
SHEMS_HD double fs_value(const double *V, const FsParams &g, double scale_b, float soc_b, float soc_ev)
{
    int ib, ie;
    double fb, fe;
    fs_axis((double)soc_b, scale_b, g.nb, ib, fb);
    fs_axis((double)soc_ev, g.scale_e, g.ne, ie, fe);
    const double *r0 = V + (int64_t)ib * g.ne + ie, *r1 = r0 + g.ne;
    const double V00 = r0[0], V01 = r0[1], V10 = r1[0], V11 = r1[1];
    return (1.0 - fe) * ((1.0 - fb) * V00 + fb * V10) + fe * ((1.0 - fb) * V01 + fb * V11);
}

// Q_t(state, (B_target, EV_target)): the DRL step of the env (penalty kept) from `s`, the arrival overwrite with h_countdown of the
// current row and (h_countdown, soc_ev) of the next one, plus V_{t+1} at the state it leaves.
SHEMS_HD double fs_q(const shems_config &c, const EnvIn &s, float h_cur, float h_next, float soc_ev_next, float B_target, float EV_target,
                     const double *V_next, const FsParams &g, double scale_b)
{
    float B, EV, soc_b_n, soc_ev_n;
    double reward;
    StepFlows f;
    action_drl(c, s, B_target, EV_target, B, EV);
    step_flows(c, s, EV_target, B, EV, false, soc_b_n, soc_ev_n, reward, f);
    if (h_next >= 0.0f && h_cur == -1.0f) soc_ev_n = soc_ev_next;                  // LU1:270-272
    return reward + fs_value(V_next, g, scale_b, soc_b_n, soc_ev_n);
}

// (value, index) order of the maximum: greater value, or equal value and smaller index.
SHEMS_HD bool fs_better(double v, int a, double best_v, int best_a) { return v > best_v || (v == best_v && a < best_a); }

constexpr int kFsNoAction = 0x7fffffff;          // the index of "nothing evaluated yet": loses every tie

// ---- the receding-horizon schedule (shems_foresight_solve_horizon_dev; foresight.horizon_plan restates it) ----
// The deployable controller sees a limited forecast.  Two integers are shared by all problems of a call:
//   horizon H >= 1         hours of forecast, the current hour included;
//   control c, 1 <= c <= H a fresh plan every c hours.
// For decision hour t (0-based) of a T-hour pass the plan in force was made at j = t - t mod c; it sees hours j .. hi - 1 with
// hi = min(j + H, T); the controller takes the first maximum over the action grid of reward_t + U_{t+1}(state'), where U_{t+1} is the
// optimal value of hours t + 1 .. hi - 1 with terminal value 0: the plane V[0] of the ordinary backward sweep on the window
// (idx0 + t + 1, nsteps = hi - (t + 1)), the zero plane when that length is 0.  The planes are laid out as the ordinary sweep's, so
// the forward pass reads them unchanged: V[p][t] = U_t for t = 1 .. T (what the forward pass reads at hour t - 1), V[p][T] = 0,
// V[p][0] = the value of the first plan at hour 0; argmax[p][t][node] = the action the controller takes at hour t from that node.
// Window j (the plans are made at j = 0, c, 2c, ...) therefore sweeps hours hi - 1 down to j + 1 -- and hour j itself where its
// arg-max or V[p][0] is wanted --, and of those it keeps planes j + 1 .. min(j + c, T) and arg-max j .. min(j + c, T) - 1.
// All arguments are taken as validated (T >= 1, 1 <= c <= H, 0 <= j < T); no sum here can overflow an int.
SHEMS_HD int fs_plan_windows(int T, int c) { return (T - 1) / c + 1; }                        // ceil(T / c)
SHEMS_HD int fs_plan_of_hour(int t, int c) { return t - t % c; }                              // j: the hour the plan in force at t was made
SHEMS_HD int fs_plan_end(int j, int H, int T) { return H < T - j ? j + H : T; }               // hi: the plan sees hours j .. hi - 1
SHEMS_HD int fs_plan_keep(int j, int c, int T) { return c < T - j ? j + c : T; }              // the last hour window j answers for, + 1
SHEMS_HD int fs_plan_first(int j, bool want_argmax) { return (want_argmax || j == 0) ? j : j + 1; }   // the earliest hour window j sweeps
// Where window j's results go: the plane of hour t (a swept hour, or hi with its zeros) into V[p][t], the arg-max of a swept hour t
// into argmax[p][t].
SHEMS_HD bool fs_plan_keeps_plane(int j, int c, int T, int t) { return t == 0 || (t > j && t <= fs_plan_keep(j, c, T)); }
SHEMS_HD bool fs_plan_keeps_argmax(int j, int c, int T, int t) { return t >= j && t < fs_plan_keep(j, c, T); }

// ---- planning on a forecast (shems_foresight_solve_forecast_dev / _track_forecast_dev; foresight.belief_offset restates it) ----
// The schedule above plans on the TRUE future rows, which no deployable controller has.  A problem may name a FORECAST TABLE: same nrow,
// in the same uploaded row array [total_rows][8], addressed by a row offset forecast_off -- the forecast of table row r is array row
// table_row0 + forecast_off + r.  forecast_off = 0: the truth is the forecast; the offset is negative when the forecast table lies
// before the truth in the array.  One table cannot express a forecast that depends on when it was issued.
// Belief of the plan made at hour j (j = t - t mod c as above): the row of hour u (table row idx0 + u) is the TRUE row for u <= j and
// the FORECAST row for u > j.  Everything the schedule defines (hi, U_t, which planes and arg-max are kept, V[p][0], the zero plane at
// hi) holds unchanged on that belief: a sweep of hour t inside window j takes its current row from the truth if t == j and from the
// forecast otherwise, and its next row always from the forecast; the sweep of hour hi - 1 = T - 1 reads forecast row idx0 + T, which
// exists because the forecast table has nrow rows.  argmax[p][t] for t > j is what the plan made at j INTENDS for hour t under its
// forecast; the forward pass decides again from what it observes.
// Forward pass: at hour t the controller observes the true state and the true row t (h_cur is the truth's), but not yet row t + 1, so
// the arrival overwrite inside Q (LU1:264-281) takes h_countdown and soc_ev of the next row from the FORECAST row t + 1; the env is
// then stepped on the truth by the ordinary DRL step.
// With forecast_off = 0, or a forecast table that is a byte copy of the truth, every plane, index and forward choice equals the
// schedule's on the truth bit for bit.
// fs_belief_off: the offset (in rows, added to table_row0) of the row of hour u in the plan made at hour j.  The forward pass at hour
// t is the case (u, j) = (t, t) for its current row and (t + 1, t) for its next.
SHEMS_HD int fs_belief_off(int u, int j, int forecast_off) { return u > j ? forecast_off : 0; }

// ---- the audit of a tracked pass (shems_foresight_audit_dev; tests/foresight_regret_ref.py restates it) ----
// Where does a pass lose against V?  Given the planes V[p][0 .. T] of a solve call on the TRUE rows and the reference's 23-column result
// rows of ANY pass over the same T hours (write_results, csrc/shems_env_dev.h: the rule-based controller's, an actor's, a foresight
// pass's, rows read back from a results file), every (pass, hour) gets three float64 and one index; nothing of the controller is needed.
// For pass e of problem p at hour t (0-based), r = results[e][t], P = the problem record:
//   row        idx = (int)r[0] - 1 (column 0 holds the row index AFTER the step); it must equal P.idx0 + t, and rows idx, idx + 1 must
//              lie inside the row array: otherwise the hour is refused (three NaN, action -1, status[e] = SHEMS_ERR_INDEX);
//   state      EnvIn{(float)r[22], (float)r[4], (float)r[1], d_e, g_e, p_buy}, the last three from columns 2, 3, 4 of table row idx --
//              what reset! and next_state! leave in the observation.  The three floats were stored as doubles: the way back is exact;
//   next row   h_cur, h_next, soc_ev_next from table rows idx and idx + 1, exactly as the forward pass takes them;
//   best_q, best_a  the first maximum (fs_better) over a = ab * nae + ae of fs_q(P.cfg, state, ..., fs_target(ab), fs_target(ae), V[p][t + 1]);
//   achieved_q      r[5] + fs_value(V[p][t + 1], Soc_b, Soc_ev of results[e][t + 1]) for t < T - 1.  At t = T - 1 it is r[5] + 0.0: the
//                   rows do not hold the pass's FINAL state, and V_T = 0 in everything a solve call leaves;
//   v_state         fs_value(V[p][t], Soc_b, Soc_ev of r).
// On the host: regret = best_q - achieved_q, discretisation = best_q - v_state.  For the planes of shems_foresight_solve_dev
//   sum_t regret_t = best_q[0] - sum_t r[5] + sum_{t >= 1} discretisation_t
// up to float64 rounding: achieved_q[t] = reward_t + v_state[t + 1] for t < T - 1, so the sum telescopes.
// Regret is NOT a bound: a controller acting off the action grid -- an actor, or the rule-based controller, whose rows carry kWh
// set-points -- can reach slightly negative values.  For the planes of shems_foresight_solve_horizon_dev best_q is what THAT controller
// would take from this state, and the identity does not apply.  An audit against a belief (planes solved on a forecast table) is not
// defined; foresight.audit refuses it.
struct FsAuditHour {
    EnvIn s;
    float h_cur, h_next, soc_ev_next;
};

// The row check and the state of hour t.  `tables`: the row array [total_rows][8].  False: the hour is refused.
SHEMS_HD bool fs_audit_hour(const shems_foresight_problem &P, const float *tables, int64_t total_rows, const double *r, int t, FsAuditHour &h)
{
    const double x = r[0];
    if (!(x >= 1.0 && x <= 2147483647.0)) return false;                           // also a NaN: the conversion below is then defined
    const int idx = (int)x - 1;
    if (idx < 1 || (int64_t)idx != (int64_t)P.idx0 + t) return false;
    const int64_t at = (int64_t)P.cfg.table_row0 + idx - 1;                         // array row of table row idx
    if (P.cfg.table_row0 < 0 || idx + 1 > P.cfg.nrow || at + 2 > total_rows) return false;
    const float *row = tables + at * SHEMS_NCOL;
    h.s = EnvIn{(float)r[22], (float)r[4], (float)r[1], row[2], row[3], row[4]};
    h.h_cur = row[0];
    h.h_next = row[SHEMS_NCOL];
    h.soc_ev_next = row[SHEMS_NCOL + 1];
    return true;
}

// Q of action index a from the state of the hour; V_next = V[p][t + 1].
SHEMS_HD double fs_audit_q(const shems_foresight_problem &P, const FsAuditHour &h, int a, const double *V_next, const FsParams &g)
{
    const int ab = a / g.nae, ae = a - ab * g.nae;
    return fs_q(P.cfg, h.s, h.h_cur, h.h_next, h.soc_ev_next, fs_target(ab, g.nab), fs_target(ae, g.nae), V_next, g, P.scale_b);
}

// r_next = results[e][t + 1], or null at t = T - 1.
SHEMS_HD double fs_audit_achieved(const shems_foresight_problem &P, const double *r, const double *r_next, const double *V_next, const FsParams &g)
{
    return r[5] + (r_next ? fs_value(V_next, g, P.scale_b, (float)r_next[22], (float)r_next[4]) : 0.0);
}

// V_cur = V[p][t].
SHEMS_HD double fs_audit_v_state(const shems_foresight_problem &P, const FsAuditHour &h, const double *V_cur, const FsParams &g)
{
    return fs_value(V_cur, g, P.scale_b, h.s.Soc_b, h.s.Soc_ev);
}

// ---- demonstrations from tracked passes (shems_foresight_demos_dev; tests/imitation_ref.py restates it) ----
// What a 9-input actor would have to answer at the states a pass was in: every (pass, hour) becomes one (observation, action) pair.
//   observation  s[0..5] = the EnvIn of fs_audit_hour (same row check, same way back from the float64 columns), s[6..8] = columns
//                5, 6, 7 of table row idx (h_cos, h_sin, season), as reset! / next_state! leave them (csrc/shems_env_dev.h): the nine
//                floats shems_get_state shows before the step that wrote the row;
//   label        a = (float)(2.0 * (double)target - 1.0) per axis, the inverse of scale_action (exact for dyadic targets k/2, k/4, ...;
//                within one float32 rounding otherwise), so that labels at targets 0 and 1 are exactly -1 and +1.  The target is given
//                (what shems_foresight_track_dev wrote), or it is (fs_target(ab, nab), fs_target(ae, nae)) of an action index
//                a = ab * nae + ae (what the audit wrote): the DAgger label at a state ANOTHER controller visited.
// An hour whose row check fails, or whose index label is outside 0 .. nab * nae - 1 (the audit's -1), gives no pair.
struct FsDemo {
    float s[SHEMS_NSTATE];
    float a[2];
};

SHEMS_HD float fs_demo_label(float target) { return (float)(2.0 * (double)target - 1.0); }

// target: the two targets of the hour, or null: `action` is an index into the action grid.  False: the hour gives no pair.
SHEMS_HD bool fs_demo_hour(const shems_foresight_problem &P, const float *tables, int64_t total_rows, const double *r, int t,
                           const float *target, int action, const FsParams &g, FsDemo &d)
{
    FsAuditHour h;
    if (!fs_audit_hour(P, tables, total_rows, r, t, h)) return false;
    float tb, te;
    if (target) {
        tb = target[0]; te = target[1];
    } else {
        if (action < 0 || action >= g.nab * g.nae) return false;
        const int ab = action / g.nae, ae = action - ab * g.nae;
        tb = fs_target(ab, g.nab); te = fs_target(ae, g.nae);
    }
    const float *row = tables + ((int64_t)P.cfg.table_row0 + ((int64_t)P.idx0 + t) - 1) * SHEMS_NCOL;      // table row idx: checked above
    d.s[0] = h.s.Soc_b; d.s[1] = h.s.Soc_ev; d.s[2] = h.s.c_ev; d.s[3] = h.s.d_e; d.s[4] = h.s.g_e; d.s[5] = h.s.p_buy;
    d.s[6] = row[5]; d.s[7] = row[6]; d.s[8] = row[7];
    d.a[0] = fs_demo_label(tb); d.a[1] = fs_demo_label(te);
    return true;
}

// The ring slot of (pass e, hour t) when the first pair goes to slot `pos`: passes one after the other, wrapping.
SHEMS_HD int64_t fs_demo_slot(int64_t pos, int64_t e, int T, int t, int64_t capacity) { return (pos + e * T + t) % capacity; }

// What the entry point refuses of the ring before anything is launched (0: accepted).
SHEMS_HD int fs_demo_check_ring(int64_t capacity, int64_t pos, int64_t n_pass, int64_t T)
{
    if (capacity < 1) return 1;
    if (n_pass * T > capacity) return 2;
    if (pos < 0 || pos >= capacity) return 3;
    return 0;
}

// ---- transitions from tracked passes (shems_foresight_transitions_dev; tests/warmstart_ref.py restates it) ----
// The rows of a DRL-mode pass hold everything a replay slot holds: every (pass, hour) with a successor becomes (s, a, r, s', done).
//   s, s2   the observations of fs_demo_hour for rows t and t + 1: the `pre` state of the next row IS the state after this step;
//   a       (fs_demo_label((float)r[21]), fs_demo_label((float)r[2])): columns 21 (B_target) and 2 (EV_target) hold the two targets
//           after scale_action (write_results, csrc/shems_env_dev.h).  Rows of a RULE-BASED pass record targets 0 and kWh set-points
//           there: they would give wrong actions, and nothing here can tell them apart;
//   rew     (float)r[5], as the fused step converts the reward before ring_push.
// The hour is refused if the row check of hour t or of hour t + 1 fails, or r[5] is not finite.
// Return-to-go of a pass, float64, sequentially from the end, g = (double)gamma:
//   G[T - 1] = r[T - 1][5];   G[t] = r[t][5] + g * G[t + 1]      (the product rounded, then the sum: fs_return_step)
// This order is the definition.  Env and tracked policy are deterministic, so G[t] is the exact Q^pi(s_t, a_t) of the controller that
// made the pass -- up to the hours the end of the pass cuts off, which is what `tail` is for.
//   SHEMS_FS_TRANS_TD   the slot holds (s, a, rew, s2, done = 0): the bytes the reference's `remember` would store;
//   SHEMS_FS_TRANS_MC   the slot holds (s, a, (float)G[t], s2, done = 1): the update forms y = r + gamma (1 - done) q' = G[t] exactly.
// tail (1 <= tail < T): hours t >= T - tail give no transition; G still sums over all T hours.  (pass e, hour t) goes to slot
// fs_demo_slot(pos, e, T - tail, t, capacity).  TD: a refused hour leaves its slot alone, the rest of the pass is written.  MC: a pass
// ANY of whose T hours fails its row check or has a non-finite reward gives no transition at all (fs_returns_hour_ok) and its row of
// returns is fs_returns_refused() in every hour.  That NaN in G[e][0] is also the per-pass verdict the transitions kernel reads: an
// accepted pass cannot produce one (its rewards are finite; with g > 0 an overflow gives an infinity, which r + g * inf keeps, and
// with g = 0 nothing is carried).
struct FsTransition {
    FsDemo d;                        // s and a
    float s2[SHEMS_NSTATE];
    float rew;
};

SHEMS_HD bool fs_finite(double x) { return x - x == 0.0; }

SHEMS_HD bool fs_transition_hour(const shems_foresight_problem &P, const float *tables, int64_t total_rows, const double *r, int t,
                                 FsTransition &x)
{
    const float target[2] = {(float)r[21], (float)r[2]};
    const FsParams none{};                                                          // targets are given: the action grid is not read
    FsDemo next;
    if (!fs_demo_hour(P, tables, total_rows, r, t, target, -1, none, x.d)) return false;
    if (!fs_demo_hour(P, tables, total_rows, r + SHEMS_NRESULT, t + 1, target, -1, none, next)) return false;
    if (!fs_finite(r[5])) return false;
    for (int k = 0; k < SHEMS_NSTATE; ++k) x.s2[k] = next.s[k];
    x.rew = (float)r[5];
    return true;
}

// What the returns of a pass need of EVERY hour (MC's verdict).
SHEMS_HD bool fs_returns_hour_ok(const shems_foresight_problem &P, const float *tables, int64_t total_rows, const double *r, int t)
{
    FsAuditHour h;
    return fs_audit_hour(P, tables, total_rows, r, t, h) && fs_finite(r[5]);
}

SHEMS_HD double fs_return_step(double reward, double g, double G_next)
{
    const double carried = g * G_next;
    return reward + carried;
}

SHEMS_HD double fs_returns_refused() { return __builtin_nan(""); }

// The returns of one pass, serially (a host build; the device spreads the row checks over a wave and keeps this chain).  res: the T
// rows of the pass, G: T float64 out.  False: the pass is refused and G holds fs_returns_refused().
SHEMS_HD bool fs_returns(const shems_foresight_problem &P, const float *tables, int64_t total_rows, const double *res, int T, float gamma,
                         double *G)
{
    const double g = (double)gamma;
    bool ok = true;
    for (int t = T - 1; t >= 0; --t) {
        const double *r = res + (int64_t)t * SHEMS_NRESULT;
        ok = fs_returns_hour_ok(P, tables, total_rows, r, t) && ok;
        G[t] = t == T - 1 ? r[5] : fs_return_step(r[5], g, G[t + 1]);
    }
    if (!ok)
        for (int t = 0; t < T; ++t) G[t] = fs_returns_refused();
    return ok;
}

// ---- hedging over a forecast ENSEMBLE (shems_foresight_track_ensemble_dev; tests/foresight_ensemble_ref.py restates it) ----
// The forecast controller above treats its one table as certain.  An ensemble problem is ONE truth (cfg, idx0) with K scenarios,
// 1 <= K <= kFsMaxScen: scenario k is a forecast table in the sense above (forecast_off[k], same nrow, same row array) with a float64
// weight w[k], finite and > 0.  The host layer normalises the weights to sum 1; nothing here renormalises.
// Planner: for each scenario k the planes are exactly the forecast controller's on the belief "truth up to j, scenario k after":
// U^k_t is what shems_foresight_solve_forecast_dev leaves in record p * K + k (problem-major, scenario-minor); no new sweep.
// Controller: at hour t it observes the true state and the true row t.  For action a the DRL step is taken ONCE (fs_step): its reward
// and (Soc_b', Soc_ev') do not depend on the scenario.  Then
//   acc = +0.0
//   for k = 0 .. K - 1, in this order:
//       Soc_ev'^k = h_next^k >= 0 && h_cur == -1 ? soc_ev_next^k : Soc_ev'               (LU1:270-272, scenario k's row t + 1)
//       acc = acc + w[k] * fs_value(V[p * K + k][t + 1], Soc_b', Soc_ev'^k)
//   Qbar = reward + acc
// with (h_next^k, soc_ev_next^k) from scenario k's row t + 1 -- fs_belief_off(t + 1, t, forecast_off[k]) -- and h_cur the truth's.
// The first maximum (fs_better) over a = ab * nae + ae wins, and the env is stepped on the truth by the ordinary DRL step.  The sum
// over k is in THIS order whatever spreads the work, so that the device, a host build and a NumPy restatement agree bit for bit.
// This is the two-stage scenario programme: the first decision is common, and after it each scenario is optimised with its OWN
// foresight.  It is therefore OPTIMISTIC about what is learnt after the first stage -- it values hour t + 1 onwards as if the
// controller then knew which scenario holds -- and nothing says an ensemble does better than one of its members.
// K = 1, w = 1.0: 0.0 + 1.0 * v = v, so every choice equals the forecast controller's on that record; the same for one scenario
// twice at w = (0.5, 0.5), since 0.5 v + 0.5 v is exact.  Three copies at (0.5, 0.25, 0.25) need not: 0.75 v rounds.
constexpr int kFsMaxScen = 16;

struct FsStep {                 // what the DRL step of one action leaves, before any arrival overwrite
    double reward;
    float  soc_b, soc_ev;
};

SHEMS_HD FsStep fs_step(const shems_config &c, const EnvIn &s, float B_target, float EV_target)
{
    float B, EV;
    FsStep o;
    StepFlows f;
    action_drl(c, s, B_target, EV_target, B, EV);
    step_flows(c, s, EV_target, B, EV, false, o.soc_b, o.soc_ev, o.reward, f);
    return o;
}

// Qbar of one action.  w, h_next, soc_ev_next: K entries each, in scenario order (any address space the caller can read); V_next: the
// plane [t + 1] of scenario 0, the plane of scenario k lies v_stride float64 further per scenario ((T + 1) * nb * ne in what
// solve_forecast_dev leaves).
SHEMS_HD double fs_q_ens(const FsStep &st, float h_cur, int K, const double *w, const float *h_next, const float *soc_ev_next,
                         const double *V_next, int64_t v_stride, const FsParams &g, double scale_b)
{
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
        const float soc_ev_n = (h_next[k] >= 0.0f && h_cur == -1.0f) ? soc_ev_next[k] : st.soc_ev;
        acc = acc + w[k] * fs_value(V_next + (int64_t)k * v_stride, g, scale_b, st.soc_b, soc_ev_n);
    }
    return st.reward + acc;
}

}  // namespace shems

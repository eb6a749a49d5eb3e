"""Shared by the ensemble tests: the receding-horizon controller that hedges over K forecast scenarios, from the definition, on the C
oracle (NOT from the package or the header).

Scenario k of a problem is a forecast table -- ("truth",), a byte copy, or (lag, kind), persistence of the columns `kind` of
foresight_forecast_ref.COLS written row by row -- with a float64 weight w[k].  The plan made at hour j under scenario k believes the
COMPOSITE table (true rows up to table row idx0 + j, scenario k's rows after it), and its planes are the receding-horizon planes on
that table: V^k[t + 1] = plane 0 of foresight_twin.twin_solve on the composite's window (idx0 + t + 1, hi - (t + 1)), zeros when that
length is 0.  At hour t the controller steps every candidate action from the true state ONCE PER SCENARIO on that scenario's belief
of hour t (the current row is the truth's in every belief, so the rewards agree bit for bit -- asserted; the next row, which carries
the arrival overwrite, is the scenario's), and takes the first maximum of
    reward + ((((+0.0 + w[0] v_0) + w[1] v_1) + ...) + w[K-1] v_{K-1}),     v_k = interp(V^k[t + 1], state'_k),
the sum in scenario order.  The env is then stepped on the truth.  Every twin window is solved once per process and shared; callers
must not modify what they get.
"""
from __future__ import annotations

import functools

import numpy as np

import foresight_forecast_ref as FC
import foresight_horizon_ref as FR
import foresight_twin as FT
import util as U
from util import oracle_c

TRUTH = ("truth",)


@functools.lru_cache(maxsize=None)
def scenario(which, p, spec):
    """The scenario table of problem p: spec = TRUTH (a byte copy) or (lag, kind)."""
    tab = FR._problem(which, p)[0]
    if spec == TRUTH:
        return np.array(tab, np.float32, copy=True)
    lag, kind = spec
    return FC.persistence(tab, lag, FC.COLS[kind])


@functools.lru_cache(maxsize=None)
def composite(which, p, spec, j):
    """What the plan made at hour j believes under the scenario: true rows up to table row idx0 + j (1-based), scenario rows after."""
    tab, _, idx0, _ = FR._problem(which, p)
    out = np.array(scenario(which, p, spec), np.float32, copy=True)
    out[:idx0 + j] = tab[:idx0 + j]
    return out


@functools.lru_cache(maxsize=None)
def twin_plane(which, p, spec, j, t, k):
    """V[0] of the twin on the k >= 1 hours that start at hour t, on the belief of the plan made at j under the scenario."""
    _, prof, idx0, shape = FR._problem(which, p)
    V, _ = FT.twin_solve(composite(which, p, spec, j), prof, idx0 + t, k, shape["nb"], shape["ne"], shape["nab"], shape["nae"])
    return V[0]


@functools.lru_cache(maxsize=None)
def planes(which, p, spec, H, c):
    """V [T + 1][N] float64 of problem p under (H, c) and one scenario: what the forecast solve leaves in that scenario's record."""
    shape = FR._problem(which, p)[3]
    T, N = shape["T"], shape["nb"] * shape["ne"]
    j, k = FR.brute_plan(T, H, c)
    V = np.zeros((T + 1, N))
    V[0] = twin_plane(which, p, spec, 0, 0, int(k[0]) + 1)
    for t in range(T):
        if k[t] > 0:
            V[t + 1] = twin_plane(which, p, spec, int(j[t]), t + 1, int(k[t]))
    return V


def crafted_planes(which, p):
    """The construction that pins the source of the next row: every plane t <= T - 1 is 10 Soc_b[node] where the node's Soc_ev < 0.75
    and -10 Soc_b[node] elsewhere, V[T] = 0."""
    _, prof, _, sh = FR._problem(which, p)
    sb, se = np.repeat(FT.nodes(sh["nb"], prof.soc_max), sh["ne"]), np.tile(FT.nodes(sh["ne"], 1.0), sh["nb"])
    plane = np.where(se < np.float32(0.75), 10.0 * sb.astype(np.float64), -10.0 * sb.astype(np.float64))
    out = np.tile(plane, (sh["T"] + 1, 1))
    out[sh["T"]] = 0.0
    return out


def controller(which, p, specs, w, V, soc_b, tg=None, res=None, next_from="own", actions=None):
    """The ensemble controller of problem p from the start states Soc_b = soc_b [n] on row idx0.  specs: the K scenarios; w: their K
    float64 weights, used as given; V: K arrays [T + 1][N], scenario k's planes.  tg None: the controller runs on its own choices;
    tg [n][T][2]: the trajectory follows those targets instead (a device's), and every choice is what the controller would take from
    the state the trajectory is in; with res [n][T][23] the replayed rewards and rows are compared bitwise.  next_from: "own" (the
    definition: scenario k's candidates are stepped on scenario k's belief), "first" / "last" (every scenario's candidates on the
    belief of scenario 0 / K - 1: what a kernel that reads one next row for all scenarios would do).  actions: (nab, nae) of another
    action grid than the problem's own.
    Returns a dict: picks [n][T][2] float32, q [n][T][A] float64 (Qbar of every action), totals [n] (the ordered float64 sum of the
    rewards), obs [n][T][9] (the state before each hour), ref (the oracle batch after the pass)."""
    tab, prof, idx0, sh = FR._problem(which, p)
    if actions is not None:
        sh = dict(sh, nab=actions[0], nae=actions[1])
    T, K = sh["T"], len(specs)
    assert len(w) == K and len(V) == K
    w = [float(x) for x in w]
    soc = np.asarray(soc_b, np.float32)
    n = len(soc)
    idx = np.full(n, idx0, np.int32)
    acts = FT.action_grid(sh["nab"], sh["nae"])
    A = len(acts)
    ref = oracle_c.Batch(n, T, tab, prof)
    ref.set_state(U.obs_of_rows(tab, idx, soc), idx.astype(np.int64), np.zeros(n, np.int64))
    a_all = np.ascontiguousarray(np.tile(acts, (n, 1)))
    totals = np.zeros(n)
    picks = np.zeros((n, T, 2), np.float32)
    qs = np.zeros((n, T, A))
    obs = np.zeros((n, T, 9), np.float32)
    for t in range(T):
        obs[:, t] = ref.state()
        acc = np.zeros(n * A)                                               # +0.0
        reward = None
        for k in range(K):
            spec = specs[k] if next_from == "own" else specs[0] if next_from == "first" else specs[-1]
            cand = oracle_c.Batch(n * A, T, composite(which, p, spec, t), prof)
            cand.set_state(np.repeat(ref.state(), A, axis=0), np.repeat(ref.idx(), A))
            rc, r, o2, _ = cand.step(a_all, 0)
            assert rc == 0
            if reward is None:
                reward = r
            assert (U.bits64(r) == U.bits64(reward)).all()                  # the step does not depend on the scenario
            acc = acc + w[k] * FT.interp(V[k][t + 1], sh["nb"], sh["ne"], prof.soc_max, o2[:, 0], o2[:, 1])
        q = (reward + acc).reshape(n, A)
        qs[:, t] = q
        picks[:, t] = acts[np.argmax(q, axis=1)]                            # the first maximum
        rc, r, _, rr = ref.step(picks[:, t] if tg is None else tg[:, t], 1, want_results=True)
        assert rc == 0
        if res is not None:
            assert (U.bits64(r) == U.bits64(res[:, t, 5])).all(), t
            assert (U.bits64(rr) == U.bits64(res[:, t])).all(), t
        totals = totals + r
    return dict(picks=picks, q=qs, totals=totals, obs=obs, ref=ref)


@functools.lru_cache(maxsize=None)
def s1_run(specs, w, H, c):
    """The free-running controller on S1 from Soc_b = 0.5 soc_max, shared: (specs, w) tuples."""
    prof = FR._problem("s1", 0)[1]
    V = [planes("s1", 0, s, H, c) for s in specs]
    return controller("s1", 0, specs, w, V, [np.float32(0.5 * float(prof.soc_max))])

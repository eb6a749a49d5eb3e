"""Shared by the foresight tests: the shapes the issue names and a float64 NumPy twin of the recursion on the C oracle.

The twin puts one oracle env per (node, action) through oracle_c.Batch.set_state / step, interpolates V_{t+1} with the formula of
csrc/shems_foresight_core.h restated here (NOT imported from the package), and takes the first maximum.  Every result is computed
once per process and shared (functools.lru_cache); callers must not modify what they get.
"""
from __future__ import annotations

import functools
import importlib

import numpy as np

import util as U
from util import oracle_c


def F():
    return importlib.import_module(U.PKG_NAME + ".foresight")


# ------------------------------------------------------------------ the twin --
def nodes(n, top):
    """(float)(i * h), h = (double)top / (n - 1); the last node is `top` itself."""
    h = float(np.float32(top)) / (n - 1)
    x = np.array([np.float32(i * h) for i in range(n)], np.float32)
    x[-1] = np.float32(top)
    return x


def targets(n):
    return np.array([1.0] if n == 1 else [np.float32(a / float(n - 1)) for a in range(n)], np.float32)


def action_grid(nab, nae):
    return np.stack([np.repeat(targets(nab), nae), np.tile(targets(nae), nab)], 1).astype(np.float32)


def interp(plane, nb, ne, soc_max, x_b, x_e):
    V = np.asarray(plane, np.float64).reshape(nb, ne)

    def axis(x, scale, n):
        u = np.asarray(x, np.float32).astype(np.float64) * scale
        i = np.clip(np.floor(u), 0, n - 2)
        return i.astype(np.int64), np.clip(u - i, 0.0, 1.0)

    ib, fb = axis(x_b, (nb - 1) / float(np.float32(soc_max)), nb)
    ie, fe = axis(x_e, float(ne - 1), ne)
    V00, V10, V01, V11 = V[ib, ie], V[ib + 1, ie], V[ib, ie + 1], V[ib + 1, ie + 1]
    return (1.0 - fe) * ((1.0 - fb) * V00 + fb * V10) + fe * ((1.0 - fb) * V01 + fb * V11)


def twin_solve(tab, prof, idx0, T, nb, ne, nab, nae):
    """V [T + 1][nb * ne] float64 and arg-max [T][nb * ne] of one problem, by the oracle."""
    N, acts = nb * ne, action_grid(nab, nae)
    A = len(acts)
    sb, se = np.repeat(nodes(nb, prof.soc_max), ne), np.tile(nodes(ne, 1.0), nb)       # node index = ib * ne + ie
    ref = oracle_c.Batch(N * A, T, tab, prof)
    a_all = np.ascontiguousarray(np.tile(acts, (N, 1)))
    V = np.zeros((T + 1, N), np.float64)
    arg = np.zeros((T, N), np.int32)
    for t in range(T - 1, -1, -1):
        obs = U.obs_of_rows(tab, np.full(N, idx0 + t), sb)
        obs[:, 1] = se
        ref.set_state(np.repeat(obs, A, axis=0), np.full(N * A, idx0 + t, np.int64))
        rc, r, o2, _ = ref.step(a_all, 0)
        assert rc == 0
        q = (r + interp(V[t + 1], nb, ne, prof.soc_max, o2[:, 0], o2[:, 1])).reshape(N, A)
        arg[t] = np.argmax(q, axis=1)                    # the first maximum
        V[t] = q[np.arange(N), arg[t]]
    return V, arg


# ---------------------------------------------------------------- the shapes --
def window_features(tab, idx0, T):
    """What rows idx0 .. idx0 + T of a table hold for T hours: (arrival, an h == 0 row, a g_e > d_e row, a g_e <= d_e row)."""
    h = tab[idx0 - 1:idx0 + T, 0]
    cur = tab[idx0 - 1:idx0 + T - 1]
    return (bool(((h[:-1] == -1) & (h[1:] >= 0)).any()), bool((cur[:, 0] == 0).any()), bool((cur[:, 3] > cur[:, 2]).any()),
            bool((cur[:, 3] <= cur[:, 2]).any()))


def first_window(tab, T, start=1):
    for idx0 in range(start, tab.shape[0] - T + 1):
        if all(window_features(tab, idx0, T)):
            return idx0
    raise AssertionError("the table holds no window with an arrival, a departure, a PV surplus and a PV shortfall")


S1 = dict(T=30, nb=9, ne=5, nab=5, nae=3)
S2 = dict(T=8, nb=33, ne=9, nab=4, nae=7)
# The first three are the cases the issue names.  The window of row 97 of Charger 5 holds no EV session on the table as it is, which
# leaves disc_weight / disc_pot inert there, so a fourth problem puts the same weights on the window of row 106, which holds an
# arrival and a departure.
S2_PROBLEMS = ((98, "eval", 9, {}), (5, "eval", 97, dict(disc_weight=0.1, disc_pot=1.0)), (1, "test", 127, dict(penalty_weight=0.2)),
               (5, "eval", 106, dict(disc_weight=0.1, disc_pot=1.0)))


@functools.lru_cache(maxsize=None)
def s1():
    """Charger98 eval table, the first window of 30 hours with an arrival, a departure, a PV surplus and a PV shortfall (row 1 today)."""
    T = U.tables_mod()
    tab = T.profile_table(98, "eval")
    idx0 = first_window(tab, S1["T"])
    V, arg = twin_solve(tab, oracle_c.profile(98), idx0, **S1)
    return dict(tab=tab, idx0=idx0, V=V, arg=arg, prof=oracle_c.profile(98))


@functools.lru_cache(maxsize=None)
def s2():
    """Four problems with different tables, start rows, capacities and reward weights in one call."""
    T = U.tables_mod()
    tabs, profs, V, arg = [], [], [], []
    for cid, split, idx0, w in S2_PROBLEMS:
        tab = T.profile_table(cid, split)
        prof = oracle_c.profile(cid, w.get("disc_weight"), w.get("disc_pot"), w.get("penalty_weight"))
        v, a = twin_solve(tab, prof, idx0, **S2)
        tabs.append(tab); profs.append(prof); V.append(v); arg.append(a)
    return dict(tabs=tabs, profs=profs, idx0=[p[2] for p in S2_PROBLEMS], V=np.stack(V), arg=np.stack(arg))


def configs(S, which):
    """The package Configs of a shape's problems (table_row0 in the concatenation of its tables)."""
    if which == "s1":
        d = s1()
        return [S.make_config(98, 0, d["tab"].shape[0])]
    d = s2()
    row0 = np.cumsum([0] + [t.shape[0] for t in d["tabs"]])
    return [S.make_config(cid, int(row0[k]), d["tabs"][k].shape[0], **w) for k, (cid, _, _, w) in enumerate(S2_PROBLEMS)]

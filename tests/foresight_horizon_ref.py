"""Shared by the receding-horizon tests: what shems_foresight_solve_horizon_dev must leave, from the definition and the oracle twin.

The expectation is built from the brute-force definition (NOT from foresight.horizon_plan or the header's helpers): for decision hour
t the plan was made at j = t - t mod c and ends at hi = min(j + H, T); V[t + 1] is plane 0 of foresight_twin.twin_solve on the window
(idx0 + t + 1, hi - (t + 1)), zeros when that length is 0; V[0] is plane 0 of the first plan; argmax[t] is row 0 of the arg-max of
the window (idx0 + t, hi - t).  Every twin window is solved once per process and shared; callers must not modify what they get.
"""
from __future__ import annotations

import functools

import numpy as np

import foresight_twin as FT


def brute_plan(T, H, c):
    """(j[t], k[t]) for t = 0 .. T - 1, written out hour by hour."""
    j, k = [], []
    for t in range(T):
        made = t - t % c
        j.append(made)
        k.append(min(made + H, T) - (t + 1))
    return np.array(j, np.int64), np.array(k, np.int64)


def _problem(which, p):
    if which == "s1":
        d = FT.s1()
        return d["tab"], d["prof"], d["idx0"], FT.S1
    d = FT.s2()
    return d["tabs"][p], d["profs"][p], d["idx0"][p], FT.S2


@functools.lru_cache(maxsize=None)
def twin_window(which, p, t, k):
    """(V[0], arg[0]) of the twin on the k >= 1 hours that start at hour t of problem p."""
    tab, prof, idx0, shape = _problem(which, p)
    V, arg = FT.twin_solve(tab, prof, idx0 + t, k, shape["nb"], shape["ne"], shape["nab"], shape["nae"])
    return V[0], arg[0]


@functools.lru_cache(maxsize=None)
def expected(which, p, H, c):
    """V [T + 1][N] float64 and argmax [T][N] int32 of problem p under (H, c)."""
    _, _, _, shape = _problem(which, p)
    T, N = shape["T"], shape["nb"] * shape["ne"]
    j, k = brute_plan(T, H, c)
    V, arg = np.zeros((T + 1, N)), np.zeros((T, N), np.int32)
    V[0] = twin_window(which, p, 0, int(k[0]) + 1)[0]
    for t in range(T):
        if k[t] > 0:
            V[t + 1] = twin_window(which, p, t + 1, int(k[t]))[0]
        arg[t] = twin_window(which, p, t, int(k[t]) + 1)[1]
    return V, arg

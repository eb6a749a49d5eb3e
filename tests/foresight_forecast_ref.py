"""Shared by the forecast tests: what shems_foresight_solve_forecast_dev must leave, from the definition and the oracle twin.

The expectation is built from the definition (NOT from the package or the header's helpers): the plan made at hour j believes the
COMPOSITE table -- the true rows up to table row idx0 + j, the forecast table's rows after it --, and everything the receding-horizon
controller defines holds on that table: for decision hour t, j = t - t mod c and hi = min(j + H, T); V[t + 1] is plane 0 of
foresight_twin.twin_solve on the composite's window (idx0 + t + 1, hi - (t + 1)), zeros when that length is 0; V[0] is plane 0 of the
first plan; argmax[t] is row 0 of the arg-max of the window (idx0 + t, hi - t).  With forecast = truth the composite is the truth and
this is foresight_horizon_ref.expected.  Every twin window is solved once per process and shared; callers must not modify what they
get.

Forecasts: persistence restated row by row (S1: lag 6, S2: lag 3); "lp" shifts load and PV, "all" the two EV columns too.
"""
from __future__ import annotations

import functools

import numpy as np

import foresight_horizon_ref as FR
import foresight_twin as FT

LAG = {"s1": 6, "s2": 3}
COLS = {"lp": (2, 3), "all": (0, 1, 2, 3), "ev": (0, 1)}               # h_countdown, soc_ev, electkwh, PV_generation = columns 0 .. 3
NAMES = {"lp": ("electkwh", "PV_generation"), "all": ("electkwh", "PV_generation", "h_countdown", "soc_ev"), "ev": ("h_countdown", "soc_ev")}


def persistence(tab, lag, cols):
    """Row i of the named columns = row i - lag for i >= lag, written out row by row."""
    out = np.array(tab, np.float32, copy=True)
    for i in range(lag, tab.shape[0]):
        for k in cols:
            out[i, k] = tab[i - lag, k]
    return out


@functools.lru_cache(maxsize=None)
def forecast(which, p, kind):
    """The forecast table of problem p: kind "truth" (a byte copy), "lp", "all" or "ev"."""
    tab = FR._problem(which, p)[0]
    return np.array(tab, np.float32, copy=True) if kind == "truth" else persistence(tab, LAG[which], COLS[kind])


@functools.lru_cache(maxsize=None)
def composite(which, p, kind, j):
    """What the plan made at hour j believes: true rows up to table row idx0 + j (1-based), forecast rows after."""
    tab, _, idx0, _ = FR._problem(which, p)
    out = np.array(forecast(which, p, kind), np.float32, copy=True)
    out[:idx0 + j] = tab[:idx0 + j]
    return out


@functools.lru_cache(maxsize=None)
def twin_window(which, p, kind, j, t, k):
    """(V[0], arg[0]) of the twin on the k >= 1 hours that start at hour t, on the belief of the plan made at j."""
    _, prof, idx0, shape = FR._problem(which, p)
    V, arg = FT.twin_solve(composite(which, p, kind, j), prof, idx0 + t, k, shape["nb"], shape["ne"], shape["nab"], shape["nae"])
    return V[0], arg[0]


@functools.lru_cache(maxsize=None)
def expected(which, p, kind, H, c):
    """V [T + 1][N] float64 and argmax [T][N] int32 of problem p under (H, c) and the forecast `kind`."""
    _, _, _, shape = FR._problem(which, p)
    T, N = shape["T"], shape["nb"] * shape["ne"]
    j, k = FR.brute_plan(T, H, c)
    V, arg = np.zeros((T + 1, N)), np.zeros((T, N), np.int32)
    V[0] = twin_window(which, p, kind, 0, 0, int(k[0]) + 1)[0]
    for t in range(T):
        if k[t] > 0:
            V[t + 1] = twin_window(which, p, kind, int(j[t]), t + 1, int(k[t]))[0]
        arg[t] = twin_window(which, p, kind, int(j[t]), t, int(k[t]) + 1)[1]
    return V, arg

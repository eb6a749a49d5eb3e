"""The perfect-foresight controller: the exact dynamic programme of shems_LU1's step! on the GPU.

The thesis scores every controller against two yardsticks: the rule-based "power mode" (harness.inference(track < 0)) and a
perfect-foresight optimiser.  With the exogenous series known in advance, the best action sequence of the environment AS WRITTEN
(action shems_LU1.jl:283-316, step! :343-485, next_state! :264-281, scored by the plain sum of rewards,
memory_plotting_saving.jl:62-89) is a finite-horizon dynamic programme over (Soc_b, Soc_ev):

    solve(tables, configs, idx0, nsteps, grid) -> Values      the backward sweep, V float64 [P][T + 1][nb * ne]  (shems_foresight_solve_dev)
    track(env, values, problem_of_env, which)                 the greedy controller on the exact env, one launch    (shems_foresight_track_dev)
    solve_horizon(tables, configs, idx0, nsteps, horizon, control) -> Values
                                                              the same recursion with `horizon` hours of forecast and a fresh plan
                                                              every `control` hours, one launch     (shems_foresight_solve_horizon_dev)
    solve_horizon(..., forecast_table=[...]) -> Values        the same controller planning on a forecast that may be wrong
                                                              (shems_foresight_solve_forecast_dev / _track_forecast_dev)
    persistence_forecast(table, lag) / append_forecasts       the standard naive forecast: hour t is what it was `lag` hours earlier
    solve_ensemble(..., scenarios=[[...]], weights) -> EnsembleValues
                                                              the same controller HEDGING over K forecasts: the K sweeps are K records
                                                              of the one forecast call, track weighs every action against all K planes
                                                              (shems_foresight_track_ensemble_dev)
    analog_scenarios(table, lags) / append_scenarios          the "same hour on previous days" ensemble: one persistence forecast per lag
    audit(values, results, problem_of_pass) -> Audit          the hourly regret of ANY tracked pass against V, one launch, parallel over
                                                              passes x hours x actions                   (shems_foresight_audit_dev)

The arithmetic lives in csrc/shems_foresight_core.h; Values.at restates its interpolation on the host, bit for bit.  A discretised
value function with a greedy policy is NOT a bound: V_0 at the start state and the achieved return differ by the discretisation error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import Config


class GridStruct(C.Structure):            # shems_foresight_grid
    _fields_ = [("nb", C.c_int32), ("ne", C.c_int32), ("nab", C.c_int32), ("nae", C.c_int32)]


class Problem(C.Structure):               # shems_foresight_problem
    _fields_ = [("cfg", Config), ("idx0", C.c_int32), ("forecast_off", C.c_int32), ("scale_b", C.c_double), ("hb", C.c_double)]


assert C.sizeof(Problem) == 72 and Problem.forecast_off.offset == 52 and C.sizeof(GridStruct) == 16

MAX_PLANE_BYTES = 150000                  # a workgroup of the sweep stages one V plane in LDS; one of solve_horizon keeps two


class Grid:
    """State nodes nb x ne over [0, soc_max] x [0, 1] and action targets nab x nae over [0, 1]^2.  The default 65 x 33 makes
    0.5 * soc_max, the start of reset!(rng = -1), a node."""

    def __init__(self, nb=65, ne=33, nab=17, nae=17):
        self.nb, self.ne, self.nab, self.nae = int(nb), int(ne), int(nab), int(nae)
        if self.nb < 2 or self.ne < 2:
            raise ValueError(f"the state grid is {self.nb} x {self.ne} nodes; each axis needs at least 2")
        if self.nab < 1 or self.nae < 1:
            raise ValueError(f"the action grid is {self.nab} x {self.nae} targets; each axis needs at least 1")
        if self.nb * self.ne * 8 > MAX_PLANE_BYTES:
            raise ValueError(f"a V plane of {self.nb} x {self.ne} nodes does not fit the {MAX_PLANE_BYTES} bytes of LDS a workgroup stages")

    nodes = property(lambda self: self.nb * self.ne)
    actions = property(lambda self: self.nab * self.nae)

    def struct(self):
        return GridStruct(self.nb, self.ne, self.nab, self.nae)

    def soc_b_nodes(self, soc_max):
        """Soc_b[i] = (float)(i * hb), hb = (double)soc_max / (nb - 1); the last node is soc_max itself."""
        hb = float(np.float32(soc_max)) / (self.nb - 1)
        x = np.array([np.float32(i * hb) for i in range(self.nb)], np.float32)
        x[-1] = np.float32(soc_max)
        return x

    def soc_ev_nodes(self):
        he = 1.0 / (self.ne - 1)
        x = np.array([np.float32(j * he) for j in range(self.ne)], np.float32)
        x[-1] = np.float32(1.0)
        return x

    @staticmethod
    def _targets(n):
        return np.array([1.0] if n == 1 else [np.float32(a / float(n - 1)) for a in range(n)], np.float32)

    def b_targets(self):
        return self._targets(self.nab)

    def ev_targets(self):
        return self._targets(self.nae)

    def targets(self):
        """[nab * nae][2] float32 (B_target, EV_target) in action-index order a = ab * nae + ae."""
        b, e = self.b_targets(), self.ev_targets()
        return np.stack([np.repeat(b, self.nae), np.tile(e, self.nab)], 1).astype(np.float32)

    def __repr__(self):
        return f"Grid(nb={self.nb}, ne={self.ne}, nab={self.nab}, nae={self.nae})"


def interpolate(plane, grid, soc_max, soc_b, soc_ev):
    """V off the nodes, the order of operations of fs_value (csrc/shems_foresight_core.h): per axis u = x * scale,
    i = clamp(floor(u), 0, n - 2), f = clamp(u - i, 0, 1); V = (1 - fe) ((1 - fb) V00 + fb V10) + fe ((1 - fb) V01 + fb V11), all
    in float64.  plane: [nb * ne] float64; soc_b / soc_ev: float32 arrays (or scalars)."""
    V = np.asarray(plane, np.float64).reshape(grid.nb, grid.ne)
    scale_b = (grid.nb - 1) / float(np.float32(soc_max))
    scale_e = float(grid.ne - 1)

    def axis(x, scale, n):
        u = np.asarray(x, np.float32).astype(np.float64) * scale
        fl = np.clip(np.floor(u), 0.0, float(n - 2))
        return fl.astype(np.int64), np.clip(u - fl, 0.0, 1.0)

    ib, fb = axis(soc_b, scale_b, grid.nb)
    ie, fe = axis(soc_ev, scale_e, grid.ne)
    V00, V01, V10, V11 = V[ib, ie], V[ib, ie + 1], V[ib + 1, ie], V[ib + 1, ie + 1]
    return (1.0 - fe) * ((1.0 - fb) * V00 + fb * V10) + fe * ((1.0 - fb) * V01 + fb * V11)


def belief_offset(u, j, forecast_off):
    """fs_belief_off of csrc/shems_foresight_core.h restated: the row offset (added to table_row0) of the row of hour u in the plan made
    at hour j -- the truth up to the hour the plan is made, the forecast table after it."""
    return int(forecast_off) if u > j else 0


def persistence_forecast(table, lag=24, columns=("electkwh", "PV_generation")):
    """The standard naive forecast of a [nrow][8] table: the named columns (names of tables.COLUMNS) of row i are those of row i - lag
    for i >= lag; rows below lag and all other columns are the truth's.  Returns [nrow][8] float32.
    The default leaves h_countdown / soc_ev true: the observation itself carries the countdown, so the departure is known once the
    car is plugged in -- and with these two columns true, FUTURE ARRIVALS are known too.  Adding "h_countdown" and "soc_ev" gives the
    controller that knows nothing ahead.  As a forecast table of solve_horizon it is causal for horizon <= lag (every forecast row is
    an hour already observed when the plan is made); for horizon > lag it is not, and nothing refuses that."""
    from .tables import COLUMNS
    tab = np.ascontiguousarray(table, dtype=np.float32)
    if tab.ndim != 2 or tab.shape[1] != _capi.NCOL:
        raise ValueError("a table must be [nrow][8] float32")
    lag = int(lag)
    if lag < 1 or lag >= tab.shape[0]:
        raise ValueError(f"lag = {lag}; persistence needs 1 <= lag < nrow = {tab.shape[0]}")
    cols = []
    for name in columns:
        if name not in COLUMNS:
            raise ValueError(f"unknown column {name!r}; a table holds {COLUMNS}")
        cols.append(COLUMNS.index(name))
    out = tab.copy()
    out[lag:, cols] = tab[:-lag, cols]
    return out


EV_COLUMNS = ("h_countdown", "soc_ev")


def append_forecasts(tables, lag=24, columns=("electkwh", "PV_generation")):
    """The table list of a batch with one persistence forecast per table appended: returns (tables + forecasts, index) with
    index[k] = the position of table k's forecast in the new list -- an entry of solve_horizon's forecast_table.  Build the
    ShemsBatch that foresight.track steps from the same list, so that both see the same row array."""
    tabs = list(tables) if isinstance(tables, (list, tuple)) else [tables]
    return tabs + [persistence_forecast(t, lag, columns) for t in tabs], [len(tabs) + k for k in range(len(tabs))]


ANALOG_LAGS = (24, 48, 72, 96, 120, 144, 168)
MAX_SCENARIOS = 16                        # kFsMaxScen of csrc/shems_foresight_core.h


def analog_scenarios(table, lags=ANALOG_LAGS, columns=("electkwh", "PV_generation")):
    """The "same hour on previous days" ensemble of a [nrow][8] table: one persistence_forecast per lag, in the order of `lags`
    (default: the same hour of each of the last seven days).  Returns a list of [nrow][8] float32 tables.  As scenario tables of
    solve_ensemble the ensemble is causal for horizon <= min(lags) (every scenario row is an hour already observed when the plan is
    made) and not beyond, and nothing refuses that.  Rows below a lag are the truth's in that member, as in persistence_forecast."""
    lags = [int(l) for l in lags]
    if not lags:
        raise ValueError("analog_scenarios needs at least one lag")
    return [persistence_forecast(table, lag, columns) for lag in lags]


def append_scenarios(tables, lags=ANALOG_LAGS, columns=("electkwh", "PV_generation")):
    """The table list of a batch with the analog ensemble of every table appended: returns (tables + scenarios, index) with
    index[k] = the list of positions of table k's scenarios in the new list -- an entry of solve_ensemble's `scenarios`.  Build the
    ShemsBatch that foresight.track steps from the same list, so that both see the same row array."""
    tabs = list(tables) if isinstance(tables, (list, tuple)) else [tables]
    out, index = list(tabs), []
    for t in tabs:
        sc = analog_scenarios(t, lags, columns)
        index.append(list(range(len(out), len(out) + len(sc))))
        out += sc
    return out, index


def _forecast_offsets(forecast_table, problems, row0, nrow, n_scen=None):
    """forecast_table (one entry per problem record: None or the index of a table) -> forecast_off per record; row0 / nrow: of the
    tables.  n_scen: the records are those of an ensemble, n_scen per problem, and a refusal names (problem, scenario); an ensemble also
    refuses an index that is no integer (a forecast_table entry is truncated)."""
    entries = list(forecast_table)
    if len(entries) != len(problems):
        raise ValueError(f"forecast_table holds {len(entries)} entries for {len(problems)} problems")
    offs = []
    for r, k in enumerate(entries):
        if k is None:
            offs.append(0)
            continue
        i = int(k)
        if n_scen is None:
            who, table, shown, ok = f"problem {r}", "forecast table", i, True
        else:
            who, table, shown, ok = f"problem {r // n_scen}, scenario {r % n_scen}", "table", repr(k), i == k
        if not ok or i < 0 or i >= len(row0):
            raise ValueError(f"{who}: {table} {shown} is outside the {len(row0)} tables")
        if int(nrow[i]) != problems[r].cfg.nrow:
            raise ValueError(f"{who}: {table} {i} has {int(nrow[i])} rows, its table {problems[r].cfg.nrow}")
        offs.append(int(row0[i]) - problems[r].cfg.table_row0)
    return offs


def _start_rows(idx0, n_problems):
    """idx0 (one start row, or one per problem) as a list of n_problems ints."""
    starts = [int(idx0)] * n_problems if np.isscalar(idx0) else [int(i) for i in idx0]
    if len(starts) != n_problems:
        raise ValueError(f"idx0 holds {len(starts)} start rows for {n_problems} problems")
    return starts


def make_problems(configs, idx0, nsteps, grid, total_rows=None):
    """The shems_foresight_problem records of one call, validated on the host (ValueError before any device work).  scale_b / hb
    are filled for the host side (Values.at); shems_foresight_solve_dev forms the device copy's own."""
    cfgs = list(configs)
    T = int(nsteps)
    if not isinstance(grid, Grid):
        raise TypeError("grid must be a foresight.Grid")
    if not cfgs:
        raise ValueError("solve needs at least one problem")
    if T < 1:
        raise ValueError(f"nsteps = {T}; the horizon must be at least 1 hour")
    starts = _start_rows(idx0, len(cfgs))
    recs = (Problem * len(cfgs))()
    for p, (c, i0) in enumerate(zip(cfgs, starts)):
        if c.table_row0 < 0 or c.nrow < 2 or (total_rows is not None and c.table_row0 + c.nrow > total_rows):
            raise ValueError(f"problem {p} names table rows {c.table_row0} .. {c.table_row0 + c.nrow} of {total_rows}")
        if i0 < 1 or i0 + T > c.nrow:
            raise ValueError(f"problem {p}: the window of rows {i0} .. {i0 + T} runs off its table of {c.nrow} rows "
                             "(a pass of n steps reads row n + 1)")
        if not c.soc_max > 0:
            raise ValueError(f"problem {p}: soc_max must be positive")
        recs[p].cfg = c
        recs[p].idx0 = i0
        recs[p].scale_b = (grid.nb - 1) / float(c.soc_max)
        recs[p].hb = float(c.soc_max) / (grid.nb - 1)
    return recs


def _declare(L):
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.shems_foresight_solve_dev.argtypes = [vp, i64, C.POINTER(Problem), vp, i32, C.POINTER(GridStruct), i32, vp, i64, vp, vp]
    L.shems_foresight_solve_dev.restype = C.c_int
    L.shems_foresight_solve_horizon_dev.argtypes = [vp, i64, C.POINTER(Problem), vp, i32, C.POINTER(GridStruct), i32, i32, i32, vp, i64, vp, vp]
    L.shems_foresight_solve_horizon_dev.restype = C.c_int
    L.shems_foresight_solve_forecast_dev.argtypes = L.shems_foresight_solve_horizon_dev.argtypes
    L.shems_foresight_solve_forecast_dev.restype = C.c_int
    L.shems_foresight_track_dev.argtypes = [C.POINTER(_capi.View), vp, i32, vp, C.POINTER(GridStruct), i32, vp, i64, vp, i64, vp, vp, vp]
    L.shems_foresight_track_dev.restype = C.c_int
    L.shems_foresight_track_forecast_dev.argtypes = L.shems_foresight_track_dev.argtypes
    L.shems_foresight_track_forecast_dev.restype = C.c_int
    L.shems_foresight_track_ensemble_dev.argtypes = [C.POINTER(_capi.View), vp, i32, i32, vp, vp, vp, C.POINTER(GridStruct), i32, vp, i64, vp, i64,
                                                     vp, vp, vp]
    L.shems_foresight_track_ensemble_dev.restype = C.c_int
    L.shems_foresight_audit_dev.argtypes = [vp, i64, vp, i32, C.POINTER(GridStruct), i32, vp, i64, vp, i32, vp, vp, vp, vp, vp]
    L.shems_foresight_audit_dev.restype = C.c_int
    return L


class Values:
    """What solve leaves on the device: V [P][T + 1][nb * ne] float64, the winning action index of every (problem, hour, node)
    [P][T][nb * ne] int32, and the problem records the forward pass needs.  horizon / control: what solve_horizon was given (None
    from solve: the whole pass is known).  forecast_off: per problem, the row offset of its forecast table (all 0: the plans saw the
    truth); total_rows: the length of the row array the solve call saw, host_rows: its host copy [total_rows][8]."""

    def __init__(self, grid, nsteps, problems, d_problems, V, argmax, tables=None, horizon=None, control=None, forecast_off=None,
                 total_rows=None, host_rows=None):
        self.grid, self.nsteps, self.problems, self.d_problems, self.V, self.argmax, self._tables = grid, int(nsteps), problems, d_problems, V, argmax, tables
        self.n_problems = len(problems)
        self.horizon, self.control = horizon, control
        self.forecast_off = [0] * self.n_problems if forecast_off is None else [int(o) for o in forecast_off]
        self.total_rows = total_rows
        self.host_rows = host_rows

    def plane(self, p, t):
        """V_t of problem p as a host array [nb][ne]."""
        return self.V[int(p), int(t)].cpu().numpy().reshape(self.grid.nb, self.grid.ne)

    def at(self, p, t, soc_b, soc_ev):
        """V_t of problem p at an off-grid state: the device's interpolation restated on the host."""
        out = interpolate(self.V[int(p), int(t)].cpu().numpy(), self.grid, self.problems[int(p)].cfg.soc_max, soc_b, soc_ev)
        return float(out) if np.ndim(out) == 0 else out


def horizon_plan(T, horizon, control=1):
    """The receding-horizon schedule of csrc/shems_foresight_core.h restated: for the decision hours t = 0 .. T - 1, j[t] = the hour
    the plan in force was made (t - t mod control) and k[t] = the look-ahead length after hour t, hi - (t + 1) with
    hi = min(j + horizon, T): U_{t+1}, the plane V[p][t + 1], is the value of those k[t] hours (zero for k[t] = 0).  Two int64 arrays."""
    T, H, c = _check_horizon(T, horizon, control)
    t = np.arange(T, dtype=np.int64)
    j = t - t % c
    return j, np.minimum(j + H, T) - (t + 1)


def _check_horizon(T, horizon, control):
    T, H, c = int(T), int(horizon), int(control)
    if T < 1:
        raise ValueError(f"nsteps = {T}; the pass must be at least 1 hour")
    if H < 1:
        raise ValueError(f"horizon = {H}; a plan sees at least the current hour")
    if c < 1 or c > H:
        raise ValueError(f"control = {c}; a fresh plan every 1 .. horizon = {H} hours")
    return T, H, c


def _table_rows(tables):
    """(row0, nrow) of the tables of a list / one table / a ShemsBatch, without touching a device."""
    if hasattr(tables, "table_row0"):
        return [int(x) for x in tables.table_row0], [int(x) for x in tables.table_nrow]
    tabs = tables if isinstance(tables, (list, tuple)) else [tables]
    nrow = [int(np.shape(t)[0]) for t in tabs]
    return [int(x) for x in np.cumsum([0] + nrow)[:-1]], nrow


def _solve(tables, configs, idx0, nsteps, grid, want_argmax, horizon=None, control=None, forecast_table=None, n_scen=None):
    import torch
    from .env import ShemsBatch
    grid = Grid() if grid is None else grid
    env = tables if isinstance(tables, ShemsBatch) else None
    rows = None
    if env is None:
        tabs = tables if isinstance(tables, (list, tuple)) else [tables]
        tabs = [np.ascontiguousarray(t, dtype=np.float32) for t in tabs]
        for t in tabs:
            if t.ndim != 2 or t.shape[1] != _capi.NCOL:
                raise ValueError("a table must be [nrow][8] float32")
        rows = np.ascontiguousarray(np.concatenate(tabs, 0))
    row0, nrow = _table_rows(tabs if env is None else env)
    total_rows = row0[-1] + nrow[-1]
    problems = make_problems(configs, idx0, nsteps, grid, total_rows)
    offs = None
    if forecast_table is not None:
        forecast_table = list(forecast_table)
        offs = _forecast_offsets(forecast_table, problems, row0, nrow, n_scen)
        for rec, o in zip(problems, offs):
            rec.forecast_off = o
        if all(k is None for k in forecast_table):
            offs = None                                      # no entry set: today's entry point
    T, P, N = int(nsteps), len(problems), grid.nodes
    if horizon is not None:
        _, horizon, control = _check_horizon(T, horizon, control)
        if 2 * N * 8 > MAX_PLANE_BYTES:
            raise ValueError(f"the two V planes of {grid.nb} x {grid.ne} nodes a window keeps take {2 * N * 8} bytes of LDS; "
                             f"a workgroup has {MAX_PLANE_BYTES} for them")
    L = _declare(_capi.lib())
    dev = torch.device("cuda", torch.cuda.current_device())
    if env is None:
        d_tables = torch.from_numpy(rows).to(dev)
        tab_ptr = d_tables.data_ptr()
    else:
        env.use_torch_stream()
        d_tables = env                                       # keeps the handle (and its tables) alive
        tab_ptr = env.view().tables
    d_prob = torch.empty(C.sizeof(problems), dtype=torch.uint8, device=dev)      # filled by the call, read by the sweep and by track
    V = torch.empty((P, T + 1, N), dtype=torch.float64, device=dev)
    arg = torch.empty((P, T, N), dtype=torch.int32, device=dev) if want_argmax else None
    g = grid.struct()
    head = (C.c_void_p(tab_ptr), total_rows, problems, C.c_void_p(d_prob.data_ptr()), P, C.byref(g), T)
    tail = (C.c_void_p(V.data_ptr()), V.numel(), C.c_void_p(arg.data_ptr()) if arg is not None else None,
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if horizon is None:
        _capi.check(L.shems_foresight_solve_dev(*head, *tail))
    elif offs is None:
        _capi.check(L.shems_foresight_solve_horizon_dev(*head, horizon, control, *tail))
    else:
        _capi.check(L.shems_foresight_solve_forecast_dev(*head, horizon, control, *tail))
    return Values(grid, T, problems, d_prob, V, arg, d_tables, horizon, control, offs, total_rows, rows if env is None else env.host_rows)


def solve(tables, configs, idx0, nsteps, grid=None, want_argmax=True):
    """The backward sweep for P problems (table, config, 1-based start row) sharing the horizon `nsteps` and the grid: one foreign
    call enqueues one launch per hour on PyTorch's current stream, no host synchronisation.  tables: a list of [nrow][8] float32
    tables (configs[p].table_row0 / nrow name problem p's rows in their concatenation, as for ShemsBatch), or a ShemsBatch, whose
    device-resident tables are then used.  configs: one Config per problem; idx0: one start row, or one per problem."""
    return _solve(tables, configs, idx0, nsteps, grid, want_argmax)


def solve_horizon(tables, configs, idx0, nsteps, horizon, control=1, grid=None, want_argmax=True, forecast_table=None):
    """The receding-horizon controller's planes for P problems, arguments as solve: at hour t the plan made at j = t - t mod control
    sees hours j .. min(j + horizon, nsteps) - 1 (horizon_plan; the definition: csrc/shems_foresight_core.h).  Values.V[p][t] is
    what track reads at hour t - 1, V[p][0] the value of the first plan, argmax[p][t] the action taken at hour t from each node;
    with horizon >= nsteps they equal solve's bit for bit.  One launch on PyTorch's current stream (shems_foresight_solve_horizon_dev),
    one workgroup per (window of `control` hours, problem) with its planes in LDS, no host synchronisation; a state grid whose two
    planes exceed 150 000 bytes is refused (129 x 65 fits).  The call always runs the window kernel: with few windows (problems x
    ceil(nsteps / control) below the device's CU count) it under-fills the device, and for horizon >= nsteps solve is the tool.
    forecast_table: one entry per problem, None (the plans see the true rows) or the index of that problem's forecast table in
    `tables` (the list, or the ShemsBatch's own tables; same nrow): the plan made at hour j then reads the true rows up to j and the
    forecast's after it (the definition: csrc/shems_foresight_core.h; shems_foresight_solve_forecast_dev, one launch), and track
    takes the arrival overwrite's next row from the forecast.  argmax[p][t] for t > j is what the plan made at j intends under its
    forecast.  One forecast table cannot depend on when the forecast was issued: persistence_forecast is causal for
    horizon <= lag and not beyond, and nothing is refused for that.  With every entry None the call is today's."""
    if horizon is None:
        raise ValueError("solve_horizon needs a horizon (solve knows the whole pass)")
    return _solve(tables, configs, idx0, nsteps, grid, want_argmax, horizon, control, forecast_table)


class EnsembleValues:
    """What solve_ensemble leaves: `values`, the Values of the ONE forecast solve over its P * K records (record p * K + k: problem p
    under scenario k), n_scen = K, and weights [P][K] float64, normalised to sum 1 per problem.  track takes it; audit refuses it."""

    def __init__(self, values, n_scen, weights):
        self.values, self.n_scen = values, int(n_scen)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.n_problems = self.weights.shape[0]
        self.grid, self.nsteps, self.horizon, self.control, self.total_rows = values.grid, values.nsteps, values.horizon, values.control, values.total_rows


def ensemble_weights(weights, n_problems, n_scen):
    """[P][K] float64 weights, normalised to sum 1 per problem: None (equal weights), one vector of K for every problem, or [P][K].
    A weight that is <= 0 or not finite, or a length that does not match, is a ValueError."""
    P, K = int(n_problems), int(n_scen)
    if weights is None:
        w = np.ones((P, K), np.float64)
    else:
        w = np.array(weights, np.float64)
        if w.shape == (K,):
            w = np.tile(w, (P, 1))
        if w.shape != (P, K):
            raise ValueError(f"weights of shape {np.shape(weights)} for {P} problems x {K} scenarios: one vector of {K}, or [{P}][{K}]")
    bad = np.argwhere(~(np.isfinite(w) & (w > 0)))
    if bad.size:
        p, k = (int(x) for x in bad[0])
        raise ValueError(f"problem {p}, scenario {k}: weight {w[p, k]!r}; a weight is finite and > 0")
    return np.ascontiguousarray(w / w.sum(axis=1, keepdims=True))


def solve_ensemble(tables, configs, idx0, nsteps, horizon, control=1, scenarios=None, weights=None, grid=None):
    """The planes of the receding-horizon controller that HEDGES over a forecast ensemble (the definition:
    csrc/shems_foresight_core.h).  tables, configs, idx0, nsteps, horizon, control, grid as solve_horizon.  scenarios: one list per
    problem of the K table indices of its scenario tables (1 <= K <= 16, the same K for every problem; append_scenarios builds such
    lists; an index may name the truth itself); weights: None (equal), K weights for every problem, or [P][K], each finite and > 0,
    normalised here to sum 1.  The K sweeps of a problem are K records of ONE shems_foresight_solve_forecast_dev call (P * K records,
    problem-major, scenario-minor, no arg-max); track then weighs every action against all K planes
    (shems_foresight_track_ensemble_dev).  The controller is the two-stage scenario programme: optimistic about what is learnt after
    the first decision, and not claimed to beat any of its members.  Refused with a ValueError before any device work: ragged
    scenario lists, K outside 1 .. 16, a bad weight or weight shape, a scenario table with the wrong nrow or outside the tables."""
    if horizon is None:
        raise ValueError("solve_ensemble needs a horizon (solve knows the whole pass)")
    cfgs = list(configs)
    if scenarios is None:
        raise ValueError("solve_ensemble needs the scenarios of every problem (lists of table indices; see append_scenarios)")
    scen = [list(s) if isinstance(s, (list, tuple, np.ndarray)) else [s] for s in scenarios]
    if len(scen) != len(cfgs):
        raise ValueError(f"scenarios holds {len(scen)} lists for {len(cfgs)} problems")
    K = len(scen[0]) if scen else 0
    if any(len(s) != K for s in scen):
        raise ValueError(f"ragged scenario lists ({[len(s) for s in scen]}): every problem takes the same number of scenarios")
    if K < 1 or K > MAX_SCENARIOS:
        raise ValueError(f"{K} scenarios; an ensemble holds 1 .. {MAX_SCENARIOS}")
    w = ensemble_weights(weights, len(cfgs), K)
    starts = _start_rows(idx0, len(cfgs))
    # the records' own refusals (rows, start rows, scenario tables) are make_problems' and _forecast_offsets', before any device work
    inner = _solve(tables, [c for c in cfgs for _ in range(K)], [i for i in starts for _ in range(K)], nsteps, grid, False, horizon, control,
                   [i for sc in scen for i in sc], K)
    return EnsembleValues(inner, K, w)


def track(env, values, problem_of_env=None, which=-1):
    """The greedy controller on the exact env, from the envs' CURRENT state (reset them onto their problem's start row first): env e
    runs values.nsteps hours of problem problem_of_env[e] (None: problem 0) in one launch.  Returns (totals [n] float64, results
    [n][T][23] float64 -- [1][T][23] of env `which` when which >= 0 --, targets [n][T][2] float32, the chosen (B_target,
    EV_target)).  An env that does not sit on its problem's start row raises BoundsError and is not stepped.  Values solved with a
    forecast table go through shems_foresight_track_forecast_dev, which reads the ENV's row array: the env's batch must hold the
    same tables in the same order as the solve call saw (a different total row count is a ValueError).  EnsembleValues (solve_ensemble)
    go through shems_foresight_track_ensemble_dev under the same condition; problem_of_env then names the problem, not its records."""
    ens = values if isinstance(values, EnsembleValues) else None
    if ens is not None:
        values = ens.values                                  # the one forecast solve: its records and planes
    forecast = any(values.forecast_off)
    if forecast:
        env_rows = int(env.table_row0[-1] + env.table_nrow[-1])
        if values.total_rows != env_rows:
            raise ValueError(f"the values were solved on a row array of {values.total_rows} rows and the env holds {env_rows}: a forecast "
                             "pass needs the env's batch to hold the same tables in the same order")
    import torch
    L = _declare(_capi.lib())
    n, T = env.n, values.nsteps
    env.use_torch_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    poe = None
    if problem_of_env is not None:
        po = np.ascontiguousarray(problem_of_env, dtype=np.int32)
        if po.shape != (n,):
            raise ValueError("problem_of_env must have shape (n_envs,)")
        poe = torch.from_numpy(po).to(dev)
    rows = n if which < 0 else 1
    res = torch.empty((rows, T, _capi.NRESULT), dtype=torch.float64, device=dev)
    total = torch.zeros(n, dtype=torch.float64, device=dev)
    tgt = torch.zeros((n, T, 2), dtype=torch.float32, device=dev)
    if ens is not None:
        d_w = torch.empty(ens.weights.shape, dtype=torch.float64, device=dev)      # filled by the call, read by the kernel
        fn, P = L.shems_foresight_track_ensemble_dev, ens.n_problems
        scen = (ens.n_scen, ens.weights.ctypes.data_as(C.c_void_p), C.c_void_p(d_w.data_ptr()))
    else:
        fn, P, scen = L.shems_foresight_track_forecast_dev if forecast else L.shems_foresight_track_dev, values.n_problems, ()
    v = env.view()
    g = values.grid.struct()
    _capi.check(fn(C.byref(v), C.c_void_p(values.d_problems.data_ptr()), P, *scen,
                   C.c_void_p(poe.data_ptr()) if poe is not None else None, C.byref(g), T,
                   C.c_void_p(values.V.data_ptr()), values.V.numel(), C.c_void_p(res.data_ptr()), int(which),
                   C.c_void_p(total.data_ptr()), C.c_void_p(tgt.data_ptr()), env._stream()))
    out, tot, targets = res.cpu().numpy(), total.cpu().numpy(), tgt.cpu().numpy()      # the pass's one synchronisation
    env.check_error()
    return tot, out, targets


def problems_of_env(env, idx=None):
    """One problem per distinct (config, start row) of a batch: returns (configs, idx0, problem_of_env).  idx: the envs' start rows
    (default: where they sit now)."""
    idx = np.asarray(env.idx if idx is None else idx, np.int64).reshape(env.n)
    co = np.zeros(env.n, np.int64) if env.cfg_of_env is None else env.cfg_of_env.astype(np.int64)
    keys, inv = np.unique(np.stack([co, idx], 1), axis=0, return_inverse=True)
    return [env.configs[int(k[0])] for k in keys], [int(k[1]) for k in keys], np.asarray(inv, np.int32).reshape(env.n)


PHASES = ("absent", "arrival", "connected", "departure")


class Audit:
    """What audit returns, all host arrays: best_q, achieved_q, v_state [n][T] float64, best_action [n][T] int32, best_targets
    [n][T][2] float32 (the grid's (B_target, EV_target) of best_action), regret = best_q - achieved_q and discretisation =
    best_q - v_state.  Regret is NOT a bound: a controller acting off the action grid (a DDPG actor, or the rule-based controller,
    whose rows carry kWh set-points) can reach slightly negative values.  For Values from solve,
        sum_t regret[t] = best_q[0] - return + sum_{t >= 1} discretisation[t]
    up to float64 rounding (the definition: csrc/shems_foresight_core.h); for Values from solve_horizon best_q is what THAT controller
    would take from the state, and the identity does not apply."""

    def __init__(self, out, best_action, targets, rewards, phase):
        self.best_q, self.achieved_q, self.v_state = (np.ascontiguousarray(out[..., k]) for k in range(3))
        self.best_action = best_action
        self.best_targets = targets[np.maximum(best_action, 0)]
        self.best_targets[best_action < 0] = np.nan
        self.regret = self.best_q - self.achieved_q
        self.discretisation = self.best_q - self.v_state
        self.rewards, self.phase = rewards, phase             # [n][T] float64; [n][T] int8, an index into PHASES

    def summary(self):
        """Per pass, a dict of [n] float64 arrays: "return" (the sum of the rewards column), "regret" and "discretisation" (sums over
        the hours), and the regret summed by EV phase of the hour -- "absent" (c_ev = -1), "arrival" (c_ev = -1 and the next row's
        h_countdown >= 0; it takes precedence over absent), "departure" (c_ev = 0), "connected" (every other hour).  The four phase
        sums add up to "regret" up to rounding."""
        out = {"return": self.rewards.sum(1), "regret": self.regret.sum(1), "discretisation": self.discretisation.sum(1)}
        for k, name in enumerate(PHASES):
            out[name] = np.where(self.phase == k, self.regret, 0.0).sum(1)
        return out


def phases(c_ev, h_next):
    """The EV phase of an hour as an index into PHASES, from the c_ev column of its results row and h_countdown of the next table row."""
    c_ev, h_next = np.asarray(c_ev), np.asarray(h_next)
    ph = np.full(c_ev.shape, PHASES.index("connected"), np.int8)
    ph[c_ev == 0] = PHASES.index("departure")
    ph[c_ev == -1] = PHASES.index("absent")
    ph[(c_ev == -1) & (h_next >= 0)] = PHASES.index("arrival")
    return ph


def _audit_device(values, results, problem_of_pass=None):
    """audit's checks and its device work: returns (out [n][T][3] float64, best_action [n][T] int32, status [n] int32, the c_ev and
    rewards columns of the rows as host arrays [n][T], problem_of_pass as an int32 array or None) without judging the status."""
    if isinstance(values, EnsembleValues):
        raise ValueError("the values were solved on a forecast ensemble: an audit against a belief is not defined (audit the pass against "
                         "the values of a solve on the true rows)")
    if any(values.forecast_off):
        raise ValueError("the values were solved on a forecast table: an audit against a belief is not defined (audit the pass against "
                         "the values of a solve on the true rows)")
    is_tensor = not isinstance(results, np.ndarray) and hasattr(results, "data_ptr")
    res = results if is_tensor else np.asarray(results, np.float64)
    if res.ndim == 2:
        res = res[None]
    T = values.nsteps
    if res.ndim != 3 or res.shape[2] != _capi.NRESULT:
        raise ValueError(f"results must be [n][T][{_capi.NRESULT}] or [T][{_capi.NRESULT}], not {tuple(res.shape)}")
    if res.shape[1] != T:
        raise ValueError(f"results hold T = {res.shape[1]} hours and the values were solved for {T}")
    n = int(res.shape[0])
    if n < 1 or n > 65535:
        raise ValueError(f"one call audits 1 .. 65535 passes, not {n}")
    po = None
    if problem_of_pass is not None:
        po = np.ascontiguousarray(problem_of_pass, dtype=np.int32)
        if po.shape != (n,):
            raise ValueError(f"problem_of_pass must have shape ({n},), one problem per pass")
    if is_tensor and not (res.is_cuda and str(res.dtype) == "torch.float64"):
        raise ValueError("a results tensor must be a float64 CUDA tensor")
    L = _declare(_capi.lib())
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    env = values._tables if hasattr(values._tables, "use_torch_stream") else None        # a ShemsBatch, or the uploaded tensor
    if env is not None:
        env.use_torch_stream()
        tab_ptr = env.view().tables
    else:
        tab_ptr = values._tables.data_ptr()
    d_res = res.contiguous() if is_tensor else torch.from_numpy(np.ascontiguousarray(res)).to(dev)
    d_po = torch.from_numpy(po).to(dev) if po is not None else None
    # one buffer, one copy back: out [n][T][3] float64 | c_ev, rewards of device-resident rows [n][T][2] float64 | best_action [n][T]
    # int32 | status [n] int32
    nb_q, nb_col, nb_act = n * T * 24, (n * T * 16 if is_tensor else 0), n * T * 4
    nb_out = nb_q + nb_col
    buf = torch.empty(nb_out + nb_act + n * 4, dtype=torch.uint8, device=dev)
    if is_tensor:
        buf[nb_q:nb_out].view(torch.float64).view(n, T, 2).copy_(d_res[..., [1, 5]])
    g = values.grid.struct()
    _capi.check(L.shems_foresight_audit_dev(C.c_void_p(tab_ptr), int(values.total_rows), C.c_void_p(values.d_problems.data_ptr()),
                                            values.n_problems, C.byref(g), T, C.c_void_p(values.V.data_ptr()), values.V.numel(),
                                            C.c_void_p(d_res.data_ptr()), n, C.c_void_p(d_po.data_ptr()) if d_po is not None else None,
                                            C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + nb_out),
                                            C.c_void_p(buf.data_ptr() + nb_out + nb_act), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    host = buf.cpu().numpy()                                 # the call's one device-to-host copy (and synchronisation)
    out = host[:nb_q].view(np.float64).reshape(n, T, 3)
    cols = host[nb_q:nb_out].view(np.float64).reshape(n, T, 2) if is_tensor else res[..., [1, 5]]
    act = host[nb_out:nb_out + nb_act].view(np.int32).reshape(n, T)
    status = host[nb_out + nb_act:].view(np.int32)
    return out, act, status, np.ascontiguousarray(cols[..., 0]), np.ascontiguousarray(cols[..., 1]), po


def audit(values, results, problem_of_pass=None):
    """The hourly regret of tracked passes against the values of a solve: for every (pass, hour) the best Q over the action grid from
    the state the pass was ACTUALLY in, the Q the pass achieved and V_t at that state (the definition: csrc/shems_foresight_core.h).
    results: the reference's 23-column rows (harness.RESULTS_HEADER) of any controller's passes -- rule-based, an actor's,
    inference_many's, a foresight pass's, rows read back from a results file --, [n][T][23] or [T][23], a NumPy array or a float64
    CUDA tensor, with T = values.nsteps; pass e belongs to problem problem_of_pass[e] (None: problem 0) and must start on that
    problem's start row.  The rows of the tables come from the row array the values were solved on.  One launch on PyTorch's current
    stream (shems_foresight_audit_dev) and one device-to-host copy.  A pass whose rows do not sit on its problem's table rows (or that
    names no problem) raises BoundsError naming the first such pass.
    Regret is not a bound (see Audit).  Values from solve_horizon are accepted: best_q is then what that controller would take.
    Values solved on a forecast table, and EnsembleValues, are refused with a ValueError: an audit against a belief is not defined."""
    out, act, status, c_ev, rewards, po = _audit_device(values, results, problem_of_pass)
    bad = np.nonzero(status)[0]
    if bad.size:
        e = int(bad[0])
        hours = np.nonzero(act[e] < 0)[0]
        raise _capi.BoundsError(int(status[e]), f"foresight.audit: pass {e} (problem {0 if po is None else int(po[e])}): the rows of {hours.size} "
                                f"hour(s), the first hour {int(hours[0]) if hours.size else -1}, do not sit on its problem's table rows "
                                f"(or it names none of the {values.n_problems} problems)")
    return Audit(out, act, values.grid.targets(), rewards, _phases_of(values, c_ev, po))


def _phases_of(values, c_ev, po):
    """The EV phase of every (pass, hour): c_ev of the rows, h_countdown of the next table row read from the host copy of the row
    array the values were solved on."""
    n, T = c_ev.shape
    host = values.host_rows
    h_next = np.empty((n, T), np.float32)
    for e in range(n):
        P = values.problems[0 if po is None else int(po[e])]
        first = P.cfg.table_row0 + P.idx0                    # array row of table row idx0 + 1
        h_next[e] = host[first:first + T, 0]
    return phases(c_ev, h_next)

"""Learner groups: many INDEPENDENT DDPG learners advanced by the same launches.

The thesis protocol is 40 seeds x 10 charger profiles, each an OS process of its own running the batch-1 loop of
DDPG_reinforce_charger_v1.jl:10-47 (run scripts `RL-SHEMS/*.sh`).  Here learner l owns one slab of device memory
(networks, targets, ADAM moments, gradients, workspace, normalisation, replay ring -- all carved identically) and the
env block [l * E, (l + 1) * E) of one ShemsBatch; `shems_act_step_group_dev` / `shems_ddpg_group_*` take learner 0's
pointers plus the slab stride and run every learner in the same grid (grid z = learner for the update kernels).
Learners never exchange anything, so a group shards over GPUs as plain replicas (no collective).

Per learner the results are bit-identical to the single-learner `Agent` driven on that learner's views
(tests/test_group_gpu.py); `LearnerGroup.learners[l]` / `.rings[l]` ARE such single-learner objects on the slab.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from .ddpg import (ACTION, BATCH_SIZE, EP_LENGTH_TRAIN, ETA_ACT, ETA_CRIT, GAMMA, L1, L2, MEM_SIZE, N_ACTOR, N_CRITIC, NOISE_SIGMA, SEED_INI,
                   STATE, TAU, Agent, RingWindow, _declare, act_kernel_name, anneal_beta, is_wide, tick32, unpad_net, unpad_net_from)
from .replay import PER_COLS, PER_MAX_SLOTS, PW_IDX, PW_W, PerArgs, ReplayRing, per_workspace_floats, check_n_step, nstep_gamma


class Group(C.Structure):              # shems_group
    _fields_ = [("count", C.c_int32), ("reserved", C.c_int32), ("stride_bytes", C.c_int64), ("envs_per_learner", C.c_int64)]


class GroupW2T(C.Structure):           # shems_group_w2t
    _fields_ = [("actor", C.c_void_p), ("critic", C.c_void_p)]


class HParams(C.Structure):            # shems_group_hparams: one learner's record of a group with per-learner hyper-parameters
    _fields_ = [("eta_act", C.c_double), ("eta_crit", C.c_double), ("gamma", C.c_float), ("tau", C.c_float),
                ("noise_mu", C.c_float), ("noise_sigma", C.c_float), ("batch", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(HParams) == 40


class XParams(C.Structure):            # shems_group_xparams: one learner's exploration / ring-size record, beside its HParams
    _fields_ = [("ou_theta", C.c_float), ("ou_dt", C.c_float), ("mem_size", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(XParams) == 16

# keys of a per-learner mapping (LearnerGroup(hparams=...)); a missing key takes today's default
HPARAM_KEYS = ("eta_act", "eta_crit", "gamma", "tau", "sigma", "mu", "batch", "hidden", "noise_type", "mem_size", "theta")
GROUP_NOISE = ("gn", "ou")             # the action noise a group can draw (one kind for the whole group); "en" / "pn" run on a single Agent
MAX_GROUP_BATCH = 128                  # one update pass holds 128 minibatch columns (the group kernels have no sub-batch path)
MAX_WIDE_BATCH = 256                   # the wide form (form="wide"): one pass of P = max(128, round_up_32(max batch)) columns
WIDE_HIDDEN = (300, 600)               # the wide form's default padded hidden size: the tuned grid's widest point


def hparam_defaults(sigma=NOISE_SIGMA):
    """Today's values: what every learner of a group without hparams trains with."""
    return dict(eta_act=ETA_ACT, eta_crit=ETA_CRIT, gamma=GAMMA, tau=TAU, sigma=sigma, mu=0.0, batch=BATCH_SIZE, hidden=(L1, L2))


def _hparams_records(count, hparams, sigma, capacity, width=None, noise_type="gn", theta=0.15, n_step=1):
    """Per-learner mappings -> (full dicts, ctypes array of HParams).  Everything the group kernels cannot hold is refused here, naming the
    learner; the records themselves go through shems_group_hparams_check.  Host only: no device work.
    width: the wide form's padded hidden size -- batch up to 256 and hidden up to `width` (shems_group_hparams_check_wide).
    noise_type, theta: the group's (a record's noise_type must be the group's; its theta, "ou" groups only, defaults to the group's).
    The full dicts also carry noise_type, theta and mem_size (default: capacity) for _xparams_records.  n_step: the records' `gamma` field
    holds nstep_gamma(gamma_l, n_step), what the updates bootstrap with (the dicts keep the one-step gamma_l)."""
    hparams = list(hparams)
    if len(hparams) != count:
        raise ValueError(f"hparams holds {len(hparams)} records for a group of {count} learners")
    full = []
    for l, h in enumerate(hparams):
        if not hasattr(h, "keys"):
            raise ValueError(f"hparams[{l}]: a mapping is needed, got {type(h).__name__}")
        unknown = sorted(set(h.keys()) - set(HPARAM_KEYS))
        if unknown:
            raise ValueError(f"hparams[{l}]: unknown keys {unknown} (known: {', '.join(HPARAM_KEYS)})")
        r = hparam_defaults(sigma)
        r.update({k: v for k, v in h.items() if k not in ("noise_type", "mem_size", "theta")})
        if h.get("noise_type", noise_type) != noise_type:
            raise ValueError(f"hparams[{l}]: noise_type {h['noise_type']!r}: every learner of a group draws the group's kind of action noise "
                             f"(LearnerGroup(noise_type={noise_type!r}))")
        if "theta" in h and noise_type != "ou":
            raise ValueError(f"hparams[{l}]: theta {h['theta']} belongs to Ornstein-Uhlenbeck noise: the group draws noise_type={noise_type!r}")
        if "mem_size" in h and not 1 <= int(h["mem_size"]) <= capacity:
            raise ValueError(f"hparams[{l}]: mem_size {h['mem_size']} outside 1 .. {capacity}, the ring capacity every learner's slab is "
                             "carved for (LearnerGroup(capacity=...))")
        r["noise_type"], r["mem_size"] = noise_type, int(h.get("mem_size", capacity))
        r["theta"] = float(np.float32(h.get("theta", theta)))
        if width is None and int(r["batch"]) > MAX_GROUP_BATCH:
            raise ValueError(f"hparams[{l}]: batch {r['batch']} > {MAX_GROUP_BATCH}: the group kernels hold one 128-column update pass")
        if width is not None and int(r["batch"]) > MAX_WIDE_BATCH:
            raise ValueError(f"hparams[{l}]: batch {r['batch']} > {MAX_WIDE_BATCH}: the wide group form holds one update pass of at most "
                             f"{MAX_WIDE_BATCH} columns")
        hid = tuple(int(x) for x in r["hidden"])
        W1, W2 = (L1, L2) if width is None else width
        if len(hid) != 2 or hid[0] < 1 or hid[1] < 1 or hid[0] > W1 or hid[1] > W2:
            raise ValueError(f"hparams[{l}]: hidden {tuple(r['hidden'])} does not fit ({W1}, {W2}): " +
                             ("wider networks run on the single-learner wide path, not in a group" if width is None else
                              "wider than the wide group's hidden size"))
        r["hidden"] = hid
        r["batch"] = int(r["batch"])
        for k in ("eta_act", "eta_crit"):         # ADAM(eta) with a Float32 literal: its Float64 value (Agent.eta_*)
            r[k] = float(np.float32(r[k]))
        for k in ("gamma", "tau", "sigma", "mu"):
            r[k] = float(np.float32(r[k]))
        full.append(r)
    arr = (HParams * count)(*[HParams(r["eta_act"], r["eta_crit"], nstep_gamma(r["gamma"], n_step), r["tau"], r["mu"], r["sigma"], r["batch"], 0)
                              for r in full])
    L = _declare_group()
    rc = (L.shems_group_hparams_check(arr, count) if width is None else
          L.shems_group_hparams_check_wide(arr, count, max(r["batch"] for r in full)))
    if rc != _capi.OK:
        raise ValueError(L.shems_last_error().decode("utf-8", "replace"))
    return full, arr


def nstep_extra_blocks(n_step, envs_per_learner):
    """The (name, floats) blocks an n_step > 1 group keeps in every learner's slab behind everything else: the staging ring and the
    history of envs_per_learner households (shems_nstep).  n_step = 1: nothing.  Host only."""
    n, E = int(n_step), int(envs_per_learner)
    if n == 1:
        return ()
    return (("ns_stage_s", E * STATE), ("ns_stage_a", E * ACTION), ("ns_stage_r", E), ("ns_stage_s2", E * STATE), ("ns_stage_done", (E + 3) // 4),
            ("ns_hist_s", n * E * STATE), ("ns_hist_a", n * E * ACTION), ("ns_hist_r", n * E))


def nstep_group_refusals(form, noise_type, sized):
    """What an n_step > 1 group refuses before any device work, each by name."""
    if form == "wide":
        raise NotImplementedError("n-step learner group: form='wide' (the layer-by-layer path) has no n-step mode")
    if noise_type == "ou":
        raise NotImplementedError("n-step learner group: Ornstein-Uhlenbeck noise ('ou') runs on the *_x entry points, which read device push "
                                  "counters the fold does not keep")
    if sized:
        raise NotImplementedError("n-step learner group: per-learner mem_size runs on the *_x entry points, which read device push counters "
                                  "the fold does not keep (the rings advance in lockstep)")


PBT_FIELD_BITS = {"eta_act": 1, "eta_crit": 2, "tau": 4, "sigma": 8}       # SHEMS_PBT_*: bit k of the mask and of the draw's word y
PBT_DEFAULT_BOUNDS = {"eta_act": (1e-6, 1e-1), "eta_crit": (1e-6, 1e-1), "tau": (1e-4, 1.0), "sigma": (0.0, 10.0)}


class PBT:
    """The settings of population-based training of a learner group (Jaderberg et al. 2017; include/shems_hip.h), for
    LearnerGroup.pbt_round and run_episodes(pbt=...).  Host only: nothing here touches the device.
    populations: one id per learner; selection never crosses populations (the learners of one charger, say).
    truncation:  the share of a population that is replaced per round, and the share it draws parents from, in (0, 0.5]; kept as
                 permille = round(1000 * truncation), the quota of a population of P learners being (P * permille) // 1000.
    fields:      what explore perturbs, of "eta_act", "eta_crit", "tau", "sigma"; each by the factor `up` or `down`, picked by one
                 random bit per field, then clamped to bounds[field] = (lo, hi) (Float32 values; defaults PBT_DEFAULT_BOUNDS).
    seed:        the Philox key of the draws; None = the group's rng_seed.
    start:       run_episodes runs a round after the sweep of episode i when start <= i < num_ep; None = test_every + 1."""

    def __init__(self, populations, truncation=0.25, fields=("eta_act", "eta_crit", "tau", "sigma"), down=0.8, up=1.2, bounds=None,
                 seed=None, start=None):
        pop = np.asarray(list(populations))
        if pop.ndim != 1 or pop.size < 1 or pop.dtype.kind not in "iu":
            raise ValueError("population-based training: populations must be one integer id per learner")
        self.populations = pop.astype(np.int32)
        if not (isinstance(truncation, (int, float)) and 0.0 < float(truncation) <= 0.5):
            raise ValueError(f"population-based training: truncation = {truncation!r} outside (0, 0.5]: the parents and the children of a "
                             "round must be disjoint")
        self.truncation = float(truncation)
        self.permille = min(500, max(1, int(round(1000.0 * self.truncation))))
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        for f in fields:
            if f not in PBT_FIELD_BITS:
                raise ValueError(f"population-based training: unknown field {f!r} (explore perturbs {', '.join(PBT_FIELD_BITS)})")
        self.fields = tuple(f for f in PBT_FIELD_BITS if f in fields)
        self.mask = sum(PBT_FIELD_BITS[f] for f in self.fields)
        self.down, self.up = float(down), float(up)
        b = dict(PBT_DEFAULT_BOUNDS)
        for f, lh in (bounds or {}).items():
            if f not in PBT_FIELD_BITS:
                raise ValueError(f"population-based training: bounds: unknown field {f!r} (explore perturbs {', '.join(PBT_FIELD_BITS)})")
            b[f] = (float(lh[0]), float(lh[1]))
        self.bounds = {f: (float(np.float32(lo)), float(np.float32(hi))) for f, (lo, hi) in b.items()}
        self.seed = None if seed is None else int(seed)
        self.start = None if start is None else int(start)
        self.params(0, 0)                              # (refuses bad factors and bounds now, by shems_pbt_params_check's message)

    def params(self, round, default_seed):
        """The shems_pbt_params of round `round`, checked by shems_pbt_params_check."""
        seed = default_seed if self.seed is None else self.seed
        lo = (C.c_double * 4)(*[self.bounds[f][0] for f in PBT_FIELD_BITS])
        hi = (C.c_double * 4)(*[self.bounds[f][1] for f in PBT_FIELD_BITS])
        p = _capi.PbtParams(int(seed) & 0xFFFFFFFFFFFFFFFF, int(round) & 0xFFFFFFFF, self.permille, self.mask, 0, self.down, self.up, lo, hi)
        L = _capi.declare_pbt()
        if L.shems_pbt_params_check(C.byref(p)) != _capi.OK:
            raise ValueError("population-based training: " + L.shems_last_error().decode("utf-8", "replace"))
        return p


def pbt_group_refusals(form, hparams, noise_type, sized, populations, count):
    """What a group refuses of population-based training before any device work, each by name.  hparams: the group's full per-learner
    mappings (LearnerGroup.hparams) or None; sized: a record carries its own mem_size."""
    if form in ("latency", "wide"):
        raise NotImplementedError(f"population-based training: form={form!r} keeps no per-learner records on the throughput path; the round "
                                  "runs on a throughput group")
    if hparams is None:
        raise ValueError("population-based training: the group has no per-learner records to inherit and perturb: pass "
                         "hparams=[{}] * count to LearnerGroup")
    if noise_type == "ou":
        raise NotImplementedError("population-based training: Ornstein-Uhlenbeck noise ('ou') runs on the *_x entry points, whose second "
                                  "record array the round does not rewrite")
    if sized:
        raise NotImplementedError("population-based training: per-learner mem_size runs on the *_x entry points, whose second record array "
                                  "the round does not rewrite")
    pop = np.asarray(populations)
    if pop.shape != (int(count),):
        raise ValueError(f"population-based training: populations holds {pop.size} ids for a group of {count} learners")
    for k in sorted(set(pop.tolist())):
        hid = sorted({tuple(hparams[l]["hidden"]) for l in np.flatnonzero(pop == k)})
        if len(hid) > 1:
            raise ValueError(f"population-based training: population {k} mixes hidden sizes {hid}: a smaller network's zero padding would not "
                             "survive the copy of a wider parent")


def _xparams_records(full, capacity, dt):
    """The XParams array beside the HParams of _hparams_records' full dicts, through shems_group_xparams_check.  Host only."""
    arr = (XParams * len(full))(*[XParams(r["theta"], float(np.float32(dt)), r["mem_size"], 0) for r in full])
    L = _declare_group()
    if L.shems_group_xparams_check(arr, len(full), int(capacity)) != _capi.OK:
        raise ValueError(L.shems_last_error().decode("utf-8", "replace"))
    return arr


def _wide_width(hparams, hidden):
    """A wide group's padded hidden size: `hidden`, else the elementwise maximum of the records' (a record without one: (250, 500)), else
    WIDE_HIDDEN."""
    if hidden is not None:
        h = (int(hidden[0]), int(hidden[1]))
    elif hparams is not None and len(hparams):
        hs = [tuple(int(x) for x in (h.get("hidden", (L1, L2)) if hasattr(h, "get") else (L1, L2))) for h in hparams]
        h = (max(x[0] for x in hs), max(x[1] for x in hs))
    else:
        h = WIDE_HIDDEN
    if not (1 <= h[0] <= 4096 and 1 <= h[1] <= 4096):
        raise ValueError(f"hidden {h}: the wide path holds hidden sizes 1..4096")
    return h


def tuned_grid(job_ids, seeds=1, chargers=1, wide=False):
    """Per-learner records of a slice of the tuned template's hyper-parameter grid (input09_08_on_01-09_eval.jl:62-106), decoded by
    main.set_hyperparameters from each JOB_ID's last two digits.  Returns (records, points, skipped): `records` holds
    len(points) x seeds x chargers mappings for LearnerGroup(hparams=...), learner (p * seeds + s) * chargers + c running point points[p];
    `skipped` lists (job_id, reason) for the points a group cannot run (BATCH_SIZE 150, (L1, L2) = (300, 600)).
    wide: records for a LearnerGroup(form="wide"), which holds every batch and hidden size of the grid: nothing is skipped for them."""
    from .main import RunConfig, set_hyperparameters
    records, points, skipped = [], [], []
    for jid in job_ids:
        jid = str(jid)
        cfg = set_hyperparameters(RunConfig(job_id=jid.zfill(2), task_id="0", gpu_id=0, template="tuned"))
        why = []
        if cfg.BATCH_SIZE > (MAX_WIDE_BATCH if wide else MAX_GROUP_BATCH):
            why.append(f"BATCH_SIZE {cfg.BATCH_SIZE} > {MAX_WIDE_BATCH if wide else MAX_GROUP_BATCH}")
        if not wide and (cfg.L1 > L1 or cfg.L2 > L2):
            why.append(f"(L1, L2) = ({cfg.L1}, {cfg.L2}) wider than ({L1}, {L2})")
        if cfg.noise_type != "gn":
            why.append(f"noise_type {cfg.noise_type!r}")
        if why:
            skipped.append((jid, "; ".join(why)))
            continue
        rec = dict(eta_act=float(np.float32(cfg.eta_act)), eta_crit=float(np.float32(cfg.eta_crit)), gamma=float(np.float32(cfg.gamma)),
                   tau=float(np.float32(cfg.tau)), sigma=float(cfg.noise_act), mu=0.0, batch=int(cfg.BATCH_SIZE), hidden=(cfg.L1, cfg.L2))
        points.append(jid)
        records += [dict(rec) for _ in range(int(seeds) * int(chargers))]
    return records, points, skipped


def input_grid(job_ids, seeds=1, chargers=1):
    """tuned_grid's twin for the template "input" (RL-SHEMS/input.jl:58-100): 27 points over MEM_SIZE, BATCH_SIZE and (L1, L2, gamma,
    sigma, theta), every one with noise_type = "ou".  Returns (records, points): `records` holds len(points) x seeds x chargers mappings
    (eta_*, gamma, tau, sigma, mu = 0, theta, batch, hidden, mem_size, noise_type = "ou"), learner (p * seeds + s) * chargers + c running
    point points[p], for LearnerGroup(form="wide", noise_type="ou", capacity=INPUT_CAPACITY, hparams=records).  Only the 27 codes 00-26
    are points of the grid: anything else is refused."""
    from .main import RunConfig, set_hyperparameters
    records, points = [], []
    for jid in job_ids:
        jid = str(jid)
        if not jid.isdigit() or not 0 <= int(jid[-2:]) <= 26:
            raise ValueError(f"JOB_ID {jid!r}: the input template's grid has the 27 points 00 .. 26 (three ternary digits)")
        cfg = set_hyperparameters(RunConfig(job_id=jid.zfill(2), task_id="0", gpu_id=0, template="input"))
        rec = dict(eta_act=float(np.float32(cfg.eta_act)), eta_crit=float(np.float32(cfg.eta_crit)), gamma=float(np.float32(cfg.gamma)),
                   tau=float(np.float32(cfg.tau)), sigma=float(cfg.sigma), mu=0.0, theta=float(cfg.theta), batch=int(cfg.BATCH_SIZE),
                   hidden=(cfg.L1, cfg.L2), mem_size=int(cfg.MEM_SIZE), noise_type=cfg.noise_type)
        points.append(jid)
        records += [dict(rec) for _ in range(int(seeds) * int(chargers))]
    return records, points


INPUT_ALL = tuple(f"{c:02d}" for c in range(27))       # every point of the input template's grid
INPUT_CAPACITY = 30000                                 # its largest MEM_SIZE: what a group of the grid carves every ring for

TUNED_RUNNABLE = tuple(f"{c:02d}" for c in range(81) if c // 27 != 2 and (c // 3) % 3 != 0)   # the 36 points tuned_grid keeps
TUNED_ALL = tuple(f"{c:02d}" for c in range(81))                                             # every point: tuned_grid(..., wide=True)


W2T_FLOATS = 32 * 4 * 64 * 64          # SHEMS_W2T_FLOATS: [4 k-tiles][8 n-tiles][m | v | p | target][64][64] per network


def _declare_group():
    L = _declare()
    if getattr(L, "_group_declared", False):
        return L
    vp, i64 = C.c_void_p, C.c_int64
    from .ddpg import ActParams, DdpgArgs
    PD, PG, PR, PT = C.POINTER(DdpgArgs), C.POINTER(Group), C.POINTER(_capi.Replay), C.POINTER(GroupW2T)
    L.shems_act_step_group_dev.argtypes = [C.POINTER(_capi.View), C.POINTER(ActParams), PG, PT, vp, vp, vp, PR, C.POINTER(RingWindow), vp]
    dbl = C.c_double
    L.shems_group_w2_to_tiled.argtypes = [PD, PG, PT, vp]
    L.shems_group_w2_to_flux.argtypes = [PD, PG, PT, vp]
    L.shems_act_step_group_kernel.argtypes = [i64, i64, C.c_int, C.c_char_p, C.c_int32]
    for fn in ("shems_group_w2_to_tiled", "shems_group_w2_to_flux", "shems_act_step_group_kernel"):
        getattr(L, fn).restype = C.c_int
    L.shems_ddpg_group_update.argtypes = [PD, PR, PG, i64, C.c_uint64, C.c_uint32, dbl, dbl, dbl, dbl, dbl, dbl, vp]
    L.shems_ddpg_group_update.restype = C.c_int
    L.shems_ddpg_group_update_tp.argtypes = [PD, PR, PG, PT, vp, i64, C.c_uint64, C.c_uint32, dbl, dbl, dbl, dbl, dbl, dbl, C.c_int32, vp]
    L.shems_ddpg_group_update_tp.restype = C.c_int
    L.shems_ddpg_group_critic_grad.argtypes = [PD, PR, PG, i64, C.c_uint64, C.c_uint32, vp]
    L.shems_ddpg_group_critic_apply.argtypes = [PD, PG, C.c_double, C.c_double, C.c_double, vp]
    L.shems_ddpg_group_actor_grad.argtypes = [PD, PG, vp]
    L.shems_ddpg_group_actor_apply.argtypes = [PD, PG, C.c_double, C.c_double, C.c_double, vp]
    L.shems_minmax_group_dev.argtypes = [PR, PG, i64, i64, C.c_uint64, vp, vp, vp]
    L.shems_group_hparams_check.argtypes = [C.POINTER(HParams), C.c_int32]
    i32 = C.c_int32
    L.shems_group_hparams_check_wide.argtypes = [C.POINTER(HParams), i32, i32]
    L.shems_wide_group_workspace_floats.argtypes = [i32, i32, i32, C.POINTER(i64)]
    L.shems_wide_group_update.argtypes = [PD, PR, PG, i32, i32, vp, i32, i64, C.c_uint64, C.c_uint32, dbl, dbl, dbl, dbl, dbl, dbl, vp]
    L.shems_wide_act_step_group_dev.argtypes = [C.POINTER(_capi.View), C.POINTER(ActParams), PG, i32, i32, vp, vp, vp, vp, PR, C.POINTER(RingWindow), vp]
    for fn in ("shems_group_hparams_check", "shems_group_hparams_check_wide",
               "shems_wide_group_workspace_floats", "shems_wide_group_update", "shems_wide_act_step_group_dev"):
        getattr(L, fn).restype = C.c_int
    PX, u64, u32 = C.POINTER(XParams), C.c_uint64, C.c_uint32
    L.shems_group_xparams_check.argtypes = [PX, i32, i64]
    L.shems_act_step_group_x_dev.argtypes = [C.POINTER(_capi.View), C.POINTER(ActParams), PG, PT, vp, vp, vp, vp, vp, PR, C.POINTER(RingWindow), vp]
    L.shems_wide_act_step_group_x_dev.argtypes = [C.POINTER(_capi.View), C.POINTER(ActParams), PG, i32, i32, vp, vp, vp, vp, vp, vp, PR,
                                                  C.POINTER(RingWindow), vp]
    L.shems_ddpg_group_update_tp_x.argtypes = [PD, PR, PG, PT, vp, vp, vp, u64, u32, dbl, dbl, dbl, dbl, dbl, dbl, i32, vp]
    L.shems_wide_group_update_x.argtypes = [PD, PR, PG, i32, i32, vp, vp, vp, i32, u64, u32, dbl, dbl, dbl, dbl, dbl, dbl, vp]
    for fn in ("shems_group_xparams_check", "shems_act_step_group_x_dev", "shems_wide_act_step_group_x_dev", "shems_ddpg_group_update_tp_x",
               "shems_wide_group_update_x"):
        getattr(L, fn).restype = C.c_int
    L.shems_group_eval_best_dev.argtypes = [PD, PG, PT, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]
    L.shems_group_eval_best_dev.restype = C.c_int
    for fn in ("shems_ddpg_group_clone_update_tp", "shems_ddpg_group_critic_update_tp"):
        getattr(L, fn).argtypes = [PD, PR, i64, PG, PT, vp, i64, u64, u32, dbl, dbl, dbl, i32, vp]
        getattr(L, fn).restype = C.c_int
    for fn in ("shems_act_step_group_dev", "shems_ddpg_group_critic_grad", "shems_ddpg_group_critic_apply",
               "shems_ddpg_group_actor_grad", "shems_ddpg_group_actor_apply", "shems_minmax_group_dev"):
        getattr(L, fn).restype = C.c_int
    L._group_declared = True
    return L


def group_act_kernel_name(n_envs, envs_per_learner, tiled):
    """The kernel the fused-step dispatcher runs for a learner group, by its profiler name (shems_act_step_group_kernel)."""
    L = _declare_group()
    buf = C.create_string_buffer(96)
    _capi.check(L.shems_act_step_group_kernel(int(n_envs), int(envs_per_learner), 1 if tiled else 0, buf, 96))
    return buf.value.decode()


def _pad4(n):
    return (int(n) + 3) & ~3


def slab_layout(n_actor, n_critic, ws_floats, capacity, tiled, extra=()):
    """One learner's slab: ({name: (float offset, floats)}, slab_floats).  Every block starts on a 16-byte boundary (float offsets are
    multiples of 4).  extra: further (name, floats) blocks of a subclass (LearnerGroup._extra_blocks), carved AFTER ring_done, so that
    no offset of a DDPG group depends on them.  Host only: no device work."""
    layout, off = {}, 0
    for name, n in (("actor", n_actor), ("critic", n_critic), ("actor_t", n_actor), ("critic_t", n_critic),
                    ("m_actor", n_actor), ("v_actor", n_actor), ("m_critic", n_critic), ("v_critic", n_critic),
                    ("w2t_actor", W2T_FLOATS if tiled else 0), ("w2t_critic", W2T_FLOATS if tiled else 0),
                    ("grad_actor", n_actor), ("grad_critic", n_critic), ("s_min", STATE), ("s_max", STATE), ("losses", 2),
                    ("ws", ws_floats), ("ring_s", capacity * STATE), ("ring_a", capacity * ACTION),
                    ("ring_r", capacity), ("ring_s2", capacity * STATE), ("ring_done", (capacity + 3) // 4), *extra):
        if name in layout:
            raise ValueError(f"slab_layout: block {name!r} twice")
        layout[name] = (off, int(n))
        off = _pad4(off + n)
    return layout, off


class LearnerGroup:
    """`count` independent learners, learner l seeded with (seed + l) for its network initialisation and (rng_seed + l)
    for its minibatch stream; exploration noise is keyed per env, so it differs between learners by construction."""

    # replay() of a group: "throughput" = csrc/shems_gupd.hip (eight launches shaped for hundreds of learners: small tiles, four workgroups
    # resident per CU, plain back-propagation), "latency" = the single-learner kernels with grid z = learner (five launches, per learner
    # bit-identical to Agent.replay), "wide" = the layer-by-layer path of csrc/shems_wide.hip with a learner dimension (24 launches; networks
    # up to 4096 wide, batches up to 256).  Default: throughput from TP_MIN_LEARNERS learners up.
    TP_MIN_LEARNERS = 16
    has_evaluate = True                    # evaluate() exists (imitation.warm_start_group asks before it trains anything)

    def __init__(self, count, envs_per_learner, seed=1231, rng_seed=None, capacity=MEM_SIZE, sigma=NOISE_SIGMA, device=None, form=None, tiled=None,
                 hparams=None, hidden=None, noise_type="gn", theta=0.15, dt=1e-2, n_step=1):
        """tiled (throughput form only; default on, SHEMS_GROUP_TILED=0 switches it off): the layer-2 state of both networks (W2, its
        ADAM moments, the target's W2) is kept in the TILED working layout (shems_group_w2t, include/shems_hip.h) while the group trains:
        one contiguous 64 KB piece per 64 x 64 tile for the update's W2-gradient / ADAM launches (4.78 against 3.85 TB/s), read from
        there by the forward / D1 launches and by the fused act/step launch.  The Flux-order blocks -- what `learners[l].actor` etc. ARE --
        keep everything else and are the API's view of W2: `flux_()` brings their W2 ranges up to date (call it before reading a learner's
        tensors, evaluating a learner through its Agent, or saving), `Agent.set_params` on a learner of the group is noticed by itself,
        any other write into those tensors must be followed by `flux_changed()`.

        hparams: None (every learner trains with today's shared values), or `count` mappings, learner l's with
        the keys of HPARAM_KEYS (eta_act, eta_crit, gamma, tau, sigma, mu, batch, hidden; a missing key takes today's default): the group
        then runs the throughput form whatever its size, with the records as the entry points' d_hp (shems_ddpg_group_update_tp,
        shems_act_step_group_dev), and learners[l] carries learner l's values.  The records are checked and uploaded once, here.
        Refused, naming the learner: batch > 128, hidden wider than (250, 500), a noise_type other than the group's, theta in a "gn"
        group, mem_size outside 1 .. capacity.

        noise_type, theta, dt (as Agent's): the action noise of the whole group, "gn" (GNoise) or "ou" (OUNoise, DDPG.jl:49-55: X +=
        theta (mu - X) dt + sigma sqrt(dt) z per env, the state in `ou_state` [n_envs][2], zeros at first and kept across episodes; a
        record's theta / sigma / mu are its learner's).  "en" and "pn" stay a single Agent's.  A record's mem_size (1 .. capacity) is
        its learner's ring size: rings[l] is a ReplayRing(mem_size_l) over the first mem_size_l slots of the ring arrays, which stay
        carved for `capacity`.  An "ou" group, or one with a mem_size record, runs the throughput or the wide form on the *_x entry
        points (shems_act_step_group_x_dev, shems_ddpg_group_update_tp_x and their wide twins): the records (built from the shared
        values when none were given), a second record array (XParams) and the device array `pushed` [count] int64, which holds every
        ring's push count -- a launch's window position is ignored there, learner l's remembered env at window position rel goes to
        slot (pushed[l] + rel) mod mem_size_l and its minibatch indexes x mod min(pushed[l], mem_size_l).  `pushed` is uploaded
        whenever the rings' host counters moved without the group (populate_memory, a test) and advanced on the stream by every step
        that remembers.  form="latency" takes neither.

        form="wide": the learners run on the layer-by-layer path (csrc/shems_wide.hip), batched over learners -- every launch runs the
        whole group.  All networks are zero-padded into one hidden size, `hidden` (default: the elementwise maximum of the records'
        hidden, or (300, 600) without records; up to 4096); a record may then hold batch up to 256 and any hidden size up to `hidden`.
        learners[l] is learner l's wide Agent at its own size (export_* / set_params).  Without hparams every learner trains with
        learners[0]'s batch (<= 128), gamma, tau and eta.  No tiled layout.

        n_step (1 .. 16): multi-step returns (include/shems_hip.h).  With n_step > 1 every learner's slab also holds a
        staging ring and the history of envs_per_learner households, carved behind the subclass's blocks (no existing offset moves; an
        n_step = 1 group carves nothing); ring_window is the stationary (window_count, 0); act_step writes the window into the staging
        rings and nstep_fold(hour) -- one launch for the group -- pushes from hour n_step - 1 on; the records (and learners[l].gamma_n)
        carry gamma_l^n, learners[l].gamma stays gamma_l.  Refused by name: form="wide", "ou" noise, per-learner mem_size."""
        import os
        import torch
        self.torch = torch
        self.L = _declare_group()
        self.count, self.envs_per_learner, self.capacity = int(count), int(envs_per_learner), int(capacity)
        self.hparams, self._hp_host, self._hp_dev = None, None, None
        self._xp_host, self._xp_dev, self._pushed_dev, self._pushed_host, self.ou_state = None, None, None, None, None
        self.hidden = None                         # form "wide": the padded hidden size of every learner's networks
        if noise_type not in GROUP_NOISE:          # every argument error before any device work
            raise ValueError(f"noise_type {noise_type!r}: a learner group draws \"gn\" or \"ou\" action noise (\"en\" and \"pn\" run on a single Agent)")
        self.noise_type, self.theta, self.dt = noise_type, float(theta), float(dt)
        ou = noise_type == "ou"
        if hparams is not None:
            hparams = list(hparams)
        sized = hparams is not None and any(hasattr(h, "keys") and "mem_size" in h for h in hparams)
        self.n_step = check_n_step(n_step)
        if self.n_step > 1:
            nstep_group_refusals(form, noise_type, sized)
        self._x = ou or sized                      # the *_x entry points: per-learner OU noise / ring sizes
        if self._x and form == "latency":
            raise ValueError("Ornstein-Uhlenbeck noise and per-learner mem_size run on the throughput or the wide form: form='latency' takes neither")
        rec_kw = dict(noise_type=noise_type, theta=self.theta, n_step=self.n_step)
        if form == "wide":
            if tiled:
                raise ValueError("form='wide' has no tiled working layout: tiled=True is refused")
            tiled = False
            self.hidden = _wide_width(hparams, hidden)
            if hparams is None and self._x:        # uniform records: the bits of the shared values
                hparams = [{"hidden": self.hidden} for _ in range(max(self.count, 0))]
            if hparams is not None:
                if self.count < 1:
                    raise ValueError("a learner group needs count >= 1")
                self.hparams, self._hp_host = _hparams_records(self.count, hparams, sigma, self.capacity, width=self.hidden, **rec_kw)
        elif hidden is not None:
            raise ValueError("hidden= belongs to form='wide'")
        elif hparams is not None or self._x:
            if form == "latency":
                raise ValueError("per-learner hyper-parameters run on the throughput form: form='latency' cannot take hparams")
            if self.count < 1:
                raise ValueError("a learner group needs count >= 1")
            self.hparams, self._hp_host = _hparams_records(self.count, hparams if hparams is not None else [{} for _ in range(self.count)], sigma,
                                                           self.capacity, **rec_kw)
            form = "throughput"
        if self._x:
            self._xp_host = _xparams_records(self.hparams, self.capacity, self.dt)
        self.mem_sizes = [r["mem_size"] for r in self.hparams] if self.hparams is not None else [self.capacity] * max(self.count, 0)
        self.form = form if form is not None else ("throughput" if self.count >= self.TP_MIN_LEARNERS else "latency")
        if self.form not in ("throughput", "latency", "wide"):
            raise ValueError("form must be 'throughput', 'latency' or 'wide'")
        self.store_grad = False                    # throughput form: also leave the gradients in grad_actor / grad_critic (tests)
        self.fused = True                          # latency form: one call (False: the four split calls, the same bits)
        self.tiled = (self.form == "throughput" and os.environ.get("SHEMS_GROUP_TILED", "1") != "0") if tiled is None else bool(tiled)
        if self.tiled and self.form != "throughput":
            raise ValueError("the tiled working layout belongs to the throughput form")
        self._flux_valid, self._tiled_valid = True, False          # which copy of the layer-2 state is current (both may be)
        if self.count < 1 or self.envs_per_learner < 32 or self.envs_per_learner % 32 != 0:
            raise ValueError("a learner group needs count >= 1 and envs_per_learner a multiple of 32")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.seed = int(seed)
        self.rng_seed = self.seed if rng_seed is None else int(rng_seed)
        nws = C.c_int64(0)
        n_actor, n_critic = N_ACTOR, N_CRITIC
        if self.form == "wide":                    # the slab carved at the group's width, ws for its pass width
            self.max_batch = max(r["batch"] for r in self.hparams) if self.hparams is not None else MAX_GROUP_BATCH
            na, nc = C.c_int64(0), C.c_int64(0)
            _capi.check(self.L.shems_wide_params(*self.hidden, C.byref(na), C.byref(nc)))
            n_actor, n_critic = na.value, nc.value
            _capi.check(self.L.shems_wide_group_workspace_floats(*self.hidden, self.max_batch, C.byref(nws)))
        else:
            _capi.check(self.L.shems_ddpg_workspace_floats(C.byref(nws)))
        self._act_ws = None                        # form "wide": scratch of the fused step (shems_wide_act_workspace_floats)
        # one slab per learner (slab_layout); a subclass appends blocks of its own behind the ring
        layout, off = slab_layout(n_actor, n_critic, nws.value, self.capacity, self.tiled,
                                  (*self._extra_blocks(n_critic), *nstep_extra_blocks(self.n_step, self.envs_per_learner)))
        self.layout, self.slab_floats = layout, off
        self.slab = torch.zeros((self.count, self.slab_floats), dtype=torch.float32, device=self.device)
        self.learners, self.rings = [], []
        for l in range(self.count):
            v = lambda name: self.slab[l, layout[name][0]:layout[name][0] + layout[name][1]]
            tens = {k: v(k) for k in ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic",
                                      "grad_actor", "grad_critic", "s_min", "s_max", "ws", "losses")}
            wkw = dict(wide=True, layout=self.hidden) if self.form == "wide" else {}
            if self.hparams is None:
                self.learners.append(Agent(seed=self.seed + l, rng_seed=self.rng_seed + l, sigma=sigma, device=self.device, tensors=tens,
                                           n_step=self.n_step, **(dict(wkw, hidden=self.hidden) if wkw else {})))
            else:                                  # smaller networks come zero-padded (ddpg.pad_net / pad_net_to) and stay so under training
                h = self.hparams[l]
                ag = Agent(seed=self.seed + l, rng_seed=self.rng_seed + l, sigma=h["sigma"], mu=h["mu"], device=self.device, tensors=tens,
                           hidden=h["hidden"], n_step=self.n_step, **wkw)
                ag.gamma, ag.tau, ag.batch, ag.eta_act, ag.eta_crit = h["gamma"], h["tau"], h["batch"], h["eta_act"], h["eta_crit"]
                ag.noise_type, ag.theta, ag.dt = self.noise_type, h["theta"], self.dt
                self.learners.append(ag)
            if self.tiled:
                self.learners[-1]._before_param_write = self._before_flux_write
            m = self.mem_sizes[l]                  # the learner's ring: the first mem_size slots of arrays carved for `capacity`
            done = v("ring_done").view(torch.uint8)[:m]
            self.rings.append(ReplayRing(m, tensors=(v("ring_s").view(self.capacity, STATE)[:m], v("ring_a").view(self.capacity, ACTION)[:m],
                                                     v("ring_r")[:m], v("ring_s2").view(self.capacity, STATE)[:m], done)))
        if self._hp_host is not None:              # the records, once, in a small device buffer the group owns
            raw = np.frombuffer(bytes(self._hp_host), dtype=np.uint8).copy()
            self._hp_dev = torch.from_numpy(raw).to(self.device)
        self._gamma1_dev, self._ns_window = None, None
        if self.n_step > 1:
            self.LN = _capi.declare_nstep()
            if self.hparams is not None:           # the fold's one-step discounts (the records hold gamma_l^n)
                self._gamma1_dev = torch.tensor([r["gamma"] for r in self.hparams], dtype=torch.float32).to(self.device)
        if self._x:
            raw = np.frombuffer(bytes(self._xp_host), dtype=np.uint8).copy()
            self._xp_dev = torch.from_numpy(raw).to(self.device)
            self._pushed_dev = torch.zeros(self.count, dtype=torch.int64, device=self.device)
            self._pushed_host = [0] * self.count
            if self.noise_type == "ou":            # OUNoise.X = zeros(Float32, 2) per env; kept across episodes, as Agent.ou_state
                self.ou_state = torch.zeros((self.n_envs, ACTION), dtype=torch.float32, device=self.device)
        self.updates = 0
        self.clones = 0                            # grouped supervised updates (clone); they advance bp_actor, not `updates`
        self.evaluations = 0                       # grouped critic-only updates (evaluate); they advance bp_critic, not `updates`
        self._hp_variants = {}                     # record arrays of clone / evaluate with a tau of the call's: built once per (kind, tau)
        self.tick = 0

    def _extra_blocks(self, n_critic):
        """(name, floats) blocks a subclass keeps in every learner's slab, carved after ring_done (td3.TD3LearnerGroup: the second
        critic).  Called once by __init__ after form / tiled are decided."""
        return ()

    # ---- population-based training (include/shems_hip.h) ---------------------------------------------------------------
    def _pbt_blocks(self):
        """Names of the subclass's slab blocks a child inherits from its parent besides the LearnerGroup's own (td3.TD3LearnerGroup: the
        second critic's parameters, target, moments and tiles)."""
        return ()

    def pbt_ranges(self):
        """The (float offset, floats) ranges of a learner's slab that a child takes over from its parent, adjacent ones merged: the
        contiguous prefix actor .. w2t_critic (parameters, targets, ADAM moments, both tiled regions), s_min and s_max, and the blocks of
        _pbt_blocks().  Never the gradients, workspaces, losses, the ring, priorities or the n-step staging and history.  Host only."""
        lay = self.layout
        spans = [(0, lay["grad_actor"][0]), (lay["s_min"][0], lay["losses"][0] - lay["s_min"][0])]
        spans += [(lay[name][0], _pad4(lay[name][1])) for name in self._pbt_blocks()]
        merged = []
        for o, n in sorted(s for s in spans if s[1] > 0):
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1] = (merged[-1][0], merged[-1][1] + n)
            else:
                merged.append((o, n))
        if len(merged) > _capi.PBT_MAX_RANGES:
            raise ValueError(f"pbt_ranges: {len(merged)} ranges; one copy launch takes {_capi.PBT_MAX_RANGES}")
        return merged

    def pbt_round(self, scores, pbt, round):
        """One round of population-based training on `scores` (float64 [count], a device tensor such as GroupRun._score, or anything
        torch.as_tensor takes): two launches with no host decision in between -- shems_pbt_select_dev ranks every population, draws each
        child's parent and writes the child's inherited and perturbed record in place; shems_pbt_copy_dev moves pbt_ranges() from every
        parent's slab to its children's -- then ONE small copy brings the records and `parent` back and every host mirror follows:
        hparams[l] (gamma from the parent's mapping: the record holds gamma^n), learners[l].eta_act / eta_crit / tau / sigma / mu /
        batch / gamma, the host records, an n-step group's one-step discounts; the record variants of clone / evaluate / TD3's hold are
        dropped and rebuilt from the new values when next asked for.  A child keeps its own ring (and priorities, n-step history,
        workspaces, random streams: it goes on with seed + l); both layouts of the layer-2 state are copied, so flux_() state is as
        before.  Returns parent, int32 [count] (parent[l] == l: kept)."""
        pbt_group_refusals(self.form, self.hparams, self.noise_type, self._x, pbt.populations, self.count)
        t = self.torch
        LB = _capi.declare_pbt()
        st = getattr(self, "_pbt_dev", None)
        if st is None or st[0] is not pbt:             # the population ids and the two outputs, once per PBT object
            ranges = self.pbt_ranges()
            st = (pbt, t.from_numpy(pbt.populations.copy()).to(self.device), t.zeros(self.count, dtype=t.int32, device=self.device),
                  t.zeros(self.count, dtype=t.int32, device=self.device), (_capi.PbtRange * len(ranges))(*[_capi.PbtRange(o, n) for o, n in ranges]))
            self._pbt_dev = st
        _, d_pop, d_parent, d_rank, ranges = st
        sc = t.as_tensor(scores, dtype=t.float64).to(self.device).contiguous()
        if sc.shape != (self.count,):
            raise ValueError(f"pbt_round: scores must hold one float64 per learner ({self.count}), got {tuple(sc.shape)}")
        params, g = pbt.params(round, self.rng_seed), self.struct()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        _capi.check(LB.shems_pbt_select_dev(C.byref(params), self.count, ptr(d_pop), ptr(sc), self._hp_ptr(), ptr(d_parent), ptr(d_rank),
                                            self._stream()))
        _capi.check(LB.shems_pbt_copy_dev(ptr(self.slab), C.byref(g), ranges, len(ranges), ptr(d_parent), self._stream()))
        host = t.cat([self._hp_dev, d_parent.view(t.uint8)]).cpu().numpy()                 # the round's one copy
        nb = C.sizeof(HParams) * self.count
        recs = (HParams * self.count).from_buffer_copy(host[:nb].tobytes())
        parent = host[nb:].view(np.int32).copy()
        old = [dict(h) for h in self.hparams]
        for l in np.flatnonzero(parent != np.arange(self.count)):
            l, r = int(l), recs[int(l)]
            h = dict(self.hparams[l], gamma=old[int(parent[l])]["gamma"], eta_act=r.eta_act, eta_crit=r.eta_crit, tau=float(r.tau),
                     sigma=float(r.noise_sigma), mu=float(r.noise_mu), batch=int(r.batch))
            self.hparams[l] = h
            ag = self.learners[l]
            ag.gamma, ag.tau, ag.batch, ag.eta_act, ag.eta_crit = h["gamma"], h["tau"], h["batch"], h["eta_act"], h["eta_crit"]
            ag.sigma, ag.mu = h["sigma"], h["mu"]
        self._hp_host = recs
        if self._gamma1_dev is not None:
            self._gamma1_dev.copy_(t.tensor([h["gamma"] for h in self.hparams], dtype=t.float32))
        self._hp_variants = {}
        self.pbt_rank = d_rank                         # the last round's ranks (device int32 [count]), for a log
        return parent

    def _hp_ptr(self):
        """The entry points' d_hp: the device records, or NULL (the shared values)."""
        return C.c_void_p(self._hp_dev.data_ptr()) if self._hp_dev is not None else None

    def _x_ptrs(self):
        """The *_x entry points' (d_xp, d_pushed).  `pushed` must hold [ring.pushed for ring in rings] when a launch reads it: the host
        counters are compared with what the device array was last given (no device work) and uploaded if they moved without the group."""
        now = [int(r.pushed) for r in self.rings]
        if now != self._pushed_host:
            self._pushed_dev.copy_(self.torch.tensor(now, dtype=self.torch.int64), non_blocking=False)
            self._pushed_host = now
        return C.c_void_p(self._xp_dev.data_ptr()), C.c_void_p(self._pushed_dev.data_ptr())

    # ---- multi-step returns ---------------------------------------------------------------------------------------------------------
    def _ns_view(self, l, name):
        o, n = self.layout[name]
        return self.slab[l, o:o + n]

    def stage_of(self, l):
        """Learner l's staging ring (n_step > 1): the one-step transitions of its window's households as the last training step left
        them, a ReplayRing over envs_per_learner slots (slot j = household j of the learner's block)."""
        E, v = self.envs_per_learner, lambda name: self._ns_view(l, name)
        return ReplayRing(E, tensors=(v("ns_stage_s").view(E, STATE), v("ns_stage_a").view(E, ACTION), v("ns_stage_r"),
                                      v("ns_stage_s2").view(E, STATE), v("ns_stage_done").view(self.torch.uint8)[:E]))

    def nstep_fold(self, hour):
        """shems_nstep_group_fold_dev behind the training step of hour `hour` of the episode: one launch folds every learner's staging
        window (the count of the last act_step) into its history and, from hour n_step - 1 on, pushes it into its ring; the rings'
        push counters advance only then.  Returns True when it pushed."""
        if self.n_step == 1 or self._ns_window is None:
            raise ValueError("nstep_fold: an n_step > 1 group folds behind an act_step with a window")
        wc = self._ns_window
        p = lambda name: self.slab.data_ptr() + 4 * self.layout[name][0]
        ns = _capi.NStepArgs(self.n_step, 0, wc, float(np.float32(self.learners[0].gamma)), 0, p("ns_hist_s"), p("ns_hist_a"), p("ns_hist_r"))
        s0, r0, g = self.stage_of(0).struct(), self._ring0(), self.struct()
        g1 = C.c_void_p(self._gamma1_dev.data_ptr()) if self._gamma1_dev is not None else None
        _capi.check(self.LN.shems_nstep_group_fold_dev(C.byref(ns), C.byref(s0), C.byref(r0), C.byref(g), g1, self.rings[0].pos, int(hour),
                                                       self._stream()))
        pushed = int(hour) >= self.n_step - 1
        if pushed:
            for ring in self.rings:
                ring.pushed += wc
        return pushed

    def _ring0(self):
        """The entry points' ring0: learner 0's ring arrays with the capacity they are carved for (rings[0] may use a prefix of them)."""
        r0 = self.rings[0].struct()
        r0.capacity = self.capacity
        return r0

    # ------------------------------------------------------------------
    def struct(self):
        return Group(self.count, 0, self.slab_floats * 4, self.envs_per_learner)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    # ---- the tiled working layout of the layer-2 state -----------------------------------------------------------------------------
    def w2t_struct(self):
        base = self.slab.data_ptr()
        return GroupW2T(base + 4 * self.layout["w2t_actor"][0], base + 4 * self.layout["w2t_critic"][0])

    def _use_tiled(self):
        """Before a launch that reads / writes the tiled regions: bring them up to date from the Flux-order blocks if those were written."""
        if self.tiled and self.form != "throughput":
            self.flux_()                               # the form was switched on a tiled group: the latency form speaks Flux order
            self._tiled_valid = False
            return False
        if not self.tiled:
            if not self._flux_valid:                   # (the flag was switched off on a group whose current layer-2 state is in the tiles)
                raise RuntimeError("this group's Flux-order blocks are stale: call flux_() while it is still tiled")
            return False
        if not self._tiled_valid:
            d, g, t = self.learners[0]._ddpg_args(), self.struct(), self.w2t_struct()
            _capi.check(self.L.shems_group_w2_to_tiled(C.byref(d), C.byref(g), C.byref(t), self._stream()))
            self._tiled_valid = True
        return True

    def flux_(self):
        """Bring the W2 ranges of the Flux-order blocks (learners[l].actor / critic / actor_t / critic_t / m_* / v_*) up to date."""
        if self.tiled and not self._flux_valid:
            d, g, t = self.learners[0]._ddpg_args(), self.struct(), self.w2t_struct()
            _capi.check(self.L.shems_group_w2_to_flux(C.byref(d), C.byref(g), C.byref(t), self._stream()))
            self._flux_valid = True
        return self

    def flux_changed(self):
        """The caller wrote into Flux-order tensors of the group (after flux_()): the tiled regions are re-made before their next use."""
        if self.tiled and not self._flux_valid:
            raise RuntimeError("flux_changed(): the Flux-order blocks were stale when they were written -- call flux_() before writing into them")
        self._tiled_valid = False
        return self

    def _before_flux_write(self):
        self.flux_()
        self._tiled_valid = False

    @property
    def n_envs(self):
        return self.count * self.envs_per_learner

    def populate_memory(self, env, seed=None):
        """populate_memory (MPS:9-29) per learner on its own env block (learner l: seed + l)."""
        seed = self.rng_seed if seed is None else int(seed)
        E = self.envs_per_learner
        scratch = None
        if self.n_step > 1:                        # every learner converts through one shared scratch ring (Agent.populate_memory_nstep)
            m = env.maxsteps - self.n_step + 1
            if m < 1:
                raise ValueError(f"populate_memory: num_steps = {env.maxsteps} < n_step = {self.n_step}: an episode must hold one full window")
            scratch = ReplayRing(min(E, -(-self.capacity // m)) * env.maxsteps, device=self.device)
        for l, (ag, ring) in enumerate(zip(self.learners, self.rings)):
            if self.n_step > 1:
                ag.populate_memory_nstep(env.slice(l * E, E), ring, seed=seed + l, scratch=scratch)
            else:
                ag.populate_memory(env.slice(l * E, E), ring, seed=seed + l)
        return self

    def min_max_buffer(self, count=None, seed=None):
        """min_max_buffer (MPS:50-53) for every learner in one launch (learner l: Philox key seed + l)."""
        g, r0 = self.struct(), self._ring0()
        seed = self.rng_seed if seed is None else int(seed)
        lens = [len(r) for r in self.rings]
        if len(set(lens)) == 1:
            n, a0 = lens[0], self.learners[0]
            _capi.check(self.L.shems_minmax_group_dev(C.byref(r0), C.byref(g), n, n if count is None else int(count), seed,
                                                      C.c_void_p(a0.s_min.data_ptr()), C.c_void_p(a0.s_max.data_ptr()), self._stream()))
            return self
        one = Group(1, 0, 0, self.envs_per_learner)        # rings of different lengths: the same launch per learner, on its own length
        for l, (ag, ring, n) in enumerate(zip(self.learners, self.rings, lens)):
            rl = ring.struct()
            _capi.check(self.L.shems_minmax_group_dev(C.byref(rl), C.byref(one), n, n if count is None else int(count), seed + l,
                                                      C.c_void_p(ag.s_min.data_ptr()), C.c_void_p(ag.s_max.data_ptr()), self._stream()))
        return self

    def act_step(self, env, train=True, tick=None, a_out=None, returns_acc=None, window=None, noise_acc=None, envs_per_learner=None):
        """One fused vector step for all learners: env i acts with learner i // E's actor; with `window` = (pos, count, offset)
        each learner stores `count` transitions of its own env block into its own ring.  noise_acc: float32 [n] device tensor, env i's
        act() noise mean is added to noise_acc[i] (DDPG.jl:224).  envs_per_learner: the env block of this step when it is not the
        group's training block (the evaluation sweep's E_eval; no window then)."""
        epl = self.envs_per_learner if envs_per_learner is None else int(envs_per_learner)
        if env.n != self.count * epl:
            raise ValueError("the env batch must hold count * envs_per_learner envs")
        if noise_acc is not None and (noise_acc.dtype != self.torch.float32 or noise_acc.numel() != env.n or not noise_acc.is_contiguous()
                                      or noise_acc.device != self.device):
            raise ValueError("noise_acc must be a contiguous float32 tensor of one value per env on the group's device")
        env.use_torch_stream()
        v, g = env.view(), self.struct()
        g.envs_per_learner = epl
        a0 = self.learners[0]
        p = a0._act_params(train, self.tick if tick is None else tick, noise_acc=noise_acc)
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        r0 = self._ring0()
        w = RingWindow(*window) if window is not None else None
        if w is not None and self.n_step > 1:      # the stationary window into the staging rings; nstep_fold pushes and counts
            if w.offset != 0 or not 1 <= w.count <= min(epl, self.capacity):
                raise ValueError(f"act_step: an n_step = {self.n_step} group remembers the stationary window (count, 0) of ring_window, "
                                 f"count in 1 .. min(envs_per_learner, capacity); got count {w.count}, offset {w.offset}")
            r0, w = self.stage_of(0).struct(), RingWindow(0, w.count, 0)
            self._ns_window = int(w.count)
        ring_w = (C.byref(r0), C.byref(w)) if w is not None else (None, None)
        if self._x:
            if w is not None and w.count > min(self.mem_sizes):
                raise ValueError(f"a window of {w.count} transitions per step exceeds the smallest ring of the group ({min(self.mem_sizes)})")
            if self.ou_state is not None:          # the group's OU state, one [2] per env of the TRAINING batch; evaluation never reads it
                if train and env.n != self.n_envs:
                    raise ValueError("a training step with Ornstein-Uhlenbeck noise runs the group's own env batch (ou_state is keyed by its envs)")
                p.ou_state = self.ou_state.data_ptr()
            xptrs = self._x_ptrs()
        if self.form == "wide":                    # four launches for the whole group (noise mu / sigma from the records, if any)
            need = C.c_int64(0)
            _capi.check(self.L.shems_wide_act_workspace_floats(*self.hidden, env.n, C.byref(need)))
            if self._act_ws is None or self._act_ws.numel() < need.value:      # (an eval batch may be wider than the training batch)
                self._act_ws = self.torch.empty(need.value, dtype=self.torch.float32, device=self.device)
            if self._x:
                _capi.check(self.L.shems_wide_act_step_group_x_dev(C.byref(v), C.byref(p), C.byref(g), *self.hidden, self._hp_ptr(), *xptrs,
                                                                   C.c_void_p(self._act_ws.data_ptr()), ptr(a_out), ptr(returns_acc), *ring_w,
                                                                   self._stream()))
            else:
                _capi.check(self.L.shems_wide_act_step_group_dev(C.byref(v), C.byref(p), C.byref(g), *self.hidden, self._hp_ptr(),
                                                                 C.c_void_p(self._act_ws.data_ptr()), ptr(a_out), ptr(returns_acc), *ring_w, self._stream()))
        else:                                      # one launch; W2 from the tiles where they are current, noise mu / sigma from the records, if any
            t = C.byref(self.w2t_struct()) if self._use_tiled() else None
            if self._x:
                _capi.check(self.L.shems_act_step_group_x_dev(C.byref(v), C.byref(p), C.byref(g), t, self._hp_ptr(), *xptrs, ptr(a_out),
                                                              ptr(returns_acc), *ring_w, self._stream()))
            else:
                _capi.check(self.L.shems_act_step_group_dev(C.byref(v), C.byref(p), C.byref(g), t, self._hp_ptr(), ptr(a_out), ptr(returns_acc), *ring_w,
                                                            self._stream()))
        if w is not None and self.n_step == 1:
            for ring in self.rings:
                ring.pushed += int(window[1])
            if self._x and int(window[1]) > 0:     # the device counters follow on the stream, after the launch that read them
                self._pushed_dev.add_(int(window[1]))
                self._pushed_host = [ring.pushed for ring in self.rings]

    def replay(self, tick=None):
        """replay() (DDPG.jl:121-145) for every learner.  form "throughput": eight launches of csrc/shems_gupd.hip; "latency": 5 launches
        in total, grid z = learner (fused = False: the split calls, 7 launches -- the same bits)."""
        if self._x:                                # the *_x entry points' precondition (their lengths are device memory): no empty ring
            xptrs = self._x_ptrs()                 # (brings the host mirror of `pushed` up to date: one pass over the rings)
            if min(self._pushed_host) < 1:
                raise _capi.ShemsError(_capi.ERR_ARG, f"replay(): the ring of learner {self._pushed_host.index(min(self._pushed_host))} is empty")
        a0, g, r0 = self.learners[0], self.struct(), self._ring0()
        d = a0._ddpg_args()
        st = self._stream()
        sample = (len(self.rings[0]), self.rng_seed, tick32(tick, self.updates))
        adam_c, adam_a = a0._adam_c, a0._adam_a
        tl = self.form != "wide" and self._use_tiled()      # (a tiled group switched to the latency form: its Flux blocks are brought up to date)
        if self.form == "wide":                    # 24 launches for the whole group (csrc/shems_wide.hip)
            if self._x:
                _capi.check(self.L.shems_wide_group_update_x(C.byref(d), C.byref(r0), C.byref(g), *self.hidden, self._hp_ptr(), *xptrs,
                                                             self.max_batch, *sample[1:], *adam_c, *adam_a, st))
            else:
                _capi.check(self.L.shems_wide_group_update(C.byref(d), C.byref(r0), C.byref(g), *self.hidden, self._hp_ptr(), self.max_batch,
                                                           *sample, *adam_c, *adam_a, st))
        elif self.form == "throughput" or self._hp_dev is not None:      # records: batch / gamma / tau / eta per learner, this form only
            t = C.byref(self.w2t_struct()) if tl else None
            if self._x:
                _capi.check(self.L.shems_ddpg_group_update_tp_x(C.byref(d), C.byref(r0), C.byref(g), t, self._hp_ptr(), *xptrs, *sample[1:],
                                                                *adam_c, *adam_a, 1 if self.store_grad else 0, st))
            else:
                _capi.check(self.L.shems_ddpg_group_update_tp(C.byref(d), C.byref(r0), C.byref(g), t, self._hp_ptr(), *sample, *adam_c, *adam_a,
                                                              1 if self.store_grad else 0, st))
            if tl:
                self._flux_valid = False
        elif self.fused:
            _capi.check(self.L.shems_ddpg_group_update(C.byref(d), C.byref(r0), C.byref(g), *sample, *adam_c, *adam_a, st))
        else:
            _capi.check(self.L.shems_ddpg_group_critic_grad(C.byref(d), C.byref(r0), C.byref(g), *sample, st))
            _capi.check(self.L.shems_ddpg_group_critic_apply(C.byref(d), C.byref(g), *adam_c, st))
            _capi.check(self.L.shems_ddpg_group_actor_grad(C.byref(d), C.byref(g), st))
            _capi.check(self.L.shems_ddpg_group_actor_apply(C.byref(d), C.byref(g), *adam_a, st))
        self._advance_learners(critic=True, actor=True, counter="updates")
        self.updates += 1

    def _advance_learners(self, critic, actor, counter):
        """The learners advance in lockstep after a grouped update: the beta powers of the networks it stepped (shared by the group's
        launches) and every learner's `counter` ("updates", "clones" or "evaluations")."""
        for ag in self.learners:
            Agent._advance(ag, critic, actor, counter)

    # ---- grouped imitation: the supervised and the critic-only update for every learner ------------------------------------------------
    def _hp_variant(self, tau, check=True):
        """The group's records with the call's tau in place of the learners' (clone, evaluate(tau=...)): a second device record array,
        built and checked once per tau.  The kernels read the learner's batch and eta (and gamma) from it as from the group's own.
        check=False: the copy is not shown to shems_group_hparams_check (tau = 0, which it refuses, holds the targets of a TD3 group
        off a policy step; every other field comes from the checked records)."""
        tau = float(np.float32(tau))
        if tau not in self._hp_variants:
            arr = (HParams * self.count)(*[HParams(r["eta_act"], r["eta_crit"], nstep_gamma(r["gamma"], self.n_step), tau, r["mu"], r["sigma"],
                                                   r["batch"], 0) for r in self.hparams])
            if check and self.L.shems_group_hparams_check(arr, self.count) != _capi.OK:
                raise ValueError(self.L.shems_last_error().decode("utf-8", "replace"))
            self._hp_variants[tau] = self.torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(self.device)
        return C.c_void_p(self._hp_variants[tau].data_ptr())

    def _group_rings(self, rings, what):
        """(ring objects, learner 0's shems_replay, ring stride in bytes, the shared length) of a clone / evaluate call: `rings` is an
        imitation.GroupDemos / GroupRings (rings[l], struct0(), stride_bytes) or None, the group's own rings inside the slabs."""
        if self.form == "wide":
            raise NotImplementedError(f"{what}: the wide group form runs layer by layer (shems_wide_*), which has no {what} update")
        if rings is None:
            objs, r0, stride = self.rings, self._ring0(), self.slab_floats * 4
        else:
            if len(rings.rings) != self.count:
                raise ValueError(f"{what}: {len(rings.rings)} rings for a group of {self.count} learners")
            if rings.rings[0].s.device != self.device:
                raise ValueError(f"{what}: the rings live on {rings.rings[0].s.device}, the group on {self.device}")
            objs, r0, stride = rings.rings, rings.struct0(), int(rings.stride_bytes)
        lens = sorted({len(r) for r in objs})
        if len(lens) != 1:
            raise ValueError(f"{what}: the rings hold unequal lengths ({lens[0]} .. {lens[-1]}): a grouped update samples every learner's "
                             "ring with one shared length")
        return objs, r0, stride, lens[0]

    def _half_update(self, what, rings, tick, tau, critic):
        objs, r0, stride, n = self._group_rings(rings, what)
        if tau is not None and not 0.0 < float(tau) <= 1.0:
            raise ValueError(f"{what}: tau {tau} outside (0, 1]")
        a0 = self.learners[0]
        tick = tick32(tick, self.evaluations if critic else self.clones)
        if self.form == "throughput" or self._hp_dev is not None:
            tl = self._use_tiled()
            d, g = a0._ddpg_args(), self.struct()
            if tau is not None:
                d.tau = float(tau)
            hp = None if self._hp_dev is None else (self._hp_ptr() if tau is None else self._hp_variant(tau))
            t = C.byref(self.w2t_struct()) if tl else None
            fn = self.L.shems_ddpg_group_critic_update_tp if critic else self.L.shems_ddpg_group_clone_update_tp
            adam = a0._adam_c if critic else a0._adam_a
            _capi.check(fn(C.byref(d), C.byref(r0), stride, C.byref(g), t, hp, n, self.rng_seed, tick, *adam,
                           1 if self.store_grad else 0, self._stream()))
            if tl:
                self._flux_valid = False
            self._advance_learners(critic=critic, actor=not critic, counter="evaluations" if critic else "clones")
        else:                                      # latency form: the single-learner call on every learner's views, the same bits
            self._use_tiled()
            for ag, ring in zip(self.learners, objs):
                ag.evaluate(ring, tick=tick, tau=tau) if critic else ag.clone(ring, tick=tick, tau=tau)
        if critic:
            self.evaluations += 1
        else:
            self.clones += 1

    def clone(self, demos, tick=None, tau=1.0):
        """One SUPERVISED update of every learner's actor on its own demonstration ring (imitation.GroupDemos): Agent.clone's definition,
        loss_l = Flux.mse(actor_l(normalize(s)), a_demo) on the first batch_l draws of the stream (rng_seed + l, tick).  Throughput form:
        four launches for the whole group (shems_ddpg_group_clone_update_tp), with per-learner records the learner's eta_act and batch
        and the call's tau; latency form: learners[l].clone(demos.rings[l]) learner by learner; wide form: NotImplementedError.
        Nothing of the critics is touched.  tau = 1.0 keeps every actor_t equal to its actor bit for bit.  bp_actor advances in lockstep
        as in replay(); the step counts in `clones` (the default tick), `updates` does not move.  On a tiled group the Flux-order view
        goes stale, as after replay().  Demonstration rings of unequal length are refused."""
        self._half_update("clone", demos, tick, tau, critic=False)

    def evaluate(self, rings=None, tick=None, tau=None):
        """One CRITIC-ONLY update of every learner (Agent.evaluate's definition) from `rings` -- an imitation.GroupRings, or None for the
        group's own rings.  Throughput form: five launches, the update's own kernels (shems_ddpg_group_critic_update_tp): from the same
        state, ring, seed and tick the critic side holds the bits replay() leaves there, and nothing of the actors is touched.  Latency
        form: learners[l].evaluate(rings.rings[l]); wide form: NotImplementedError.  tau: None = the learners' own.  bp_critic advances
        in lockstep; the step counts in `evaluations` (the default tick)."""
        self._half_update("evaluate", rings, tick, tau, critic=True)

    def ring_window(self, num_steps=72, window_count=None):
        """(count, offset) of the transitions each learner stores at the CURRENT tick.
        window_count None: the vectorised default (SURVEY 8(d) replay-capacity note): a rotating window of min(E, capacity / num_steps)
        of the learner's E households per step, so the ring spans about one episode of each (capacity: the smallest mem_size).
        window_count 1: the reference's ratio -- episode! remembers ONE transition per replay() (DDPG.jl:229-233, push order
        [s, a, r, s', done] MPS:46-47): always household 0 of the learner's block, so that consecutive ring entries are one household's
        trajectory (s' of entry t = s of entry t + 1 inside an episode), as the reference's single env fills its CircularBuffer.
        Any other count: a rotating window of that many households."""
        E = self.envs_per_learner
        smallest = min(getattr(self, "mem_sizes", None) or (self.capacity,))       # (a bare namespace, tests/test_host_logic.py, has only capacity)
        wc = min(E, max(1, smallest // int(num_steps))) if window_count is None else int(window_count)
        if not 1 <= wc <= E:
            raise ValueError("window_count must be in 1 .. envs_per_learner")
        if getattr(self, "n_step", 1) > 1:         # n-step: the same households every hour, so that the history follows them
            return wc, 0
        return wc, (0 if wc == 1 else (self.tick * wc) % E)

    def episode_(self, env, train=True, num_steps=None, rng_ep=0, episode=0, window_count=None, noise_acc=None):
        """episode! for all learners at once (cf. Agent.episode_).  Returns the per-env episode returns [count * E].
        window_count: see ring_window (1 = one remembered transition per update, the thesis protocol's update-to-data ratio).
        noise_acc: float32 [count * E] device tensor that accumulates every env's act() noise mean (Agent.last_noise)."""
        t = self.torch
        num_steps = env.maxsteps if num_steps is None else int(num_steps)
        if train and self.n_step > 1:
            if num_steps < self.n_step:
                raise ValueError(f"episode_: num_steps = {num_steps} < n_step = {self.n_step}: an episode must hold one full window")
            if len(self.rings[0]) == 0:
                raise ValueError(f"episode_: n_step = {self.n_step} on empty rings: the first {self.n_step - 1} hours of an episode push "
                                 "nothing, so the updates of those hours need filled rings (populate_memory)")
        env.reset_(rng_ep, episode=episode) if rng_ep != -1 else env.reset_(-1)
        returns = t.zeros(env.n, dtype=t.float64, device=self.device)
        for step in range(num_steps):
            tick = (int(episode) * 4096 + step) & 0xFFFFFFFF
            win = (self.rings[0].pos, *self.ring_window(num_steps, window_count)) if train else None
            self.act_step(env, train=train, tick=tick, returns_acc=returns, window=win, noise_acc=noise_acc)
            if train and self.n_step > 1:
                self.nstep_fold(step)
            if train:
                self.replay()
            self.tick += 1
        return returns

    # ---- run_episodes (DDPG.jl:244-298) for every learner ----------------------------------------------------------------------------
    def run_episodes(self, env_train, env_eval, num_ep, test_every=100, test_runs=100, seed=None, window_count=None, on_eval=None,
                     on_best=None, pbt=None):
        """Agent.run_episodes for every learner at once: `num_ep` training episodes (episode_ with rng_ep = seed, episode = i), and when
        i % test_every == 1 an evaluation sweep on env_eval (eval_batch: count blocks of E_eval envs, learner l's block on its charger):
        every block reset with the Agent's fixed key (SEED_INI, episode 0, env indices from 0 inside the block), 72 fused group steps
        without noise, then ONE launch (shems_group_eval_best_dev) scores every learner on its first test_runs envs and snapshots the
        actors that beat their best score.  A sweep leaves the training state alone (networks, moments, tiles, rings, tick, updates).
        Per episode the learners' mean return and mean act() noise stay on the device (no host synchronisation); a sweep copies its
        scores to the host once, for on_eval(l, i, total_reward_l, score_l) (every learner) and on_best(l, i, best_actor_l,
        total_reward_l [i], score_mean_l [sweeps so far]) (the learners that improved; best_actor_l at the learner's own hidden size).
        On return flux_() has run, so learners[l].export_actor() is the last actor.  Returns a GroupRun.
        pbt: a PBT -- after the sweep of episode i with pbt.start <= i < num_ep (start defaults to test_every + 1, so neither the sweep
        of episode 1 nor a final sweep triggers one) pbt_round runs on that sweep's scores, round number = the sweep's index; the
        GroupRun's pbt_parent [count][rounds], pbt_episodes and pbt_hparams (the records after each round) log it.  The best-actor
        snapshot and best score stay the history of the SLOT: a child does not inherit its parent's."""
        E_eval = run_episodes_check(self.count, self.n_envs, getattr(env_train, "n", None), getattr(env_eval, "n", None), num_ep, test_every,
                                    test_runs)
        if pbt is not None:
            pbt_group_refusals(self.form, self.hparams, self.noise_type, self._x, pbt.populations, self.count)
            pbt_start = int(test_every) + 1 if pbt.start is None else pbt.start
            parents = []
        t = self.torch
        L, E, num_ep, test_every, test_runs = self.count, self.envs_per_learner, int(num_ep), int(test_every), int(test_runs)
        seed = self.seed if seed is None else int(seed)
        dev = self.device
        res = GroupRun(self, num_ep, test_every)
        noise_acc = t.zeros(self.n_envs, dtype=t.float32, device=dev)
        ev = t.cuda.Event
        t_start, t_end, sweeps = ev(enable_timing=True), ev(enable_timing=True), []
        t_start.record()
        for i in range(1, num_ep + 1):
            noise_acc.zero_()
            ret = self.episode_(env_train, train=True, rng_ep=seed, episode=i, window_count=window_count, noise_acc=noise_acc)
            res._total[:, i - 1] = ret.view(L, E).mean(1).to(t.float32)
            res._noise[:, i - 1] = noise_acc.view(L, E).mean(1)
            if i % test_every != 1:
                continue
            k = -(-i // test_every) - 1
            e0, e1 = ev(enable_timing=True), ev(enable_timing=True)
            e0.record()
            returns = self._eval_returns(env_eval, E_eval)
            d, g = self.learners[0]._ddpg_args(), self.struct()
            g.envs_per_learner = E_eval
            tl = self.tiled and not self._flux_valid           # the current W2 lives in the tiles only
            w2t = self.w2t_struct() if tl else None
            l1, l2 = self.hidden if self.form == "wide" else (0, 0)
            ptr = lambda x: C.c_void_p(x.data_ptr())
            _capi.check(self.L.shems_group_eval_best_dev(C.byref(d), C.byref(g), C.byref(w2t) if tl else None, l1, l2, ptr(returns), test_runs, i,
                                                         ptr(res._score), ptr(res._best_score), ptr(res._best_run), ptr(res._improved),
                                                         ptr(res.best), res.best_stride, self._stream()))
            res._score_mean[:, k] = res._score
            e1.record()
            sweeps.append((e0, e1))
            if pbt is not None and pbt_start <= i < num_ep:
                parents.append(self.pbt_round(res._score, pbt, k))
                res.pbt_episodes.append(i)
                res.pbt_hparams.append([dict(h) for h in self.hparams])
            if on_eval is None and on_best is None:
                continue
            host = t.stack([res._score, res._improved.to(t.float64), res._total[:, i - 1].to(t.float64)]).cpu().numpy()    # the sweep's one copy
            score, imp, tot = host[0], host[1] > 0, host[2].astype(np.float32)
            if on_best is not None and imp.any():
                won = np.flatnonzero(imp)
                rows = res.best[t.as_tensor(won, device=dev), :res.n_actor].cpu().numpy()
                tr, sm = res._total[:, :i].cpu().numpy(), res._score_mean[:, :k + 1].cpu().numpy()
                for r, l in enumerate(won):
                    on_best(int(l), i, res._unpad(int(l), rows[r]), tr[l], sm[l])
            if on_eval is not None:
                for l in range(L):
                    on_eval(l, i, float(tot[l]), float(score[l]))
        t_end.record()
        t_end.synchronize()
        res.wall_ms = t_start.elapsed_time(t_end)
        res.sweep_ms = sum(a.elapsed_time(b) for a, b in sweeps)
        res.sweeps = len(sweeps)
        if pbt is not None and parents:
            res.pbt_parent = np.stack(parents, axis=1)
        self.flux_()
        return res


    def _eval_returns(self, env_eval, E_eval):
        """The 72 hours of one evaluation sweep: every learner's block reset with Agent.run_episodes' fixed key (SEED_INI, episode 0, env
        indices from 0 inside the block: the same starts every sweep, DDPG.jl:273-277), then the fused group steps without noise.
        Returns the per-env float64 returns [count * E_eval]."""
        from .env import EnvSlice
        t = self.torch
        for l in range(self.count):
            EnvSlice(env_eval, l * E_eval, E_eval).reset_(SEED_INI, episode=0)
        returns = t.zeros(env_eval.n, dtype=t.float64, device=self.device)
        for step in range(EP_LENGTH_TRAIN):
            self.act_step(env_eval, train=False, tick=step, returns_acc=returns, envs_per_learner=E_eval)
        return returns

    def eval_scores(self, env_eval, test_runs=100):
        """One evaluation sweep of the CURRENT actors (no snapshot, no best tracking): every learner's score, the mean of its first
        test_runs eval returns summed in ascending order (float64 [count]), as run_episodes scores them."""
        E_eval = run_episodes_check(self.count, self.n_envs, self.n_envs, getattr(env_eval, "n", None), 1, 1, test_runs)
        r = self._eval_returns(env_eval, E_eval).view(self.count, E_eval)[:, :int(test_runs)].cpu().numpy()
        return np.cumsum(r, axis=1)[:, -1] / int(test_runs)


def per_extra_blocks(capacity):
    """The (name, floats) blocks a prioritized group keeps in every learner's slab behind ring_done: the priorities, pmax (padded to 16
    bytes) and the sampler workspace.  Host only."""
    return (("per_prio", int(capacity)), ("per_pmax", 4), ("per_ws", per_workspace_floats(int(capacity))))


def variant_group_refusals(w, form, noise_type, hparams, hidden):
    """The walk the variants of the throughput group share (per_group_refusals, td3.group_refusals): form, then "ou", then hidden=, then
    the records' mem_size / batch / hidden, in the variant's words `w`.  Host only."""
    no = lambda words: NotImplementedError(f"{w['name']}: {words}")
    if form in ("latency", "wide"):
        raise no(f"form={form!r} has no {w['head']}; the group runs the throughput form ({w['entry']}) whatever its count")
    if form not in (None, "throughput"):
        raise ValueError("form must be 'throughput'")
    if noise_type == "ou":
        raise no(f"Ornstein-Uhlenbeck noise runs on the *_x entry points, which have no {w['update']}")
    if hidden is not None:
        raise no(f"hidden= belongs to form='wide', which has no {w['update']}")
    for l, h in enumerate(hparams or ()):
        if hasattr(h, "keys") and "mem_size" in h:
            raise no(f"hparams[{l}]: per-learner mem_size runs on the *_x entry points, which have no {w['update']}{w['mem_size']}")
        if hasattr(h, "keys") and int(h.get("batch", 0)) > MAX_GROUP_BATCH:
            raise no(f"hparams[{l}]: batch {h['batch']} > {MAX_GROUP_BATCH}: {w['batch']}")
        if hasattr(h, "keys") and "hidden" in h and is_wide(h["hidden"]):
            raise no(f"hparams[{l}]: hidden {tuple(h['hidden'])} is wider than ({L1}, {L2}): the wide form has no {w['update']}")


_PER_WORDS = dict(name="prioritized learner group", head="weighted head", update="prioritized update", entry="shems_ddpg_group_update_per_tp",
                  mem_size=" (the rings advance in lockstep)", batch=f"the sampler draws at most {MAX_GROUP_BATCH} columns")


def per_group_refusals(form=None, noise_type="gn", hparams=None, hidden=None, capacity=MEM_SIZE, alpha=0.6, beta=0.4, eps=1e-6):
    """What PrioritizedLearnerGroup refuses before any device work, each by name."""
    import math
    variant_group_refusals(_PER_WORDS, form, noise_type, hparams, hidden)
    if int(capacity) > PER_MAX_SLOTS:
        raise NotImplementedError(f"prioritized learner group: capacity {int(capacity)} > {PER_MAX_SLOTS}: a learner's sampler workgroup keeps "
                                  "every block sum in LDS")
    for name, v in (("alpha", alpha), ("beta", beta), ("eps", eps)):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"prioritized learner group: {name} = {v!r} must be finite and >= 0")
    if beta > 1.0:
        raise ValueError(f"prioritized learner group: beta = {beta!r} must be in [0, 1]")


class PrioritizedLearnerGroup(LearnerGroup):
    """`count` independent DDPG learners that each draw their minibatch by priority (proportional prioritized replay, Schaul et al. 2016;
    shems_ddpg_group_update_per_tp): a LearnerGroup whose slabs also hold prio [capacity], pmax and the sampler workspace
    per learner, carved behind the ring, so every offset of a DDPG group is unchanged.  alpha, beta and eps are the group's; beta is
    read at every update (run_episodes(anneal_beta_from=...) anneals it).  `covered` counts the pushes whose priorities are set, for
    the whole group: the rings advance in lockstep, and the pushes since the last update (populate_memory's, the fused step's window)
    receive each learner's pmax before its draw.  Throughput form only, whatever the count.  act_step, populate_memory, min_max_buffer,
    ring_window, eval_scores, clone (it reads the demonstration rings, not the priorities) and flux_() are the LearnerGroup's.  Refused by
    name (NotImplementedError): form 'latency' / 'wide', "ou" noise and per-learner mem_size (the *_x entry points), batch > 128, wide
    hidden sizes, capacity > 262144, evaluate() and with it imitation.warm_start_group, a class that is also a TD3LearnerGroup."""

    has_evaluate = False

    def __init__(self, count, envs_per_learner, alpha=0.6, beta=0.4, eps=1e-6, **kw):
        if any(c.__name__ == "TD3LearnerGroup" for c in type(self).__mro__):
            raise NotImplementedError("prioritized learner group: the twin-critic update (TD3LearnerGroup) has no weighted head")
        if kw.get("hparams") is not None:
            kw["hparams"] = list(kw["hparams"])              # (a generator is walked once, here)
        per_group_refusals(kw.get("form"), kw.get("noise_type", "gn"), kw.get("hparams"), kw.get("hidden"), kw.get("capacity", MEM_SIZE),
                           alpha, beta, eps)
        kw["form"] = "throughput"
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        self._anneal = None                                  # (beta0, num_ep) while run_episodes(anneal_beta_from=beta0) runs
        super().__init__(count, envs_per_learner, **kw)
        self.LP = _capi.declare_group_per()
        self.slab[:, self.layout["per_pmax"][0]] = 1.0       # pmax: 1.0 at the start
        self.covered = 0                                     # pushes whose priorities are set (host state, the whole group's)

    def _extra_blocks(self, n_critic):
        return per_extra_blocks(self.capacity)

    # ---- views ----
    def _view(self, l, name):
        o, n = self.layout[name]
        return self.slab[l, o:o + n]

    def prio_of(self, l):
        """Learner l's priorities pi = p^alpha, [capacity]."""
        return self._view(l, "per_prio")

    def pmax_of(self, l):
        """Learner l's running maximum of every pi ever written, [1]."""
        return self._view(l, "per_pmax")[:1]

    def sampled_of(self, l):
        """The slots of learner l's last draw, int32 [128] (-1 in the pad columns)."""
        return self._view(l, "per_ws")[PW_IDX:PW_IDX + PER_COLS].view(self.torch.int32)

    def weights_of(self, l):
        """The importance weights of learner l's last draw, [128] (0 in the pad columns)."""
        return self._view(l, "per_ws")[PW_W:PW_W + PER_COLS]

    def fresh_range(self):
        """(fresh_pos, fresh_count) of the next update: the pushes since `covered` (PrioritizedRing.fresh_range for the group)."""
        n = self.rings[0].pushed - self.covered
        if n < 0:
            raise ValueError("prioritized learner group: pushed went backwards")
        return self.covered % self.capacity, min(n, self.capacity)

    def per_struct(self):
        """Learner 0's shems_per (learner l's arrays lie at + l * the slab stride)."""
        p = lambda name: self.slab.data_ptr() + 4 * self.layout[name][0]
        return PerArgs(p("per_prio"), p("per_pmax"), p("per_ws"), self.alpha, self.beta, self.eps, 0)

    def per_sample(self, tick=None, fresh=None, batch=None):
        """The sampler launch alone (shems_per_group_sample_dev): fresh fill, sums, draw and weights of every learner, as the next
        replay() would draw them.  fresh: (pos, count) in place of fresh_range(); `covered` does not move."""
        a0, g, per = self.learners[0], self.struct(), self.per_struct()
        pos, cnt = self.fresh_range() if fresh is None else fresh
        _capi.check(self.LP.shems_per_group_sample_dev(C.byref(per), C.byref(g), self._hp_ptr(), self.capacity, len(self.rings[0]), int(pos),
                                                       int(cnt), self.rng_seed, tick32(tick, self.updates), a0.batch if batch is None else int(batch),
                                                       self._stream()))

    # ---- refused paths ----
    def evaluate(self, rings=None, tick=None, tau=None):
        raise NotImplementedError("prioritized learner group: evaluate() is the critic-only update on a uniform draw; the prioritized group "
                                  "has none (and so imitation.warm_start_group does not run on it)")

    def _update(self, tick, flags):
        if self.form != "throughput":
            raise NotImplementedError(f"prioritized learner group: form={self.form!r} has no weighted head")
        a0, g, r0 = self.learners[0], self.struct(), self._ring0()
        if self._hp_dev is None and a0.batch > MAX_GROUP_BATCH:
            raise NotImplementedError(f"prioritized learner group: batch {a0.batch} > {MAX_GROUP_BATCH}: the sampler draws at most "
                                      f"{MAX_GROUP_BATCH} columns")
        tl = self._use_tiled()
        d, per = a0._ddpg_args(), self.per_struct()
        t = C.byref(self.w2t_struct()) if tl else None
        _capi.check(self.LP.shems_ddpg_group_update_per_tp(C.byref(d), C.byref(r0), C.byref(g), t, self._hp_ptr(), C.byref(per), len(self.rings[0]),
                                                           *self.fresh_range(), self.rng_seed, tick32(tick, self.updates), *a0._adam_c, *a0._adam_a,
                                                           flags | (_capi.TP_STORE_GRAD if self.store_grad else 0), self._stream()))
        if tl:
            self._flux_valid = False
        self._advance_learners(critic=True, actor=True, counter="updates")
        self.updates += 1

    def replay(self, tick=None):
        """One prioritized update of every learner (shems_ddpg_group_update_per_tp: nine launches).  The pushes since `covered` are the
        fresh range; bp_critic, bp_actor and `updates` advance as in LearnerGroup.replay().  On a tiled group the Flux-order view goes
        stale, as after LearnerGroup.replay()."""
        self._update(tick, 0)
        self.covered = self.rings[0].pushed

    def replay_given(self, idx, weights):
        """replay() on slots and weights the caller supplies (SHEMS_TP_PER_GIVEN): idx int32 [count][128] (-1 in the pad columns) and
        weights float32 [count][128], device tensors, copied into the learners' sampler workspaces.  No sampler launch, no write-back,
        `covered` does not move; with learner l's idx = sample_indices(rng_seed + l, tick) and weights of 1.0 it leaves
        LearnerGroup.replay()'s bits.  State advances as in replay()."""
        t = self.torch
        shape = (self.count, PER_COLS)
        if idx.dtype != t.int32 or weights.dtype != t.float32 or tuple(idx.shape) != shape or tuple(weights.shape) != shape:
            raise ValueError(f"replay_given: idx int32 {list(shape)}, weights float32 {list(shape)}")
        if idx.device != self.device or weights.device != self.device:
            raise ValueError(f"replay_given: idx and weights must live on {self.device}")
        o = self.layout["per_ws"][0]
        self.slab[:, o + PW_IDX:o + PW_IDX + PER_COLS].view(t.int32).copy_(idx)
        self.slab[:, o + PW_W:o + PW_W + PER_COLS].copy_(weights)
        self._update(None, _capi.TP_PER_GIVEN)

    def episode_(self, env, train=True, num_steps=None, rng_ep=0, episode=0, window_count=None, noise_acc=None):
        if train and self._anneal is not None:     # Agent.run_episodes' rule: linear in the episode, exactly 1.0 in the last one
            beta0, num_ep = self._anneal
            self.beta = anneal_beta(beta0, int(episode) - 1, max(1, num_ep - 1))
        return super().episode_(env, train=train, num_steps=num_steps, rng_ep=rng_ep, episode=episode, window_count=window_count,
                                noise_acc=noise_acc)

    def run_episodes(self, env_train, env_eval, num_ep, test_every=100, test_runs=100, seed=None, window_count=None, on_eval=None,
                     on_best=None, anneal_beta_from=None, pbt=None):
        """LearnerGroup.run_episodes on prioritized updates.  anneal_beta_from: beta of episode i is anneal_beta(anneal_beta_from, i - 1,
        num_ep - 1): linear in the episode, exactly 1.0 in the last one (Agent.run_episodes' rule); None keeps `beta` as it stands.
        pbt: as LearnerGroup.run_episodes; a child keeps its own ring, priorities and pmax."""
        if anneal_beta_from is not None:
            anneal_beta(anneal_beta_from, 0, 1)              # (refuses a beta0 outside [0, 1] before anything runs)
            self._anneal = (float(anneal_beta_from), int(num_ep))
        try:
            return super().run_episodes(env_train, env_eval, num_ep, test_every=test_every, test_runs=test_runs, seed=seed,
                                        window_count=window_count, on_eval=on_eval, on_best=on_best, pbt=pbt)
        finally:
            self._anneal = None


def run_episodes_check(count, n_envs, n_train, n_eval, num_ep, test_every, test_runs):
    """LearnerGroup.run_episodes' argument checks (host only, before any device work).  Returns E_eval, the eval block of one learner."""
    if n_train != n_envs:
        raise ValueError(f"env_train holds {n_train} envs; the group trains count x envs_per_learner = {n_envs}")
    if int(num_ep) < 1 or int(test_every) < 1:
        raise ValueError(f"num_ep ({num_ep}) and test_every ({test_every}) must be >= 1")
    if n_eval is None or n_eval < count or n_eval % count:
        raise ValueError(f"env_eval holds {n_eval} envs: it must hold count = {count} equal blocks (eval_batch builds it)")
    E_eval = n_eval // count
    if E_eval % 32:
        raise ValueError(f"env_eval's block of {E_eval} envs per learner is not a multiple of 32 (eval_batch rounds test_runs up)")
    if not 1 <= int(test_runs) <= E_eval:
        raise ValueError(f"test_runs {test_runs} must be in 1 .. {E_eval}, env_eval's block per learner")
    return E_eval


class GroupRun:
    """What LearnerGroup.run_episodes returns: per learner the curves, the best run and the device snapshot slab `best`
    ([count][row] float32, row l = actor (the group's padded layout) | pad | s_min[9] | pad | s_max[9] | pad, harness.inference_many's row)."""

    def __init__(self, grp, num_ep, test_every):
        t = grp.torch
        L, dev = grp.count, grp.device
        self.count, self.hidden_of = L, [ag.hidden for ag in grp.learners]
        self.layout_hidden = grp.hidden if grp.form == "wide" else (L1, L2)
        self.n_actor = grp.layout["actor"][1]
        self.row = _pad4(self.n_actor) + 32
        self.best_stride = self.row * 4
        self.best = t.zeros((L, self.row), dtype=t.float32, device=dev)
        self._total = t.zeros((L, num_ep), dtype=t.float32, device=dev)
        self._noise = t.zeros((L, num_ep), dtype=t.float32, device=dev)
        self._score_mean = t.zeros((L, -(-num_ep // test_every)), dtype=t.float64, device=dev)
        self._score = t.zeros(L, dtype=t.float64, device=dev)
        self._best_score = t.full((L,), -100000.0, dtype=t.float64, device=dev)      # best_score = -100000 (DDPG.jl:246)
        self._best_run = t.zeros(L, dtype=t.int32, device=dev)
        self._improved = t.zeros(L, dtype=t.uint8, device=dev)
        self.wall_ms = self.sweep_ms = 0.0
        self.sweeps = 0
        self.pbt_parent = np.zeros((L, 0), dtype=np.int32)         # run_episodes(pbt=...): parent[l] of every round (l itself: kept)
        self.pbt_episodes, self.pbt_hparams = [], []               # the episodes whose sweeps ran a round; the records after each round

    total_reward = property(lambda self: self._total.cpu().numpy())          # [L][num_ep] float32
    noise_mean = property(lambda self: self._noise.cpu().numpy())            # [L][num_ep] float32
    score_mean = property(lambda self: self._score_mean.cpu().numpy())       # [L][ceil(num_ep / test_every)] float64
    best_run = property(lambda self: self._best_run.cpu().numpy())           # [L] int32, 0: no sweep beat -100000
    best_score = property(lambda self: self._best_score.cpu().numpy())

    def _unpad(self, l, flat):
        h = self.hidden_of[l]
        return unpad_net_from(flat, STATE, ACTION, h, self.layout_hidden) if self.layout_hidden != (L1, L2) else unpad_net(flat, STATE, ACTION, h)

    def best_actor(self, l):
        """Learner l's best actor at its own hidden size (what the reference's saveBSON(...; path="temp") holds)."""
        return self._unpad(l, self.best[l, :self.n_actor].cpu().numpy())

    def best_norm(self, l):
        """(s_min, s_max) stored with learner l's best actor."""
        o = _pad4(self.n_actor)
        r = self.best[l].cpu().numpy()
        return r[o:o + STATE].copy(), r[o + 16:o + 16 + STATE].copy()


def eval_batch(tables, table_of_learner, count, test_runs=100, maxsteps=1439, charger_ids=None, device=None):
    """The grouped eval ShemsBatch of LearnerGroup.run_episodes: count x E_eval envs, E_eval = test_runs rounded up to 32; learner l's
    block runs on tables[table_of_learner[l]] with its config (make_config(charger_ids[k], ...); default charger 98) through cfg_of_env.
    maxsteps: the eval data set's episode length (main.EP_LENGTH; 1439 = ("all", "eval"))."""
    from .env import ShemsBatch, make_config
    tabs = list(tables)
    count, test_runs = int(count), int(test_runs)
    if count < 1 or test_runs < 1:
        raise ValueError(f"count ({count}) and test_runs ({test_runs}) must be >= 1")
    if not tabs:
        raise ValueError("eval_batch needs at least one table")
    tol = np.asarray(table_of_learner, dtype=np.int64).reshape(-1)
    if tol.size != count:
        raise ValueError(f"table_of_learner holds {tol.size} entries for {count} learners")
    if tol.size and (tol.min() < 0 or tol.max() >= len(tabs)):
        raise ValueError(f"table_of_learner names table {int(tol.max() if tol.max() >= len(tabs) else tol.min())}; there are {len(tabs)}")
    ids = [98] * len(tabs) if charger_ids is None else [int(c) for c in charger_ids]
    if len(ids) != len(tabs):
        raise ValueError(f"charger_ids holds {len(ids)} entries for {len(tabs)} tables")
    if int(maxsteps) < EP_LENGTH_TRAIN:
        raise ValueError(f"maxsteps {maxsteps} < {EP_LENGTH_TRAIN}: a sweep runs {EP_LENGTH_TRAIN} steps")
    E_eval = -(-test_runs // 32) * 32
    row0 = np.cumsum([0] + [np.asarray(t).shape[0] for t in tabs])
    cfgs = [make_config(c, row0[k], np.asarray(tabs[k]).shape[0]) for k, c in enumerate(ids)]
    co = np.repeat(tol, E_eval).astype(np.uint16)
    import torch
    dev = torch.cuda.current_device() if device is None else int(device)
    return ShemsBatch(count * E_eval, int(maxsteps), tabs, cfgs, co, device=dev).use_torch_stream()


def foresight_scores(env_eval, test_runs=100, grid=None, count=None, horizon=None, control=1):
    """The perfect-foresight return next to score_mean: for an eval_batch, every learner's block is reset with Agent.run_episodes'
    fixed key exactly as a sweep does (LearnerGroup._eval_returns), the backward sweep runs once per distinct (table, config, start
    row) over the sweep's 72 hours, the greedy forward pass steps every env, and learner l's number is the mean of its first
    test_runs returns summed in ascending order (float64 [count]).  count: learners of the batch (default: one block of E_eval =
    test_runs rounded up to 32 per learner).  horizon: the receding-horizon controller's return instead (foresight.solve_horizon with
    `horizon` hours of forecast and a fresh plan every `control` hours)."""
    from . import foresight
    from .env import EnvSlice
    test_runs = int(test_runs)
    E_eval = -(-test_runs // 32) * 32 if count is None else env_eval.n // int(count)
    if test_runs < 1 or E_eval < test_runs or env_eval.n % E_eval:
        raise ValueError(f"env_eval holds {env_eval.n} envs: not whole blocks of {E_eval} for test_runs = {test_runs} (eval_batch builds it)")
    L = env_eval.n // E_eval
    env_eval.use_torch_stream()
    for l in range(L):
        EnvSlice(env_eval, l * E_eval, E_eval).reset_(SEED_INI, episode=0)
    cfgs, idx0, poe = foresight.problems_of_env(env_eval)
    if horizon is None:
        values = foresight.solve(env_eval, cfgs, idx0, EP_LENGTH_TRAIN, grid, want_argmax=False)
    else:
        values = foresight.solve_horizon(env_eval, cfgs, idx0, EP_LENGTH_TRAIN, horizon, control, grid, want_argmax=False)
    totals, _, _ = foresight.track(env_eval, values, poe, which=0)
    r = totals.reshape(L, E_eval)[:, :test_runs]
    return np.cumsum(r, axis=1)[:, -1] / test_runs


class GroupWorkload:
    """bench.py's "group" step: one fused vector step of all learners' envs + one replay() of every learner."""

    name = "group"
    dtype = "f32"
    EP_LEN = 72

    def __init__(self, S, torch, n, learners, seed, mixed=False, form=None, window=None):
        """window: transitions each learner remembers per vector step (None: min(E, MEM_SIZE / 72), the rotating window; 1: the reference's
        one transition per replay(), LearnerGroup.ring_window)."""
        self.S, self.torch, self.n, self.count = S, torch, int(n), int(learners)
        if self.n % self.count or (self.n // self.count) % 32:
            raise ValueError("--envs must be learners x a multiple of 32")
        E = self.n // self.count
        if mixed:                       # the thesis grid: learner l trains on charger profile l mod 10 (ids 1-9, 98; LU1:47-58)
            ids = (1, 2, 3, 4, 5, 6, 7, 8, 9, 98)
            tabs = [S.tables.synthetic_table("train", c) for c in ids]
            row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
            cfgs = [S.make_config(c, row0[k], tabs[k].shape[0]) for k, c in enumerate(ids)]
            co = ((np.arange(self.n) // E) % len(ids)).astype(np.uint16)
            self.env = S.ShemsBatch(self.n, self.EP_LEN, tabs, cfgs, co, device=torch.cuda.current_device()).use_torch_stream()
        else:
            self.tab = S.tables.synthetic_table("train", 98)
            self.env = S.ShemsBatch(self.n, self.EP_LEN, [self.tab], [S.make_config(98, 0, self.tab.shape[0])],
                                    device=torch.cuda.current_device()).use_torch_stream()
        self.env_seed = int(seed)
        self.group = LearnerGroup(self.count, E, seed=1231, rng_seed=self.env_seed, form=form)
        self.group.populate_memory(self.env, seed=self.env_seed)
        self.group.min_max_buffer()
        self.window = None if window is None else int(window)
        self.win = self.group.ring_window(self.EP_LEN, self.window)[0]
        self.t, self.episode = 0, 1
        self.env.reset_(self.env_seed, episode=self.episode)

    def step(self):
        if self.t and self.t % self.EP_LEN == 0:
            self.episode += 1
            v = self.env.view()
            _capi.check(_capi.lib().shems_reset_seeded_dev(C.byref(v), self.env_seed, self.episode, self.env._stream()))
        g = self.group
        g.tick = self.t
        g.act_step(self.env, train=True, tick=self.t, window=(g.rings[0].pos, *g.ring_window(self.EP_LEN, self.window)))
        g.replay()
        self.t += 1

    def finish(self):
        self.torch.cuda.synchronize()
        self.env.check_error()
        end = self.group.layout["ws"][0]               # networks, targets, moments, gradients, normalisation, losses (the workspace
        if not bool(self.torch.isfinite(self.group.slab[:, :end]).all()):      # keeps int32 slots whose -1 pad reads as NaN)
            raise RuntimeError("non-finite learner state after the timed steps")

    def kernel_pass(self, reps):
        """HIP-event timing of the fused act/step launch (all learners' envs) and of one grouped replay()."""
        torch = self.torch
        from .timing import time_launches
        g = self.group
        reset = lambda k, i: self.env.reset_(self.env_seed, episode=100000 + i) if k % 8 == 0 else None
        def act(i):
            g.tick = i
            g.act_step(self.env, train=True, tick=i, window=(g.rings[0].pos, *g.ring_window(self.EP_LEN, self.window)))
        avg_us, med_us, reps = time_launches(torch, act, min(reps, 96), before_group=reset)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        nup = 20
        e0.record()
        for _ in range(nup):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        self.update_us = e0.elapsed_time(e1) * 1e3 / nup
        flops = 2 * (9 * 250 + 250 * 500 + 500 * 2) * self.n
        act = dict(kernel=group_act_kernel_name(self.n, g.envs_per_learner, g.tiled), avg_us=avg_us, median_us=med_us, launches=reps,
                   bound="mfma", algorithmic=flops, unit="TFLOP/s", peak=157.3)
        if self.update_us <= avg_us:
            return act
        # the grouped replay() is the larger share of the step: it is the kernel the roofline object describes.
        # Work per learner-update: 2.565 MFLOP x B = 307.8 MFLOP, and 12.4 MB that have to move (258 003 parameters x
        # (28 B ADAM + 12 B soft update) + one pass over the four networks' weights) -- at 400 learners 0.78 ms at the fp32-MFMA peak and
        # 0.62 ms at 8 TB/s: the matrix pipe is the binding roof, HBM within 25 % of it.
        upd_bytes = 258003 * 40 + 2 * 4 * (129002 + 129001)
        tp = g.form == "throughput"
        name = ("grouped replay(), throughput form: k_tp_prep + k_tp_fwd x3 + k_tp_d1 x2 + k_tp_gw2 x2 (csrc/shems_gupd.hip)" if tp else
                "grouped replay(), latency form: k_fwd x2 + k_mid + k_grad x2 with grid z = learner (csrc/shems_ddpg.hip)")
        t_s = self.update_us * 1e-6
        return dict(kernel=name, avg_us=self.update_us, median_us=self.update_us, launches=nup, bound="mfma",
                    algorithmic=2.565e6 * BATCH_SIZE * self.count, unit="TFLOP/s", peak=157.3,
                    algorithmic_bytes=upd_bytes * self.count, algorithmic_gbs=upd_bytes * self.count / t_s / 1e9,
                    hbm_frac_of_8tbs=upd_bytes * self.count / t_s / 8e12, per_learner_update_us=self.update_us / self.count,
                    launches_per_update=8 if tp else 5,
                    other_kernel={"kernel": act["kernel"], "avg_us": avg_us, "frac": flops / (avg_us * 1e-6) / 1e12 / 157.3},
                    method=f"HIP events around {nup} grouped replay() calls back to back ({8 if tp else 5} launches each, all learners per launch)")

    def extra(self):
        return {"learners": self.count, "envs_per_learner": self.n // self.count, "updates_per_step": self.count,
                "batch_size": BATCH_SIZE, "mem_size": MEM_SIZE, "replay_window_envs_per_step": self.win,
                "group_update_us": getattr(self, "update_us", None), "update_mflop": 307.8, "update_form": self.group.form,
                "w2_layout": "tiled (shems_group_w2t: one 64 KB piece per 64 x 64 tile of W2 | m | v | target)" if self.group.tiled else "Flux order"}

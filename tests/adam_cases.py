"""The cases of tests/test_adam_edges_gpu.py (and of the CPU measurement in tests/test_adam_horizon_host.py): beta powers by the host's
own repeated product, and full parameter vectors whose value classes are assigned by index modulo, so that every run of 64 consecutive
elements -- every Flux.params block but the one- or two-element b3, every 1024-element workgroup, every 64 x 64 tile -- holds every
gradient class in every moment state.

No NaN, no infinity, no |g| above 1e18: the reference defines no behaviour for them."""
from __future__ import annotations

import functools

import numpy as np

import adam_ref as AR

f32, f64 = np.float32, np.float64

HORIZON = 80_000                       # a thesis run (1001 episodes x 72 steps = 72 072 updates) plus margin
THESIS_UPDATES = 72_072
TAU = float(f32(1e-3))                 # the project's default (ddpg.TAU)
ETA_ACT, ETA_CRIT = float(f32(1e-4)), float(f32(1e-3))        # the thesis values
ETA_MIN, ETA_MAX = float(f32(1e-5)), float(f32(5e-3))         # the extremes of group.tuned_grid (asserted in the host test)
N_MAX = 11 * 300 + 300 + 300 * 600 + 600 + 600 + 1            # the largest network the cases are cut from: the (300, 600) critic


@functools.lru_cache(maxsize=None)
def _power_table():
    """bp[t - 1] = (bp1, bp2) as update t receives them: [0.9, 0.999] advanced t - 1 times by Python float multiplication, exactly as
    ddpg.Agent, td3.TD3Agent, LearnerGroup._advance_learners and the native loop's record advance them."""
    out, b1, b2 = [], 0.9, 0.999
    for _ in range(HORIZON):
        out.append((b1, b2))
        b1, b2 = b1 * 0.9, b2 * 0.999
    return out


def powers(step):
    return _power_table()[int(step) - 1]


SETTLED_BP1 = 5 * 2.0 ** -1074         # where 0.9^t sticks: 5 units of the smallest subnormal (asserted in the host test)
BP_STEPS = (1, 2, 100, 7000, THESIS_UPDATES)

# ---- value classes ---------------------------------------------------------------------------------------------------------------
G_CLASSES = ("zero", "+1e-23", "-1e-23", "+3e-20", "-3e-20", "+1e-10", "-1e-10", "+1e-3", "-1e-3", "+1", "-1", "+1e18", "-1e18",
             "cancel", "random", "cancel-near")
M_STATES = ("zero", "one-step", "late", "v-subnormal")
NG, NM, NP = len(G_CLASSES), len(M_STATES), 3
PERIOD = NG * NM                       # 64: one run of this length holds every (gradient class, moment state) pair


def g_class(i):
    return np.asarray(i) % NG


def m_state(i):
    return (np.asarray(i) // NG) % NM


def p_class(i):
    return np.asarray(i) % NP           # 3 is coprime to 64: over 192 elements every triple occurs


def state(seed, n=N_MAX):
    """(p, m, v, target, g) float32 [n]; element i's classes depend on i alone, its magnitudes on (seed, i)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    dec = lambda lo, hi: 10.0 ** (lo + (hi - lo) * rng.random(n))
    # moments
    g_prev = rng.normal(0, 1, n) * dec(-5, -1)
    m = np.zeros(n, f64)
    v = np.zeros(n, f64)
    ms = m_state(i)
    one = ms == 1
    m[one] = (0.1 * g_prev)[one]
    v[one] = (0.001 * g_prev * g_prev)[one]
    late = ms == 2
    m[late] = (sign * 1e-4 * dec(-2, 2))[late]
    v[late] = (1e-8 * dec(-2, 2))[late]
    sub = ms == 3
    m[sub] = (sign * 1e-20 * dec(-2, 2))[sub]
    v[sub] = (2.0 ** -149 * np.floor(1 + rng.random(n) * 2.0 ** 20))[sub]          # 1 .. 2^20 units of the smallest fp32 subnormal
    m, v = m.astype(f32), v.astype(f32)
    assert (v[sub] > 0).all() and (v[sub] < AR.F32_MIN_NORMAL).all()
    # gradients
    gc = g_class(i)
    g = np.zeros(n, f64)
    for k, name in enumerate(G_CLASSES):
        if name[0] in "+-":
            g[gc == k] = float(name)
    rnd = gc == G_CLASSES.index("random")
    g[rnd] = (rng.normal(0, 1, n) * 1e-3)[rnd]
    # m and g of opposite sign, |(1 - b1) g| ~ |b1 m|: g = -9 m, exactly as fp32 rounds it ("cancel") or a few fp32 ulp away
    # ("cancel-near"); a zero moment has nothing to cancel and takes -9e-4
    for name, wobble in (("cancel", 0.0), ("cancel-near", 2.0 ** -21)):
        c = gc == G_CLASSES.index(name)
        g[c] = np.where(m[c] != 0, -9.0 * m[c].astype(f64) * (1.0 + wobble * rng.integers(-3, 4, n)[c]), -9e-4)
    g = g.astype(f32)
    # parameters: glorot-sized, tiny (a step is resolved to the last bit), exactly zero / large
    pc = p_class(i)
    p = np.where(pc == 0, (rng.random(n) - 0.5) * 0.2, np.where(pc == 1, sign * 1e-12 * dec(-3, 3), np.where((i // NP) % 2 == 0, 0.0, sign * 2.5)))
    p = p.astype(f32)
    t = (p.astype(f64) + rng.normal(0, 1, n) * 1e-3 * np.abs(p)).astype(f32)
    t[(i // PERIOD) % 5 == 0] = (rng.normal(0, 0.05, n)[(i // PERIOD) % 5 == 0]).astype(f32)     # targets far from their parameters too
    return p, m, v, t, g


# ---- the apply entry points' cases -------------------------------------------------------------------------------------------------
def apply_cases(critic):
    """[(name, seed, step, eta, tau)]: every beta-power step at the default tau and the network's thesis eta; tau = 0 and 1, and the
    tuned grid's smallest and largest eta, at an early and at the settled step."""
    eta = ETA_CRIT if critic else ETA_ACT
    out = [(f"step{s}", 100 + k, s, eta, TAU) for k, s in enumerate(BP_STEPS)]
    for s in (1, THESIS_UPDATES):
        out += [(f"step{s}-tau0", 200 + s % 7, s, eta, 0.0), (f"step{s}-tau1", 300 + s % 7, s, eta, 1.0)]
    for s in (100, THESIS_UPDATES):
        out += [(f"step{s}-eta-min", 400 + s % 7, s, ETA_MIN, TAU), (f"step{s}-eta-max", 500 + s % 7, s, ETA_MAX, TAU)]
    return out


@functools.lru_cache(maxsize=None)
def apply_case(critic, name):
    """-> dict(old = (p, m, v, target), g, ref = (p, m, v, target), delta, eta, tau, bp) at N_MAX elements; slices of it are the case of a
    smaller network (the arithmetic is elementwise).  Computed once, shared, read-only."""
    (_, seed, step, eta, tau), = [c for c in apply_cases(critic) if c[0] == name]
    p, m, v, t, g = state(seed)
    bp = powers(step)
    ref = AR.reference(p, m, v, t, g, eta, tau, *bp)
    delta = AR.reference_delta(m, v, g, eta, *bp)
    for a in (p, m, v, t, g, delta) + tuple(ref):
        a.setflags(write=False)
    return dict(old=(p, m, v, t), g=g, ref=ref, delta=delta, eta=eta, tau=tau, bp=bp, step=step)


def assert_not_vacuous(case, blocks):
    """The reference's own step is non-zero for every gradient class except exact zero on a zero moment, and every class occurs in every
    Flux.params block (lo, hi) longer than the two elements of b3."""
    n = len(case["g"])
    i = np.arange(n)
    m = case["old"][1]
    must = ~((case["g"] == 0) & (m == 0))
    assert (case["delta"][must] != 0).all(), "a case whose reference step is zero checks nothing"
    assert (case["delta"][~must] == 0).all()
    for lo, hi in blocks:
        if hi - lo > 2:
            assert len(np.unique(g_class(i[lo:hi]))) == NG and len(np.unique(m_state(i[lo:hi]))) == NM, (lo, hi)
            if hi - lo >= PERIOD:
                assert len(np.unique(g_class(i[lo:hi]) * NM + m_state(i[lo:hi]))) == PERIOD, (lo, hi)


# ---- the grouped kernels' late regime ------------------------------------------------------------------------------------------------
def late_moments(seed, n):
    """(m, v) float32 [n] as thousands of updates leave them -- "late" (m ~ 1e-4, v ~ 1e-8, random signs, four decades) and
    "v-subnormal" -- alternating in runs of 16, so that every 64 x 64 tile and every block holds both."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    dec = lambda lo, hi: 10.0 ** (lo + (hi - lo) * rng.random(n))
    sub = (i // NG) % 2 == 1
    m = np.where(sub, sign * 1e-20 * dec(-2, 2), sign * 1e-4 * dec(-2, 2)).astype(f32)
    v = np.where(sub, 2.0 ** -149 * np.floor(1 + rng.random(n) * 2.0 ** 20), 1e-8 * dec(-2, 2)).astype(f32)
    assert (v > 0).all() and (v[sub] < AR.F32_MIN_NORMAL).all() and (m != 0).all()
    return m, v


GROUP_E, GROUP_CAP, GROUP_BATCH = 32, 128, 17          # the smallest group that reaches the grouped kernels (tests/group_td3_cases.py's shapes)
GROUP_TAUS = (TAU, float(f32(0.01)), 1.0, float(f32(0.005)))


def group_records(count, **other):
    """Per-learner records spanning the tuned grid's extremes: learner l's eta_act, eta_crit and tau differ from its neighbours'."""
    etas = (ETA_MIN, ETA_MAX, ETA_ACT, ETA_CRIT)
    return [dict(eta_act=etas[l % 4], eta_crit=etas[(l + 1 + l // 4) % 4], tau=GROUP_TAUS[(l + l // 4) % 4], batch=GROUP_BATCH, **other) for l in range(count)]

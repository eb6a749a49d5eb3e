"""The cases of prioritized replay for learner groups (group.PrioritizedLearnerGroup, shems_ddpg_group_update_per_tp), kept in ONE
place: tests/test_group_per_gpu.py runs them on the device, tests/test_group_per_host.py proves on the CPU -- on the NumPy twins alone --
that the rings, seeds and ticks chosen here hold what the GPU cases are there for.  TEST INFRASTRUCTURE ONLY.

Shapes of tests/test_group_td3_gpu.py: 32 envs per learner, L in {2, 48} (both launch shapes), a seed per learner.  Rings are synthetic
(tests/warmstart_ref.py: critic_data, seed 100 + l) of capacity 1 000: four blocks of the sum structure, the last one partial.  Learner
0's priorities are tests/per_cases.py's "heavy" ring (five slots that each cover several strata: some columns share a slot, others do
not), every other learner's span four decades.  Learner l samples with the Philox key RNG_SEED + l on the prioritized stream.

The twin of a prioritized group is tests/per_ref.py per learner -- key seed + l, the learner's own batch, the group's ring_len / fresh
range / alpha / beta / eps -- composed with the float64 evaluation every group test holds the throughput form to (oracle/ddpg_oracle.py)."""
import functools

import numpy as np

import ddpg_oracle as DO
import per_cases as PC
import per_ref as PR
import warmstart_ref as WR

f32 = np.float32
E, CAP = 32, 1000
SEED, RNG_SEED = 21, 77
ALPHA, BETA, EPS_P = PR.ALPHA, PR.BETA, PR.EPS_P
TICKS = (1, 2)                         # (chosen on the CPU: at ticks 0 and 3 the float64 evaluation of learner 0's actor pass has a tied relu)
TIE = 1e-7                             # a relu whose float64 pre-activation is this close to zero may be decided either way
DUP_LEARNER = 0                        # the learner whose ring has partial duplicates

# (learners, batch): 2 learners run the narrow launch shapes, 48 the wide ones
STAGE_CASES = [(2, 120), (48, 120), (2, 17)]
# the comparisons that needed a tied relu decided the other way: [(network, learner, tick)]
EXPECTED_TIES = {c: [] for c in STAGE_CASES}
CASE_TICKS = {}                        # a case whose tick ties takes another one here (none does)
# two learners with their own batch (and eta_crit, gamma): the sampler's batch_l and the head's divisor come from the record
RECORD_CASE = [dict(batch=17, eta_crit=2e-3, gamma=0.9), dict(batch=120, eta_crit=5e-4, gamma=0.99)]
# the sampler's ring and batch edges at the group's shapes: tests/per_cases.py's cases whose ring fits a slab of capacity <= 1 000
BIG = dict(capacity=24000, ring_len=24000, batch=120, kind="decades", fresh=(0, 0), pmax=1.0, beta=0.4, seed=RNG_SEED, tick=5)


def checked(L):
    return (0, L - 1)


def ticks_of(case):
    return CASE_TICKS.get(tuple(case), TICKS)


@functools.lru_cache(maxsize=None)
def learner_data(l):
    """Learner l's networks, targets, normalisation and ring (read only)."""
    d = dict(WR.critic_data(100 + l, CAP))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def priorities(l):
    """Learner l's initial priorities [CAP] (read only): "heavy" for DUP_LEARNER, four decades for every other learner."""
    p = PC.priorities("heavy" if l == DUP_LEARNER else "decades", CAP, CAP, np.random.default_rng(900 + l))
    p.setflags(write=False)
    return p


def draw(l, tick, batch, prio=None, pmax=1.0, fresh=(0, 0), beta=BETA, ring_len=CAP, capacity=CAP):
    """The twin's draw of learner l (steps 1-4): per_ref.sample with the key RNG_SEED + l.  Returns (dict, prio after the fresh fill)."""
    p = np.array(priorities(l) if prio is None else prio, f32)
    return PR.sample(p, pmax, capacity, ring_len, fresh[0], fresh[1], RNG_SEED + l, tick, batch, beta), p


def minibatch(l, slots):
    d = learner_data(l)
    j = np.asarray(slots, np.int64)
    return d["s"][j], d["a"][j], d["r"][j], d["s2"][j], d["done"][j].astype(bool)


def per_learner(l, pa=None, pc=None, pa_t=None, pc_t=None):
    """tests/per_ref.py's learner (the weighted head on the oracle) on learner l's networks, or on the given ones."""
    d = learner_data(l)
    P = PR.PerLearner(np.array(d["pa"] if pa is None else pa), np.array(d["pc"] if pc is None else pc), d["s_min"], d["s_max"])
    P.actor_t, P.critic_t = np.array(d["pa_t"] if pa_t is None else pa_t), np.array(d["pc_t"] if pc_t is None else pc_t)
    return P


def target_y(P, r, s2, done, gamma=DO.GAMMA):
    """y = r + gamma (1 - done) critic_t(s', actor_t(s')) in float32, with a learner's own gamma (DO.Learner.targets has the shared one)."""
    s2n = DO.normalize(s2, P.s_min, P.s_max)
    q2 = DO.critic_forward(P.critic_t, s2n, DO.actor_forward(P.actor_t, s2n))
    return (r + f32(gamma) * (f32(1) - done.astype(f32)) * q2).astype(f32)


@functools.lru_cache(maxsize=None)
def twin_update(l, tick, batch, beta=BETA):
    """One prioritized update of learner l from its INITIAL state on the twin: the draw, the float32 oracle's y / diff, the write-back.
    Returns a read-only dict: idx, slots, w, T, diff, prio (after), pmax (after), writer {slot: column}."""
    tw, p = draw(l, tick, batch, beta=beta)
    j = tw["slots"][:batch]
    s, a, r, s2, done = minibatch(l, j)
    P = per_learner(l)
    y = P.targets(r, s2, done)
    _, _, diff = P.critic_grad_w(s, a, y, tw["w"][:batch])
    pmax = PR.write_back(p, 1.0, j, diff, EPS_P, ALPHA)
    out = dict(idx=tw["idx"], slots=tw["slots"], w=tw["w"], T=tw["T"], diff=diff, prio=p, pmax=pmax,
               writer={int(slot): m for m, slot in enumerate(j)}, y=y)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def duplicates(slots):
    """(slots drawn by more than one column, slots drawn by exactly one)."""
    u, c = np.unique(np.asarray(slots), return_counts=True)
    return u[c > 1], u[c == 1]


def tied_units(p, x, in_dim, out_dim):
    """[(index of the unit's bias in the flat parameter vector, sign of its closest-to-zero float64 pre-activation)]"""
    _, (_, z1, _, z2, _, _) = DO.mlp_forward(p, x, in_dim, out_dim, out_dim == 2, keep=True, dtype=np.float64)
    out = []
    for z, off in ((z1, in_dim * 250), (z2, in_dim * 250 + 250 + 250 * 500)):
        for u in np.unique(np.where(np.abs(z) < TIE)[1]):
            col = z[:, u]
            out.append((off + int(u), float(np.sign(col[np.argmin(np.abs(col))]) or 1.0)))
    return out


def initial_ties(l, tick, batch):
    """Tied relus of the float64 evaluation from learner l's INITIAL state on the twin's slots: the critic on [s_n; a], the actor on s_n."""
    d = learner_data(l)
    s, a, _, _, _ = minibatch(l, twin_update(l, tick, batch)["slots"][:batch])
    sn = DO.normalize(s, d["s_min"], d["s_max"])
    return ([("critic", l, tick)] * bool(tied_units(d["pc"], np.concatenate([sn, a], 1), 11, 1)) +
            [("actor", l, tick)] * bool(tied_units(d["pa"], sn, 9, 2)))


def sampler_edge_cases():
    """tests/per_cases.py's sampler cases at capacity <= CAP (ring_len 1 / 255 / 256 / 257 / 1 000 x batch 1 / 17 / 120 / 128; zeros, one
    slot, last block, decades; the fresh ranges; beta = 0): [(name, case)].  The 24 000-slot ring is BIG, run at L = 2 alone."""
    return [(n, c) for n, c in PC.sampler_cases() if c["capacity"] <= CAP]

"""The cases of the grouped TD3 update (td3.TD3LearnerGroup, shems_td3_group_update_tp), kept in ONE place: tests/test_group_td3_gpu.py
runs them on the device, tests/test_group_td3_host.py proves on the CPU -- on the NumPy twin (tests/td3_ref.py) alone -- that the seeds
and ticks chosen here meet the coverage and tie conditions the GPU cases assert.  TEST INFRASTRUCTURE ONLY.

Shapes of tests/test_group_imitation_gpu.py: 32 envs per learner, rings of 128 synthetic slots (tests/warmstart_ref.py: critic_data, a
different seed per learner).  The actor target's b3 is lifted to (1.5, -1.5) so that a~' reaches the clamp, sigma_trg = clip_trg = 0.5 so
that eps reaches the clip.  Learner l samples with the Philox key RNG_SEED + l and draws its target noise from the same key."""
import functools

import numpy as np

import ddpg_oracle as DO
import imitation_ref as IR
import td3_ref as TR
import warmstart_ref as WR

f32 = np.float32
E, CAP = 32, IR.CLONE_CAP
SEED, RNG_SEED = 21, 77
SIGMA, CLIP = 0.5, 0.5
C2_OFFSET = 1000
TICKS = (3, 4)
TIE = 1e-7                             # a relu whose float64 pre-activation is this close to zero may be decided either way
COVERAGE_FROM = 17                     # batch 1 is column 0 alone: exempt

# (learners, batch, policy step?): 2 learners run the narrow launch shapes, 48 the wide ones
STAGE_CASES = [(2, 1, True), (2, 17, True), (2, 128, True), (48, 120, True), (2, 17, False)]
# the comparisons that needed a tied relu decided the other way: [(network, learner, tick)]
EXPECTED_TIES = {c: [] for c in STAGE_CASES}
# The two ticks of a case.  The second update starts from the device's own bytes, so its relus cannot be looked at on the CPU beforehand:
# at (48, 120, policy) tick 4 puts a layer-2 pre-activation of learner 0's actor pass within TIE of zero (seen on the device: the block
# then needed the other decision), tick 5 does not.
CASE_TICKS = {(48, 120, True): (3, 5)}
# two learners with their own batch, eta_crit and gamma (test 5)
RECORD_CASE = [dict(batch=17, eta_crit=2e-3, gamma=0.9), dict(batch=120, eta_crit=5e-4, gamma=0.99)]


def checked(L):
    return (0, L - 1)


def ticks_of(case):
    return CASE_TICKS.get(tuple(case), TICKS)


@functools.lru_cache(maxsize=None)
def learner_data(l):
    """Learner l's networks, targets, normalisation and ring (read only)."""
    d = dict(WR.critic_data(100 + l, CAP))
    rng = np.random.default_rng(6000 + l)      # (chosen on the CPU: with 5000 + l the float64 evaluation of two cases has a tied relu)
    n = len(d["pc"])
    pa_t = d["pa_t"].copy()
    pa_t[len(pa_t) - 2:] = (1.5, -1.5)
    pc2 = DO.init_params(SEED + l + C2_OFFSET, 11, 1, 1)
    pc2[n - 501:n - 1] *= 30.0
    pc2[11 * 250:11 * 250 + 250] = rng.normal(0, 0.05, 250)
    pc2_t = (pc2 + rng.normal(0, 1e-3, n)).astype(f32)
    # two independently initialised critics differ by an offset larger than their spread over a minibatch: critic2_t's b3 is shifted by
    # the ring's median q'1 - q'2 (at the unsmoothed target action), so that both argmins of the twin minimum occur
    s2n = DO.normalize(d["s2"], d["s_min"], d["s_max"])
    a_t = DO.actor_forward(pa_t, s2n)
    pc2_t[n - 1] += f32(np.median(DO.critic_forward(d["pc_t"], s2n, a_t) - DO.critic_forward(pc2_t, s2n, a_t)))
    d.update(pa_t=pa_t, pa_t_plain=d["pa_t"], pc2=pc2, pc2_t=pc2_t)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def twin_of(pa, pa_t, pc, pc_t, pc2, pc2_t, s_min, s_max, sigma=SIGMA, clip=CLIP):
    tw = TR.Twin(np.array(pa), np.array(pc), np.array(pc2), s_min, s_max, sigma, clip)
    tw.L.actor_t, tw.L.critic_t, tw.L2.critic_t = np.array(pa_t), np.array(pc_t), np.array(pc2_t)
    return tw


def twin(l, sigma=SIGMA, clip=CLIP):
    d = learner_data(l)
    return twin_of(d["pa"], d["pa_t"], d["pc"], d["pc_t"], d["pc2"], d["pc2_t"], d["s_min"], d["s_max"], sigma, clip)


def minibatch(l, tick, batch, length=CAP):
    d = learner_data(l)
    idx = DO.sample_indices(RNG_SEED + l, tick, batch, length)
    return d["s"][idx], d["a"][idx], d["r"][idx], d["s2"][idx], d["done"][idx].astype(bool)


@functools.lru_cache(maxsize=None)
def stage(l, tick, batch):
    """The twin's target stage of learner l's INITIAL state at (tick, batch): computed once, read only."""
    s, a, r, s2, done = minibatch(l, tick, batch)
    tg = twin(l).targets(r, s2, done, RNG_SEED + l, tick)
    for v in tg.values():
        v.setflags(write=False)
    return tg


def coverage(tg):
    raw = f32(SIGMA) * tg["z"]
    return dict(clipped=int((np.abs(raw) > CLIP).sum()), clamped=int((np.abs(tg["a_t"] + tg["eps"]) > 1).sum()),
                at_one=int((np.abs(tg["a_smooth"]) == 1).sum()), pick1=int((tg["q1"] <= tg["q2"]).sum()), pick2=int((tg["q2"] < tg["q1"]).sum()))


def assert_coverage(l, tick, batch):
    """What TD3 adds is exercised -- asserted on the twin before any device result is looked at."""
    c = coverage(stage(l, tick, batch))
    print(f"learner {l}, tick {tick}, batch {batch}: {c}")
    if batch >= COVERAGE_FROM:
        assert c["clipped"] >= 1 and c["clamped"] >= 1 and c["at_one"] >= 1 and c["pick1"] >= 1 and c["pick2"] >= 1, (l, tick, batch, c)
    return c


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
    """Tied relus of the float64 evaluation from learner l's INITIAL state: both critics on [s_n; a], the actor on s_n."""
    d = learner_data(l)
    s, a, _, _, _ = minibatch(l, tick, batch)
    sn = DO.normalize(s, d["s_min"], d["s_max"])
    x = np.concatenate([sn, a], 1)
    return ([("critic", l, tick)] * bool(tied_units(d["pc"], x, 11, 1)) + [("critic2", l, tick)] * bool(tied_units(d["pc2"], x, 11, 1)) +
            [("actor", l, tick)] * bool(tied_units(d["pa"], sn, 9, 2)))

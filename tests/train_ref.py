"""The followed ("teacher-forced") trajectory of the training loop.  TEST INFRASTRUCTURE ONLY: plain NumPy + the C oracle, no torch.

The loop under test is episode! (DDPG.jl:186-242) for a whole batch: TrainWorkload.step / shems_train_steps / GroupWorkload.step.
Per vector step t the follower reads the state of the "device under test" before and after the step (through a small adapter) and,
FROM THE STATE BEFORE, holds everything the step did to its oracle:

    boundary   t > 0 and t % 72 == 0: the state act() saw is the seeded reset of (env_seed, episode + 1) (philox_np.reset_draws +
               oracle_c.Batch.reset); otherwise the previous post-step state
    act        the unscaled actions against DO.act(actor BEFORE the step, pre-state, ..., tick = t) in float64 -- which actor act(t)
               reads; the actions of the remembered envs are the ring's, the others come from the adapter's shadow launch
    shadow     the shadow launch's bytes on the remembered envs are the ring's
    env        oracle_c stepped with scale_action of those actions: obs, idx, step and the float32 rewards bit for bit
    ring       slots (pushed + rel) % cap for the envs with rel = (i - (t * win) % E) % E < win hold (pre-state, action, float32
               reward, next state, done = 0) bit for bit, every other slot of the five arrays keeps its bytes, pushed advanced by win
    sampler    the update's slots are DO.sample_indices(rng_seed + l, update count, batch, min(pushed AFTER the insert, cap))
    targets    y against float64 from the TARGET networks of the state before
    critic_grad / actor_grad / losses   per Flux.params block against float64 (the actor's through the kernel's UPDATED critic)
    adam / soft_update   element-wise from the kernel's own gradient, the moments of the state before and bp = beta^(u + 1)
    counters   t, episode, updates and the Float64 beta powers advanced as DDPG.jl / Flux advance them

Then it adopts the state after the step and goes on: divergence cannot accumulate, so the single-update bounds hold at every step.

The adapter (see tests/test_train_follow_host.py for a CPU one, tests/test_train_follow_gpu.py for the device ones) has
    n, count, E            envs, learners, envs per learner (n = count * E; learner l owns envs [l E, (l + 1) E))
    cap, batch, updates    ring capacity, minibatch size, updates per vector step
    env_seed, act_seed, rng_seed    keys of the seeded reset, of the exploration noise (global env index), of learner 0's sampler
    table, profile         the envs' table and oracle_c profile (one config: mixed batches are held in test_fused_configs_gpu.py)
    ws_idx, ws_y           float offsets of the sampled slots (int32) / of y inside a learner's workspace, None where not readable
    window(t) -> (win, offset)      transitions each learner remembers at step t and the window's rotation inside its block
    snapshot() -> Snap     everything below, copied to the host
    step() -> [learner states]      one vector step; returns the learner states between the step's updates (updates - 1 of them)
    shadow(learner state, obs, idx, step, tick) -> actions [n][2]   (or shadow = None) a second launch of the fused step
"""
from __future__ import annotations

import json

import numpy as np

import util as U                     # noqa: F401  (puts oracle/ on the path)
import ddpg_oracle as DO
import oracle_c
import philox_np
import test_ddpg_gpu as TD
import test_group_gpu as TG

NETS = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic")
LEARNER_KEYS = NETS + ("grad_actor", "grad_critic", "losses", "ws", "s_min", "s_max")
RING_KEYS = ("s", "a", "r", "s2", "done")
EP_LEN = 72
ACT_TOL = 5e-6 + 1e-5                 # the fused step's action bound (tests/test_policy_gpu.py)
BLOCK_TOL = TD.BLOCK_TOL
WS_IDX, WS_Y = 30 * 128, 22 * 128     # csrc/shems_ddpg.hip's workspace: sampled slots (int32), y (tests/test_ddpg_gpu.py reads both)
WS_IDX_TP = 2 * 12 * 128 + 2 * 128    # csrc/shems_gupd.hip's (tests/test_group_gpu.py)
MAX_WIDENED = 0.1                     # at most 1 in 10 block comparisons of a case may take the f32 oracle's widened bound


class FollowError(AssertionError):
    """A followed step missed a check; `check` names it."""

    def __init__(self, check, msg):
        super().__init__(f"[{check}] {msg}")
        self.check = check


def _need(ok, check, msg):
    if not ok:
        raise FollowError(check, msg() if callable(msg) else msg)


class Snap:
    """The state of the loop between two vector steps, on the host.
    obs [n][9] f32, idx [n], step [n]; learners: per learner {LEARNER_KEYS: array}; rings: per learner {RING_KEYS: array};
    t, episode, updates; pushed: per learner; bp_actor, bp_critic: [beta1^k, beta2^k] Float64; rew32 [n] f32 or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


class _Bounds:
    """Stands where test_ddpg_gpu stands in test_group_gpu._assert_blocks_or_the_other_relu_decision: the per-block bound of one gradient
    comparison.  BLOCK_TOL of the block's max-abs, except (a) the critic's b3 -- ONE element, the signed mean of the residuals
    2 (q - y) / B, which cancels towards zero as the critic fits -- is held as |g - g64| <= BLOCK_TOL * sum_m |2 (q64_m - y_m) / B|;
    (b) where the f32 NumPy oracle's own error on the same inputs exceeds BLOCK_TOL / 2, the bound of that block is 4 x that error
    (the rule BLOCK_TOL itself was made by); every such widening is recorded and printed."""

    def __init__(self, g32, b3_scale, tag):
        self.g32, self.b3_scale, self.tag = g32, b3_scale, tag
        self.best32 = None
        self.last = None

    def _errs(self, g, g64, in_dim, out_dim):
        out = {}
        for name, lo, hi in DO.blocks(in_dim, out_dim):
            scale = max(np.abs(g64[lo:hi]).max(), 1e-30)
            if name == "b3" and self.b3_scale is not None:
                scale = max(self.b3_scale, 1e-30)
            out[name] = float(np.abs(g[lo:hi] - g64[lo:hi]).max() / scale)
        return out

    def _assert_blocks(self, g, g64, in_dim, out_dim, what, tol=BLOCK_TOL):
        for name, lo, hi in DO.blocks(in_dim, out_dim):
            assert np.abs(g64[lo:hi]).max() > 0, (what, name, "reference block is all zero: the step does not exercise it")
        errs, e32 = self._errs(g, g64, in_dim, out_dim), self._errs(self.g32, g64, in_dim, out_dim)
        if self.best32 is not None:               # second evaluation (tied relus the other way): the f32 oracle's error is its distance to
            e32 = {k: min(v, self.best32[k]) for k, v in e32.items()}      # the evaluation that decides the relus as IT did
        self.best32 = e32
        tols = {k: (4 * e32[k] if e32[k] > tol / 2 else tol) for k in errs}
        self.last = dict(errs=errs, e32=e32, widened=[k for k in errs if e32[k] > tol / 2])
        bad = {k: (e, tols[k]) for k, e in errs.items() if not e <= tols[k]}
        assert not bad, (what, "block: (error, bound)", bad, "all blocks", errs, "f32 oracle", e32)
        return errs


class Follower:
    def __init__(self, adapter, case="", collect=False):
        """collect: keep going after a missed check (measuring runs): the misses are kept in `failures`."""
        self.ad, self.case, self.collect = adapter, case, collect
        ad = adapter
        assert ad.n == ad.count * ad.E
        self.ref = oracle_c.Batch(ad.n, EP_LEN, ad.table, ad.profile)
        self.last = None
        self.steps, self.wrapped, self.boundaries = [], [], []
        self.ties = []                    # (case, network, step) -- (case, network, step, learner / update) where there are several
        self.worst, self.worst32 = {}, {}  # per block: the device's worst error, the f32 oracle's on the same comparison
        self.oracle_worst = {}            # per block: the f32 oracle's own worst error over the stretch
        self.comparisons, self.widened = 0, []
        self.act_err = 0.0
        self.failures = []

    # ------------------------------------------------------------------ one step
    def step(self):
        before = self.ad.snapshot() if self.last is None else self.last
        mids = self.ad.step()
        after = self.ad.snapshot()
        self.last = after
        try:
            self.check(before, mids, after)
        except FollowError as e:
            if not self.collect:
                raise
            self.failures.append((before.t, e.check, str(e)[:2000]))
        return after

    def follow(self, k):
        for _ in range(int(k)):
            self.step()
        return self

    def _guard(self, fn, *a):
        try:
            return fn(*a)
        except FollowError as e:
            if not self.collect:
                raise
            self.failures.append((a[-1] if a else None, e.check, str(e)[:2000]))

    def check(self, b, mids, a):
        ad, ref = self.ad, self.ref
        n, E, cap, t = ad.n, ad.E, ad.cap, int(b.t)
        self.steps.append(t)
        boundary = t > 0 and t % EP_LEN == 0
        episode = int(b.episode) + (1 if boundary else 0)
        # ---- the state act() saw
        if boundary:
            self.boundaries.append(t)
            i0, s0 = philox_np.reset_draws(ad.env_seed, episode, n, ad.table.shape[0], EP_LEN, ad.profile.soc_max)
            ref.reset(False, i0, s0)
            pre_obs, pre_idx, pre_step = ref.state().copy(), ref.idx().copy(), ref.steps().copy()
            _need((pre_step == 0).all(), "boundary", "the oracle's reset leaves step != 0")
            _need((a.idx.astype(np.int64) == pre_idx + 1).all() and (a.step == 1).all(), "boundary",
                  lambda: f"step {t}: the rows after the step are not one past the seeded reset of (env_seed, episode {episode}): "
                          f"{int((a.idx.astype(np.int64) != pre_idx + 1).sum())} of {n} envs differ")
        else:
            pre_obs, pre_idx, pre_step = b.obs, b.idx.astype(np.int64), b.step.astype(np.int64)
        # ---- the window: which envs are remembered, and where
        win, off = ad.window(t)
        j = np.arange(E)
        rel = (j - off) % E
        stored_local = rel < win
        known = np.zeros(n, bool)
        a_dev = np.full((n, 2), np.nan, np.float32)
        slots_of, envs_of = [], []
        for l in range(ad.count):
            pos = int(b.pushed[l])
            if pos % cap + win >= cap:
                if t not in self.wrapped:
                    self.wrapped.append(t)
            envs = l * E + j[stored_local]
            slots = (pos + rel[stored_local]) % cap
            slots_of.append(slots); envs_of.append(envs)
            _need(_same(a.rings[l]["s"][slots], pre_obs[envs]), "ring",
                  lambda: f"step {t}, learner {l}: ring.s at the window's slots is not the pre-step state of the window's envs "
                          f"(window {win} from offset {off}, slots from {pos % cap})")
            a_dev[envs] = a.rings[l]["a"][slots]
            known[envs] = True
        # ---- act: which actor, which tick, which normalisation (the remembered envs first: their actions are the loop's own)
        a64 = np.empty((n, 2), np.float32)
        for l in range(ad.count):
            Lb = b.learners[l]
            a64[l * E:(l + 1) * E] = DO.act(Lb["actor"], pre_obs, Lb["s_min"], Lb["s_max"], True, ad.act_seed, tick=t, dtype=np.float64)[l * E:(l + 1) * E]

        def act_check(which, whose):
            err = float(np.abs(a_dev[which] - a64[which]).max())
            self.act_err = max(self.act_err, err)
            _need(err < ACT_TOL, "act", f"step {t}: {whose} actions are {err:.3g} from act(actor before the step, tick {t}) in float64 (bound {ACT_TOL:.3g})")
            _need(np.abs(a_dev[which]).max() <= 1.0, "act", f"step {t}: {whose} actions outside [-1, 1] (scale_action's output was stored?)")
        act_check(known.copy(), "the remembered")
        if not known.all() and ad.shadow is not None:
            assert ad.count == 1
            sh = np.asarray(ad.shadow(b.learners[0], pre_obs, pre_idx, pre_step, t), np.float32)
            _need(_same(sh[known], a_dev[known]), "shadow", f"step {t}: the shadow launch's actions differ from ring.a on the window's envs")
            a_dev[~known] = sh[~known]
            act_check(~known, "the shadow launch's")
            known[:] = True
        # ---- env
        ref.set_state(pre_obs, pre_idx, pre_step)
        rc, r64, obs2, _ = ref.step(oracle_c.scale_action(np.where(known[:, None], a_dev, a64)), 0)
        _need(rc == 0, "env", f"step {t}: the oracle refused the step")
        r32 = r64.astype(np.float32)
        _need((a.idx.astype(np.int64) == ref.idx()).all() and (a.step.astype(np.int64) == ref.steps()).all(), "env", f"step {t}: idx / step differ from the oracle")
        _need(_same(a.obs[known], obs2[known]), "env",
              lambda: f"step {t}: {int((_bits(a.obs) != _bits(obs2)).any(1).sum())} envs' observations differ from the oracle stepped with the device's actions")
        if a.rew32 is not None:
            _need(_same(a.rew32[known], r32[known]), "env", f"step {t}: float32 rewards differ from the oracle's")
        # ---- ring: the whole arrays against the mirror
        mirror = [{k: v.copy() for k, v in ring.items()} for ring in b.rings]
        for l in range(ad.count):
            m, slots, envs = mirror[l], slots_of[l], envs_of[l]
            m["s"][slots], m["a"][slots], m["r"][slots], m["s2"][slots], m["done"][slots] = pre_obs[envs], a_dev[envs], r32[envs], obs2[envs], 0
            for k in RING_KEYS:
                _need(_same(a.rings[l][k], m[k]), "ring",
                      lambda: f"step {t}, learner {l}: ring.{k} differs from the mirror in {int((_bits(a.rings[l][k]) != _bits(m[k])).reshape(cap, -1).any(1).sum())} slots")
            _need(int(a.pushed[l]) == int(b.pushed[l]) + win, "ring", f"step {t}, learner {l}: pushed {b.pushed[l]} -> {a.pushed[l]}, window {win}")
        # ---- the updates
        chain = [b.learners] + list(mids) + [a.learners]
        _need(len(chain) == ad.updates + 1, "counters", f"step {t}: {len(chain) - 1} learner states for {ad.updates} updates")
        for k in range(ad.updates):
            for l in range(ad.count):
                self._guard(self.check_update, l, chain[k][l], chain[k + 1][l], mirror[l], int(b.updates) + k, min(int(a.pushed[l]), cap), k, t)
        # ---- counters
        _need(int(a.t) == t + 1 and int(a.episode) == episode, "counters", f"step {t}: t -> {a.t}, episode {b.episode} -> {a.episode} (expected {episode})")
        _need(int(a.updates) == int(b.updates) + ad.updates, "counters", f"step {t}: updates {b.updates} -> {a.updates}")
        for name in ("bp_actor", "bp_critic"):
            have, was = getattr(a, name), getattr(b, name)
            want = [float(was[0]), float(was[1])]
            for _ in range(ad.updates):
                want = [want[0] * 0.9, want[1] * 0.999]                     # Flux: beta_t .*= beta, in Float64
            u = int(b.updates)
            _need(abs(was[0] - 0.9 ** (u + 1)) <= 1e-13 and abs(was[1] - 0.999 ** (u + 1)) <= 1e-13, "counters",
                  f"step {t}: {name} before the step is {list(was)}, not beta^{u + 1}")
            _need(float(have[0]) == want[0] and float(have[1]) == want[1], "counters", f"step {t}: {name} {list(was)} -> {list(have)}, expected {want}")

    # ------------------------------------------------------------------ one update of one learner
    def _tie_tag(self, net, t, l, k):
        ad = self.ad
        return (self.case, net, t) + ((l,) if ad.count > 1 else ()) + ((k,) if ad.updates > 1 else ())

    def _record(self, kind, bounds, tag):
        self.comparisons += len(bounds.last["errs"])
        for blk, e in bounds.last["errs"].items():
            key = f"{kind}.{blk}"
            if e > self.worst.get(key, -1.0):
                self.worst[key], self.worst32[key] = e, bounds.last["e32"][blk]
            self.oracle_worst[key] = max(self.oracle_worst.get(key, 0.0), bounds.last["e32"][blk])
        for blk in bounds.last["widened"]:
            self.widened.append((tag, blk, bounds.last["e32"][blk]))
            print(f"widened bound: {tag} {kind}.{blk}: f32 oracle {bounds.last['e32'][blk]:.3g} of the block -> bound {4 * bounds.last['e32'][blk]:.3g}")

    def check_update(self, l, B, A, ring, u, ring_len, k, t):
        ad = self.ad
        nb = ad.batch
        where = f"step {t}, learner {l}, update {u}"
        idx = DO.sample_indices(ad.rng_seed + l, u, nb, ring_len)
        if ad.ws_idx is not None:
            got = np.ascontiguousarray(A["ws"][ad.ws_idx:ad.ws_idx + nb]).view(np.int32)
            _need(np.array_equal(got, idx), "sampler",
                  lambda: f"{where}: sampled slots are not sample_indices(seed {ad.rng_seed + l}, tick {u}, {nb}, ring_len {ring_len}); first: {got[:6]} / {idx[:6]}")
        s, a, r, s2, done = (ring[key][idx] for key in RING_KEYS)
        s_min, s_max = B["s_min"], B["s_max"]
        Lr = DO.Learner(B["actor"], B["critic"], s_min, s_max)
        Lr.actor_t, Lr.critic_t = B["actor_t"], B["critic_t"]
        y = Lr.targets(r, s2, done.astype(bool))
        sn, s2n = DO.normalize(s, s_min, s_max), DO.normalize(s2, s_min, s_max)
        q2 = DO.critic_forward(B["critic_t"], s2n, DO.actor_forward(B["actor_t"], s2n, dtype=np.float64), dtype=np.float64)
        y64 = r.astype(np.float64) + float(DO.GAMMA) * (1.0 - done.astype(np.float64)) * q2
        _need(np.allclose(y, y64, rtol=2e-5, atol=2e-5), "targets", f"{where}: the f32 oracle's y is off float64")
        if ad.ws_y is not None:
            Y = A["ws"][ad.ws_y:ad.ws_y + nb]
            _need(np.allclose(Y, y64, rtol=2e-5, atol=2e-5), "targets",
                  lambda: f"{where}: y is {np.abs(Y - y64).max():.3g} from r + gamma (1 - done) critic_t(s', actor_t(s')) in float64")
        # critic: gradient, loss, ADAM, soft update
        gc = A["grad_critic"]
        gc64, lc64 = Lr.critic_grad(s, a, y, dtype=np.float64)
        gc32, _ = Lr.critic_grad(s, a, y)
        xin = np.concatenate([sn, a], 1)
        q64 = DO.critic_forward(B["critic"], sn, a, dtype=np.float64)
        b3_scale = float(np.abs(2.0 * (q64 - y) / nb).sum())

        def crit_eval(P):
            return DO.Learner(B["actor"], P["critic"], s_min, s_max).critic_grad(s, a, y, dtype=np.float64)[0]
        bounds = _Bounds(gc32, b3_scale, where)
        try:
            _, tie = TG._assert_blocks_or_the_other_relu_decision(bounds, gc, crit_eval, {"critic": (B["critic"], xin, 11, 1)}, 11, 1,
                                                                  f"critic gradient, {where}: vs float64")
        except AssertionError as e:
            raise FollowError("critic_grad", str(e)[:3000]) from None
        self._record("critic", bounds, where)
        if tie:
            self.ties.append(self._tie_tag("critic", t, l, k))
        _need(abs(float(A["losses"][0]) - lc64) < 1e-4 * max(1.0, abs(lc64)), "losses", f"{where}: critic loss {A['losses'][0]} against {lc64}")
        opt = DO.Adam(len(gc), DO.ETA_CRIT)
        opt.m, opt.v, opt.bp = B["m_critic"].copy(), B["v_critic"].copy(), [0.9 ** (u + 1), 0.999 ** (u + 1)]
        pc1 = opt.step(B["critic"], gc)
        crit = A["critic"]
        _need(np.allclose(crit, pc1, rtol=0, atol=1e-7), "adam", lambda: f"{where}: critic is {np.abs(crit - pc1).max():.3g} from ADAM(bp = beta^{u + 1}) of the kernel's gradient")
        _need(np.allclose(A["m_critic"], opt.m, rtol=1e-6, atol=1e-12) and np.allclose(A["v_critic"], opt.v, rtol=1e-6, atol=1e-15), "adam",
              f"{where}: the critic's ADAM moments")
        ct = DO.soft_update(B["critic_t"], crit)
        _need(np.allclose(A["critic_t"], ct, rtol=0, atol=1e-7), "soft_update", lambda: f"{where}: critic_t is {np.abs(A['critic_t'] - ct).max():.3g} from (1 - tau) critic_t + tau critic")
        # actor: through the kernel's UPDATED critic (DDPG.jl:137-140)
        Lr.critic = crit
        ga = A["grad_actor"]
        ga64, la64 = Lr.actor_grad(s, dtype=np.float64)
        ga32, _ = Lr.actor_grad(s)
        a_pi = DO.actor_forward(B["actor"], sn, dtype=np.float64)

        def act_eval(P):
            return DO.Learner(P["actor"], P["critic"], s_min, s_max).actor_grad(s, dtype=np.float64)[0]
        bounds = _Bounds(ga32, None, where)
        try:
            _, tie = TG._assert_blocks_or_the_other_relu_decision(bounds, ga, act_eval, {"actor": (B["actor"], sn, 9, 2), "critic": (crit, np.concatenate([sn, a_pi], 1), 11, 1)},
                                                                  9, 2, f"actor gradient, {where}: vs float64 through the updated critic")
        except AssertionError as e:
            raise FollowError("actor_grad", str(e)[:3000]) from None
        self._record("actor", bounds, where)
        if tie:
            self.ties.append(self._tie_tag("actor", t, l, k))
        _need(abs(float(A["losses"][1]) - la64) < 1e-4 * max(1.0, abs(la64)), "losses", f"{where}: actor loss {A['losses'][1]} against {la64}")
        opt = DO.Adam(len(ga), DO.ETA_ACT)
        opt.m, opt.v, opt.bp = B["m_actor"].copy(), B["v_actor"].copy(), [0.9 ** (u + 1), 0.999 ** (u + 1)]
        pa1 = opt.step(B["actor"], ga)
        act = A["actor"]
        _need(np.allclose(act, pa1, rtol=0, atol=1e-7), "adam", lambda: f"{where}: actor is {np.abs(act - pa1).max():.3g} from ADAM(bp = beta^{u + 1}) of the kernel's gradient")
        _need(np.allclose(A["m_actor"], opt.m, rtol=1e-6, atol=1e-12) and np.allclose(A["v_actor"], opt.v, rtol=1e-6, atol=1e-15), "adam",
              f"{where}: the actor's ADAM moments")
        at = DO.soft_update(B["actor_t"], act)
        _need(np.allclose(A["actor_t"], at, rtol=0, atol=1e-7), "soft_update", lambda: f"{where}: actor_t is {np.abs(A['actor_t'] - at).max():.3g} from (1 - tau) actor_t + tau actor")

    # ------------------------------------------------------------------ what a case asserts at its end
    def report(self):
        return dict(case=self.case, steps=self.steps, wrapped=self.wrapped, boundaries=self.boundaries, ties=self.ties,
                    comparisons=self.comparisons, widened=len(self.widened), act_err=self.act_err,
                    worst={k: (self.worst[k], self.worst32[k]) for k in sorted(self.worst)},
                    oracle_worst={k: self.oracle_worst[k] for k in sorted(self.oracle_worst)}, failures=self.failures)

    def assert_case(self, expected_ties):
        """The stretch held the ring's wrap-around and an episode boundary, every reference block was non-zero (asserted per comparison),
        the comparisons that needed the second relu evaluation are exactly the committed ones, at most 1 in 10 took a widened bound."""
        print("followed trajectory: " + json.dumps(self.report(), default=str))
        assert not self.failures, self.failures
        assert self.wrapped, (self.case, "no followed step wrapped the ring's end", self.steps)
        assert self.boundaries, (self.case, "no followed step crossed an episode boundary", self.steps)
        assert self.comparisons >= 12 * len(self.steps) * self.ad.count * self.ad.updates, (self.case, self.comparisons)
        assert self.ties == list(expected_ties), (self.case, self.ties, list(expected_ties))
        assert len(self.widened) <= MAX_WIDENED * self.comparisons, (self.case, self.widened, self.comparisons)

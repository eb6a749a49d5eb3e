"""The follower of tests/train_ref.py proven on the CPU: a stand-in "device" -- the C oracle as the env, DO.act / DO.Learner.replay in
float32 as the learner, composed in episode!'s order (DDPG.jl:186-242) -- passes a followed stretch across t = 72 that also wraps
the ring's end and fills the ring on the way; every deliberately wrong composition of the same pieces fails, and fails at the check
named for it.  This is the evidence that tests/test_train_follow_gpu.py would notice a subtly wrong loop."""
import numpy as np
import pytest

import util as U                      # noqa: F401
import ddpg_oracle as DO
import oracle_c
import philox_np
import train_ref as TR

f32 = np.float32
N, WIN, CAP, T0 = 20, 7, 200, 70      # 20 envs, 7 remembered per step (the rotation wraps the batch every 3rd step), a 200-slot ring
PUSHED0 = 190                         # at t = 70: step 70 fills slots 190..196 (ring_len 197), step 71 wraps the end (197..203 -> 200 slots)


class HostLoop:
    """The adapter of train_ref.Follower over a CPU loop.  flaws: names of the wrong compositions to build in."""

    count, E, n, cap, batch = 1, N, N, CAP, 120
    env_seed = act_seed = rng_seed = 7
    ws_idx, ws_y = TR.WS_IDX, TR.WS_Y
    shadow = None

    def __init__(self, updates=1, flaws=(), with_shadow=True):
        self.updates, self.flaws = int(updates), set(flaws)
        S = U.pkg()
        self.table = S.tables.synthetic_table("train", 98)
        self.profile = oracle_c.profile(98)
        self.env = oracle_c.Batch(N, 72, self.table, self.profile)
        rng = np.random.default_rng(3)
        # a ring of PUSHED0 real transitions under uniform random actions (populate_memory's kind), from the episode-1 start
        self._reset(1)
        self.ring = dict(s=np.zeros((CAP, 9), f32), a=np.zeros((CAP, 2), f32), r=np.zeros(CAP, f32), s2=np.zeros((CAP, 9), f32), done=np.zeros(CAP, np.uint8))
        self.pushed = 0
        while self.pushed < PUSHED0:
            pre = self.env.state().copy()
            raw = (rng.random((N, 2)) * 2 - 1).astype(f32)
            _, r, obs, _ = self.env.step(oracle_c.scale_action(raw), 0)
            k = min(N, PUSHED0 - self.pushed)
            sl = slice(self.pushed, self.pushed + k)
            self.ring["s"][sl], self.ring["a"][sl], self.ring["r"][sl], self.ring["s2"][sl] = pre[:k], raw[:k], r[:k].astype(f32), obs[:k]
            self.pushed += k
        s = self.ring["s"][:PUSHED0]
        pa, pc = DO.init_params(1231, 9, 2, 0), DO.init_params(1231, 11, 1, 1)
        self.L = DO.Learner(pa, pc, s.min(0), s.max(0))
        self.grads = [np.zeros_like(pa), np.zeros_like(pc)]
        self.losses = np.zeros(2, f32)
        self.ws = np.zeros(31 * 128, f32)
        # the loop stands at t = T0 of episode 1, T0 * updates updates behind it; three of them are run so that the targets have left the
        # online networks and the moments are not zero
        self.t, self.episode, self.n_upd = T0, 1, T0 * self.updates - 3
        for opt in (self.L.opt_a, self.L.opt_c):
            opt.bp = [0.9 ** (self.n_upd + 1), 0.999 ** (self.n_upd + 1)]
        self.prev_actor = self.L.actor.copy()
        for _ in range(3):
            self._replay(self.n_upd, PUSHED0, self.ring, set())
        self.env.set_state(self.env.state(), self.env.idx(), np.full(N, T0, np.int64))
        self.rew32 = np.zeros(N, f32)
        if with_shadow:
            self.shadow = lambda Lb, obs, idx, step, tick: DO.act(Lb["actor"], obs, Lb["s_min"], Lb["s_max"], True, self.act_seed, tick=tick)

    def _reset(self, episode):
        i0, s0 = philox_np.reset_draws(self.env_seed, episode, N, self.table.shape[0], 72, self.profile.soc_max)
        self.env.reset(False, i0, s0)

    def window(self, t):
        return WIN, (t * WIN) % N

    def _learner(self):
        L = self.L
        return dict(actor=L.actor.copy(), critic=L.critic.copy(), actor_t=L.actor_t.copy(), critic_t=L.critic_t.copy(),
                    m_actor=L.opt_a.m.copy(), v_actor=L.opt_a.v.copy(), m_critic=L.opt_c.m.copy(), v_critic=L.opt_c.v.copy(),
                    grad_actor=self.grads[0].copy(), grad_critic=self.grads[1].copy(), losses=self.losses.copy(), ws=self.ws.copy(),
                    s_min=L.s_min.copy(), s_max=L.s_max.copy())

    def snapshot(self):
        L = self.L
        return TR.Snap(obs=self.env.state().copy(), idx=self.env.idx(), step=self.env.steps(), learners=[self._learner()],
                       rings=[{k: v.copy() for k, v in self.ring.items()}], t=self.t, episode=self.episode, pushed=[self.pushed],
                       updates=self.n_upd, bp_actor=list(L.opt_a.bp), bp_critic=list(L.opt_c.bp), rew32=self.rew32.copy())

    def _replay(self, tick, ring_len, ring, flaws):
        L = self.L
        idx = DO.sample_indices(self.rng_seed, tick, self.batch, ring_len)
        s, a, r, s2, done = (ring[k][idx] for k in TR.RING_KEYS)
        self.ws[TR.WS_IDX:TR.WS_IDX + self.batch] = idx.astype(np.int32).view(f32)
        if not flaws & {"online_targets", "old_critic", "stale_beta", "tau_side"}:
            self.ws[TR.WS_Y:TR.WS_Y + self.batch] = L.targets(r, s2, done.astype(bool))
            got = []
            lc, la = L.replay(s, a, r, s2, done.astype(bool), allreduce=lambda g: (got.append(g.copy()), g)[1])
            self.grads = [got[1], got[0]]
        else:                                                          # DO.Learner.replay's own lines, with the flaw built in
            if "online_targets" in flaws:
                s2n = DO.normalize(s2, L.s_min, L.s_max)
                y = (r + DO.GAMMA * (f32(1) - done.astype(f32)) * DO.critic_forward(L.critic, s2n, DO.actor_forward(L.actor, s2n))).astype(f32)
            else:
                y = L.targets(r, s2, done.astype(bool))
            self.ws[TR.WS_Y:TR.WS_Y + self.batch] = y
            if "stale_beta" in flaws:
                L.opt_c.bp, L.opt_a.bp = [0.9, 0.999], [0.9, 0.999]
            gc, lc = L.critic_grad(s, a, y)
            old = L.critic
            L.critic = L.opt_c.step(L.critic, gc)
            if "old_critic" in flaws:
                new, L.critic = L.critic, old
                ga, la = L.actor_grad(s)
                L.critic = new
            else:
                ga, la = L.actor_grad(s)
            L.actor = L.opt_a.step(L.actor, ga)
            if "tau_side" in flaws:
                L.actor_t = (DO.TAU * L.actor_t + (f32(1) - DO.TAU) * L.actor).astype(f32)
                L.critic_t = (DO.TAU * L.critic_t + (f32(1) - DO.TAU) * L.critic).astype(f32)
            else:
                L.actor_t, L.critic_t = DO.soft_update(L.actor_t, L.actor), DO.soft_update(L.critic_t, L.critic)
            if "stale_beta" in flaws:
                L.opt_c.bp, L.opt_a.bp = [0.9 ** (self.n_upd + 2), 0.999 ** (self.n_upd + 2)], [0.9 ** (self.n_upd + 2), 0.999 ** (self.n_upd + 2)]
            self.grads = [ga, gc]
        self.losses = np.array([lc, la], f32)
        self.n_upd += 1

    def step(self):
        fl, t = self.flaws, self.t
        if t and t % 72 == 0:
            if "stale_episode" not in fl:
                self.episode += 1
            self._reset(self.episode)
            if "stale_episode" in fl:
                self.episode += 1                 # (the counter itself moves: only the reset was handed the old number)
        pre = self.env.state().copy()
        actor = self.prev_actor if "stale_actor" in fl else self.L.actor
        a = DO.act(actor, pre, self.L.s_min, self.L.s_max, True, self.act_seed, tick=t)
        self.prev_actor = self.L.actor.copy()
        _, r, obs, _ = self.env.step(oracle_c.scale_action(a), 0)
        self.rew32 = r.astype(f32)
        before = {k: v.copy() for k, v in self.ring.items()}
        off = 0 if "no_rotation" in fl else (t * WIN) % N
        for i in range(N):
            rel = (i - off) % N
            if rel < WIN:
                slot = self.pushed % CAP + rel
                if slot >= CAP:
                    if "no_wrap" in fl:
                        continue                  # (the tail of the window is lost instead of landing at the ring's start)
                    slot -= CAP
                for k, v in (("s", pre[i]), ("a", a[i]), ("r", self.rew32[i]), ("s2", obs[i]), ("done", 0)):
                    self.ring[k][slot] = v
        self.pushed += WIN
        mids = []
        for k in range(self.updates):
            tick = t if "tick_is_t" in fl else self.n_upd
            if "sample_before_insert" in fl:
                self._replay(tick, min(self.pushed - WIN, CAP), before, fl)
            else:
                self._replay(tick, min(self.pushed, CAP), self.ring, fl)
            if k < self.updates - 1:
                mids.append([self._learner()])
        self.t += 1
        return mids


def test_faithful_loop_passes_six_followed_steps_across_the_episode_boundary_and_the_ring_wrap():
    fol = TR.Follower(HostLoop(), "host")
    fol.follow(6)
    assert fol.steps == [70, 71, 72, 73, 74, 75] and fol.boundaries == [72] and 71 in fol.wrapped
    fol.assert_case([])
    # the stand-in IS the f32 oracle: every gradient error recorded is the oracle's own, a widened bound included
    assert all(e == e32 for e, e32 in fol.report()["worst"].values())


def test_faithful_loop_with_two_updates_per_step_and_no_shadow():
    """Both updates of a step are followed, with ticks u and u + 1, from the learner state between them; without a shadow launch
    the envs outside the window are held for idx and step only."""
    fol = TR.Follower(HostLoop(updates=2, with_shadow=False), "host2")
    fol.follow(3)
    assert fol.comparisons == 3 * 2 * 12 and fol.last.updates == 2 * 70 + 6
    assert not fol.failures and fol.ties == []


# (flaw, updates per step, steps to follow, the check that must catch it)
WRONG = [("sample_before_insert", 1, 1, "sampler"),       # ring_len 190 instead of 197 at step 70
         ("tick_is_t", 2, 1, "sampler"),                   # tick 70 instead of the update count 140
         ("stale_episode", 1, 3, "boundary"),
         ("no_rotation", 1, 1, "ring"),
         ("no_wrap", 1, 2, "ring"),
         ("stale_actor", 1, 1, "act"),
         ("online_targets", 1, 1, "targets"),
         ("old_critic", 1, 1, "actor_grad"),
         ("stale_beta", 1, 1, "adam"),
         ("tau_side", 1, 1, "soft_update")]


@pytest.mark.parametrize("flaw,updates,steps,check", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_composition_fails_at_its_named_check(flaw, updates, steps, check):
    fol = TR.Follower(HostLoop(updates=updates, flaws=[flaw]), flaw)
    fol.follow(steps - 1)                                     # the steps before the flaw shows pass
    with pytest.raises(TR.FollowError) as e:
        fol.step()
    assert e.value.check == check, str(e.value)
    assert fol.last.t == T0 + steps


def test_targets_flaw_is_caught_by_the_gradient_where_the_workspace_is_not_readable():
    """The throughput group form keeps its own workspace layout: there the critic's gradient stands in for the y check."""
    ad = HostLoop(flaws=["online_targets"])
    ad.ws_y = None
    with pytest.raises(TR.FollowError) as e:
        TR.Follower(ad, "no-ws").step()
    assert e.value.check == "critic_grad", str(e.value)

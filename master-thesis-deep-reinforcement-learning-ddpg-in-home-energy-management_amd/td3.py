"""TD3 on the learner path (Fujimoto, van Hoof, Meger 2018): twin critics, target-policy smoothing, a delayed actor.

The reference carries TD3's hyper-parameter (`noise_trg = 0.2f0`, input.jl:231; `σ_trg` of GNoise, input.jl:201) and keys its wait
tables by "TD3", but has no algorithm file; the definition is the one of include/shems_hip.h (shems_td3_update), in the conventions of
replay() (DDPG.jl:121-145): Float32 arithmetic, Flux 0.12.1 ADAM, the minibatch of sample_indices(seed, tick).

    TD3Agent(Agent)        the DDPG learner plus a second critic (critic2, critic2_t, m_critic2, v_critic2, grad_critic2, losses2);
                           replay() is one TD3 update: update u (0-based) is a policy step when is_policy_step(u, policy_delay)
    TD3LearnerGroup(LearnerGroup)   `count` independent TD3 learners in the same launches (shems_td3_group_update_tp, throughput form): a second
                           critic per learner behind the ring of every slab; replay() follows the same schedule in lockstep
    is_policy_step(u, d)   the schedule
    parse_algo(value)      SHEMS_ALGO of the entry script

act, act_step, episode_, run_episodes, populate_memory, min_max_buffer and clone are the Agent's.  What TD3 does not cover is refused by
name (NotImplementedError), never run as DDPG: the "td3" rows of ddpg.REFUSALS; for a TD3LearnerGroup see its docstring.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _capi
from . import ddpg as D
from . import group as G

SIGMA_TRG, CLIP_TRG, POLICY_DELAY = 0.2, 0.5, 2        # input.jl:231; the paper's clip and delay
CRITIC2_SEED_OFFSET = 1000
BP = G.MAX_GROUP_BATCH                                 # 128 columns of one update pass (csrc/shems_ddpg.hip); the groups' walk tests it


class Td3Args(C.Structure):            # shems_td3
    _fields_ = [("d", D.DdpgArgs)] + \
               [(n, C.c_void_p) for n in ("critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2", "ws2", "losses2")] + \
               [("sigma_trg", C.c_float), ("clip_trg", C.c_float)]


def is_policy_step(updates, d):
    """Update number `updates` (0-based, the learner's counter BEFORE the update) moves the actor and the targets when
    (updates + 1) % d == 0: with d = 2 the updates 1, 3, 5, ..."""
    d = int(d)
    if d < 1:
        raise ValueError(f"policy_delay = {d}: the actor moves every 1 or more updates")
    return (int(updates) + 1) % d == 0


def parse_algo(value):
    """SHEMS_ALGO -> ("ddpg", None) when unset or "ddpg", ("td3", dict(policy_delay, sigma_trg, clip_trg)) for
    td3[:d[:sigma_trg[:clip_trg]]].  Anything else is refused by name."""
    if value is None or value == "ddpg":
        return "ddpg", None
    parts = str(value).split(":")
    if parts[0] != "td3" or len(parts) > 4:
        raise ValueError(f"SHEMS_ALGO = {value!r} is not ddpg or td3[:d[:sigma_trg[:clip_trg]]]")
    out = dict(policy_delay=POLICY_DELAY, sigma_trg=SIGMA_TRG, clip_trg=CLIP_TRG)
    try:
        if len(parts) > 1:
            out["policy_delay"] = int(parts[1])
        for key, raw in zip(("sigma_trg", "clip_trg"), parts[2:]):
            out[key] = float(raw)
    except ValueError:
        raise ValueError(f"SHEMS_ALGO = {value!r}: d is an integer, sigma_trg and clip_trg are numbers") from None
    if out["policy_delay"] < 1:
        raise ValueError(f"SHEMS_ALGO = {value!r}: the actor moves every d >= 1 updates")
    for key in ("sigma_trg", "clip_trg"):
        if not (math.isfinite(out[key]) and out[key] >= 0.0):
            raise ValueError(f"SHEMS_ALGO = {value!r}: {key} must be finite and >= 0")
    return "td3", out


def case_suffix(policy_delay, sigma_trg, clip_trg):
    """What the entry script appends to its `case` string, so that no file of a TD3 run collides with a DDPG run's."""
    return f"_td3-d{int(policy_delay)}-s{float(sigma_trg):g}-c{float(clip_trg):g}"


def _declare():
    L = D._declare()
    if getattr(L, "_td3_declared", False):
        return L
    dbl = C.c_double
    L.shems_td3_workspace_floats.argtypes = [C.POINTER(C.c_int64)]
    L.shems_td3_workspace_floats.restype = C.c_int
    L.shems_td3_update.argtypes = [C.POINTER(Td3Args), C.POINTER(_capi.Replay), C.c_int64, C.c_uint64, C.c_uint32, dbl, dbl, dbl, dbl, dbl, dbl,
                                   C.c_int, C.c_void_p]
    L.shems_td3_update.restype = C.c_int
    L._td3_declared = True
    return L


GROUP_WS2_PUB = 31112                                  # SHEMS_TD3_GROUP_WS2_PUB: a~' [2][128] | y | q'1 | q'2 inside a group learner's ws2
CRITIC2_BLOCKS = ("critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2")


def group_extra_blocks(n_critic, tiled, ws2_floats):
    """The blocks a TD3 learner group appends to every learner's slab, behind ring_done (group.slab_layout(extra=...)).  Host only."""
    return tuple((n, int(n_critic)) for n in CRITIC2_BLOCKS) + (("w2t_critic2", G.W2T_FLOATS if tiled else 0), ("ws2", int(ws2_floats)),
                                                                 ("losses2", 1))


_GROUP_WORDS = dict(name="TD3 learner group", head="twin-critic update", update="twin-critic update", entry="shems_td3_group_update_tp",
                    mem_size="", batch=f"the twin-critic update holds one {BP}-column pass")


def group_refusals(form=None, noise_type="gn", hparams=None, hidden=None, sigma_trg=SIGMA_TRG, clip_trg=CLIP_TRG, policy_delay=POLICY_DELAY):
    """What TD3LearnerGroup refuses before any device work, each by name."""
    G.variant_group_refusals(_GROUP_WORDS, form, noise_type, hparams, hidden)
    if not (math.isfinite(float(sigma_trg)) and float(sigma_trg) >= 0.0 and math.isfinite(float(clip_trg)) and float(clip_trg) >= 0.0):
        raise ValueError(f"TD3 learner group: sigma_trg = {sigma_trg}, clip_trg = {clip_trg} must be finite and >= 0")
    is_policy_step(0, policy_delay)                          # (refuses d < 1)


def _declare_group():
    L = G._declare_group()
    _declare()
    if getattr(L, "_td3_group_declared", False):
        return L
    dbl, vp = C.c_double, C.c_void_p
    L.shems_td3_group_workspace_floats.argtypes = [C.POINTER(C.c_int64)]
    L.shems_td3_group_workspace_floats.restype = C.c_int
    L.shems_td3_group_update_tp.argtypes = [C.POINTER(Td3Args), C.POINTER(_capi.Replay), C.POINTER(G.Group), C.POINTER(G.GroupW2T), vp, vp, vp,
                                            C.c_int64, C.c_uint64, C.c_uint32, dbl, dbl, dbl, dbl, dbl, dbl, C.c_int, C.c_int32, vp]
    L.shems_td3_group_update_tp.restype = C.c_int
    L._td3_group_declared = True
    return L


class TD3LearnerGroup(G.LearnerGroup):
    """`count` independent TD3 learners advanced by the same launches (shems_td3_group_update_tp): a LearnerGroup whose slabs also hold a
    second critic per learner (critic2, critic2_t, m_critic2, v_critic2, grad_critic2, w2t_critic2 on the tiled layout, ws2, losses2 --
    carved behind the ring, so every offset of a DDPG group is unchanged).  Learner l's critic 2 is initialised from seed + l +
    critic2_seed_offset, as TD3Agent initialises its own.  sigma_trg, clip_trg and policy_delay are the group's; the schedule runs in
    lockstep.  Throughput form only, whatever the count.  act_step, populate_memory, min_max_buffer, ring_window, episode_, eval_scores,
    run_episodes, clone and imitation.dagger_group are the LearnerGroup's (they read or train the actor only).  Refused by name
    (NotImplementedError): form 'latency' / 'wide', "ou" noise and per-learner mem_size (the *_x entry points), batch > 128, wide hidden
    sizes, evaluate() and with it imitation.warm_start_group."""

    has_evaluate = False

    def __init__(self, count, envs_per_learner, sigma_trg=SIGMA_TRG, clip_trg=CLIP_TRG, policy_delay=POLICY_DELAY,
                 critic2_seed_offset=CRITIC2_SEED_OFFSET, **kw):
        if kw.get("hparams") is not None:
            kw["hparams"] = list(kw["hparams"])              # (a generator is walked once, here)
        group_refusals(kw.get("form"), kw.get("noise_type", "gn"), kw.get("hparams"), kw.get("hidden"), sigma_trg, clip_trg, policy_delay)
        kw["form"] = "throughput"
        self.sigma_trg, self.clip_trg, self.policy_delay = float(sigma_trg), float(clip_trg), int(policy_delay)
        self.critic2_seed_offset = int(critic2_seed_offset)
        super().__init__(count, envs_per_learner, **kw)
        self.L = _declare_group()
        t = self.torch
        for l, ag in enumerate(self.learners):
            c2 = D.pad_net(D.init_params(ag.seed + self.critic2_seed_offset, D.STATE + D.ACTION, 1, 1, ag.hidden), D.STATE + D.ACTION, 1, ag.hidden)
            self.critic2_of(l).copy_(t.from_numpy(c2))
            self.critic2_t_of(l).copy_(self.critic2_of(l))
        self._tiled_valid = False                            # (critic 2's Flux-order blocks were just written)

    def _extra_blocks(self, n_critic):
        nws = C.c_int64(0)
        _capi.check(_declare_group().shems_td3_group_workspace_floats(C.byref(nws)))
        return group_extra_blocks(n_critic, self.tiled, nws.value)

    def _pbt_blocks(self):
        """What a child of a population-based-training round inherits of the second critic: parameters, target, ADAM moments and, on the
        tiled layout, its tiled region -- not grad_critic2, ws2 or losses2."""
        return ("critic2", "critic2_t", "m_critic2", "v_critic2", "w2t_critic2")

    # ---- views ----
    def _view(self, l, name):
        o, n = self.layout[name]
        return self.slab[l, o:o + n]

    def critic2_of(self, l):
        """Learner l's critic 2 in Flux order (on a tiled group: current after flux_())."""
        return self._view(l, "critic2")

    def critic2_t_of(self, l):
        return self._view(l, "critic2_t")

    def a_smooth(self, l):
        """a~' = clamp(actor_t(s') + eps, -1, 1) of learner l's last update, [2][128] (columns >= batch_l are padding)."""
        return self._view(l, "ws2")[GROUP_WS2_PUB:GROUP_WS2_PUB + 2 * BP].view(2, BP)

    def y_target(self, l):
        return self._view(l, "ws2")[GROUP_WS2_PUB + 2 * BP:GROUP_WS2_PUB + 3 * BP]

    def q_target1(self, l):
        return self._view(l, "ws2")[GROUP_WS2_PUB + 3 * BP:GROUP_WS2_PUB + 4 * BP]

    def q_target2(self, l):
        return self._view(l, "ws2")[GROUP_WS2_PUB + 4 * BP:GROUP_WS2_PUB + 5 * BP]

    @property
    def losses2(self):
        """[count] the mse of every learner's critic 2 at its last update."""
        o = self.layout["losses2"][0]
        return self.slab[:, o]

    # ---- the tiled layout covers critic 2: the layout launches again, on the record whose critic fields name critic 2's blocks ----
    def _td3_args(self):
        """Learner 0's shems_td3: its shems_ddpg and the critic-2 blocks of its slab."""
        a0 = self.learners[0]
        p = lambda name: self.slab.data_ptr() + 4 * self.layout[name][0]
        return Td3Args(a0._ddpg_args(), p("critic2"), p("critic2_t"), p("m_critic2"), p("v_critic2"), p("grad_critic2"), p("ws2"), p("losses2"),
                       self.sigma_trg, self.clip_trg)

    def _critic2_alias(self):
        """(shems_ddpg, shems_group_w2t) that name critic 2 where critic 1 stands: what shems_group_w2_to_tiled / _to_flux take for it."""
        t3, w = self._td3_args(), self.w2t_struct()
        d = t3.d
        d.critic, d.critic_t, d.m_critic, d.v_critic, d.grad_critic = t3.critic2, t3.critic2_t, t3.m_critic2, t3.v_critic2, t3.grad_critic2
        return d, G.GroupW2T(w.actor, self.slab.data_ptr() + 4 * self.layout["w2t_critic2"][0])

    def _use_tiled(self):
        was = self._tiled_valid
        on = super()._use_tiled()
        if on and not was:
            d, w = self._critic2_alias()
            g = self.struct()
            _capi.check(self.L.shems_group_w2_to_tiled(C.byref(d), C.byref(g), C.byref(w), self._stream()))
        return on

    def flux_(self):
        stale = self.tiled and not self._flux_valid
        super().flux_()
        if stale:
            d, w = self._critic2_alias()
            g = self.struct()
            _capi.check(self.L.shems_group_w2_to_flux(C.byref(d), C.byref(g), C.byref(w), self._stream()))
        return self

    def set_params(self, l, actor=None, critic=None, sync_targets=True, critic2=None):
        """learners[l].set_params, and critic2: a flat Flux-layout vector of learner l's critic size (padded here) or of the (250, 500)
        layout, as TD3Agent.set_params takes it."""
        ag = self.learners[l]
        ag.set_params(actor=actor, critic=critic, sync_targets=sync_targets)
        if critic2 is not None:
            v = np.asarray(critic2, D.f32)
            n_own = D.net_size(D.STATE + D.ACTION, 1, ag.hidden)
            if v.size not in (ag.n_critic, n_own):
                raise ValueError(f"set_params: critic2 has {v.size} parameters; a {ag.hidden} network holds {n_own}")
            if v.size != ag.n_critic:
                v = D.pad_net(v, D.STATE + D.ACTION, 1, ag.hidden)
            self._before_flux_write()
            self.critic2_of(l).copy_(self.torch.as_tensor(v))
            if sync_targets:
                self.critic2_t_of(l).copy_(self.critic2_of(l))

    # ---- refused paths ----
    def evaluate(self, rings=None, tick=None, tau=None):
        raise NotImplementedError("TD3 learner group: evaluate() is the critic-only update of ONE critic; the twin critics have none "
                                  "(and so imitation.warm_start_group does not run on a TD3 group)")

    def _hold_ptr(self):
        if self._hp_dev is None:
            return None
        return self._hp_variant(0.0, check=False)

    def replay(self, tick=None, update_policy=None):
        """One TD3 update of every learner (shems_td3_group_update_tp: seven launches, ten on a policy step).  update_policy: None = the
        schedule, is_policy_step(self.updates, self.policy_delay).  bp_critic advances on every update, bp_actor on policy steps, both
        in lockstep over the learners; `updates` counts updates.  On a tiled group the Flux-order view goes stale, critic 2 included."""
        if self.form != "throughput":
            raise NotImplementedError(f"TD3 learner group: form={self.form!r} has no twin-critic update")
        policy = is_policy_step(self.updates, self.policy_delay) if update_policy is None else bool(update_policy)
        a0, g, r0 = self.learners[0], self.struct(), self._ring0()
        if self._hp_dev is None and a0.batch > BP:
            raise NotImplementedError(f"TD3 learner group: batch {a0.batch} > {BP}: the twin-critic update holds one {BP}-column pass")
        tl = self._use_tiled()
        t3 = self._td3_args()
        w = C.byref(self.w2t_struct()) if tl else None
        w2 = C.c_void_p(self.slab.data_ptr() + 4 * self.layout["w2t_critic2"][0]) if tl else None
        _capi.check(self.L.shems_td3_group_update_tp(C.byref(t3), C.byref(r0), C.byref(g), w, w2, self._hp_ptr(), self._hold_ptr(),
                                                     len(self.rings[0]), self.rng_seed, D.tick32(tick, self.updates), *a0._adam_c, *a0._adam_a,
                                                     1 if policy else 0, 1 if self.store_grad else 0, self._stream()))
        if tl:
            self._flux_valid = False
        self._advance_learners(critic=True, actor=policy, counter="updates")
        self.updates += 1


class TD3Agent(D.Agent):
    """The TD3 learner state on one GPU: an Agent and a second critic."""

    _CRITIC2_TENSORS = ("critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2", "losses2")
    _LEARNER_TENSORS = D.Agent._LEARNER_TENSORS + _CRITIC2_TENSORS

    def __init__(self, seed=1231, sigma_trg=SIGMA_TRG, clip_trg=CLIP_TRG, policy_delay=POLICY_DELAY, critic2_seed=None, **kw):
        hidden = tuple(int(h) for h in kw.get("hidden", (D.L1, D.L2)))
        D.refuse("td3.init", dict(wide=kw.get("wide") or D.is_wide(hidden), hidden=hidden, pn=kw.get("noise_type", "gn") == "pn",
                                  slab=kw.get("tensors") is not None))
        if not (math.isfinite(float(sigma_trg)) and float(sigma_trg) >= 0.0 and math.isfinite(float(clip_trg)) and float(clip_trg) >= 0.0):
            raise ValueError(f"TD3: sigma_trg = {sigma_trg}, clip_trg = {clip_trg} must be finite and >= 0")
        is_policy_step(0, policy_delay)                      # (refuses d < 1)
        super().__init__(seed=seed, **kw)
        self.L = _declare()
        self.sigma_trg, self.clip_trg, self.policy_delay = float(sigma_trg), float(clip_trg), int(policy_delay)
        self.critic2_seed = self.seed + CRITIC2_SEED_OFFSET if critic2_seed is None else int(critic2_seed)
        t = self.torch
        z = lambda n: t.zeros(n, dtype=t.float32, device=self.device)
        n = self.n_critic
        self.critic2, self.critic2_t, self.m_critic2, self.v_critic2, self.grad_critic2 = z(n), z(n), z(n), z(n), z(n)
        self.losses2 = z(1)
        nws = C.c_int64(0)
        _capi.check(self.L.shems_td3_workspace_floats(C.byref(nws)))
        self.ws2 = z(nws.value)
        c2 = D.pad_net(D.init_params(self.critic2_seed, D.STATE + D.ACTION, 1, 1, self.hidden), D.STATE + D.ACTION, 1, self.hidden)
        self.critic2.copy_(t.from_numpy(c2))
        self.critic2_t.copy_(self.critic2)

    # ---- what the last update published (views of ws2; columns >= batch are padding) ----
    @property
    def a_smooth(self):
        """a~' = clamp(actor_t(s') + eps, -1, 1), [2][128] (output-major, as every array of the update)."""
        return self.ws2[0:2 * BP].view(2, BP)

    @property
    def y_target(self):
        """y = r + gamma (1 - done) min(q'1, q'2), [128]."""
        return self.ws2[2 * BP:3 * BP]

    @property
    def q_target1(self):
        """q'1 = critic_t([s'; a~']), [128]."""
        return self.ws2[3 * BP:4 * BP]

    @property
    def q_target2(self):
        """q'2 = critic2_t([s'; a~']), [128]."""
        return self.ws2[4 * BP:5 * BP]

    # ---- refused paths ----
    def use_tiled(self, on=True):
        if on:
            raise NotImplementedError(D.TD3_NEVER["use_tiled"])
        return super().use_tiled(False)

    def evaluate(self, ring, tick=None, tau=None):
        raise NotImplementedError(D.TD3_NEVER["evaluate"])

    def enable_data_parallel(self, dist, native=None):
        raise NotImplementedError(D.TD3_NEVER["enable_data_parallel"])

    def set_params(self, actor=None, critic=None, sync_targets=True, critic2=None):
        """As Agent.set_params, and critic2: a flat Flux-layout vector of this learner's critic size (padded here) or of the (250, 500)
        layout."""
        super().set_params(actor=actor, critic=critic, sync_targets=sync_targets)
        if critic2 is not None:
            v = np.asarray(critic2, D.f32)
            n_own = D.net_size(D.STATE + D.ACTION, 1, self.hidden)
            if v.size not in (self.n_critic, n_own):
                raise ValueError(f"set_params: critic2 has {v.size} parameters; a {self.hidden} network holds {n_own}")
            if v.size != self.n_critic:
                v = D.pad_net(v, D.STATE + D.ACTION, 1, self.hidden)
            self.critic2.copy_(self.torch.as_tensor(v))
            if sync_targets:
                self.critic2_t.copy_(self.critic2)

    def _td3_args(self):
        p = lambda x: x.data_ptr()
        return Td3Args(self._ddpg_args(), p(self.critic2), p(self.critic2_t), p(self.m_critic2), p(self.v_critic2), p(self.grad_critic2),
                       p(self.ws2), p(self.losses2), self.sigma_trg, self.clip_trg)

    def replay_given(self, ring, idx, weights):
        raise NotImplementedError(D.TD3_NEVER["replay_given"])

    def replay(self, ring, tick=None, exclude=None, publish=None, update_policy=None):
        """One TD3 update from `ring` (shems_td3_update).  update_policy: None = the schedule, is_policy_step(self.updates,
        self.policy_delay).  bp_critic advances on every update, bp_actor on policy steps; `updates` counts updates.  With `bc` set
        (ddpg.BC) the policy step's actor loss is the behaviour-regularised one (shems_td3_update_bc)."""
        D.refuse("td3", self._facts(ring, exclude, publish))
        self._same_device(None, ring)
        policy = is_policy_step(self.updates, self.policy_delay) if update_policy is None else bool(update_policy)
        a, rs = self._td3_args(), ring.struct()
        if self.bc is not None:
            # the policy step's actor loss is the behaviour-regularised one (shems_td3_update_bc); off a policy step nothing of it runs
            b = self.bc.struct(self.bc_out.data_ptr())
            _capi.check(_capi.declare_bc().shems_td3_update_bc(C.byref(a), C.byref(rs), *self._sample(ring, tick), *self._adam_c, *self._adam_a,
                                                               1 if policy else 0, C.byref(b), self._stream()))
        else:
            _capi.check(self.L.shems_td3_update(C.byref(a), C.byref(rs), *self._sample(ring, tick), *self._adam_c, *self._adam_a,
                                                1 if policy else 0, self._stream()))
        self._advance(critic=True, actor=policy, counter="updates")

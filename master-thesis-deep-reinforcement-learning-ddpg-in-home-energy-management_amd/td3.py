"""TD3 on the learner path (Fujimoto, van Hoof, Meger 2018): twin critics, target-policy smoothing, a delayed actor.

The reference carries TD3's hyper-parameter (`noise_trg = 0.2f0`, input.jl:231; `σ_trg` of GNoise, input.jl:201) and keys its wait
tables by "TD3", but has no algorithm file; the definition is the one of include/shems_hip.h (shems_td3_update), in the conventions of
replay() (DDPG.jl:121-145): Float32 arithmetic, Flux 0.12.1 ADAM, the minibatch of sample_indices(seed, tick).

    TD3Agent(Agent)        the DDPG learner plus a second critic (critic2, critic2_t, m_critic2, v_critic2, grad_critic2, losses2);
                           replay() is one TD3 update: update u (0-based) is a policy step when is_policy_step(u, policy_delay)
    is_policy_step(u, d)   the schedule
    parse_algo(value)      SHEMS_ALGO of the entry script

act, act_step, episode_, run_episodes, populate_memory, min_max_buffer and clone are the Agent's.  What TD3 does not cover is refused by
name (NotImplementedError), never run as DDPG: networks wider than (250, 500), batches above 128, parameter noise, data-parallel
replicas, the tiled working layout, evaluate(), learners of a learner group, the pipelined forms of replay() (exclude / publish).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _capi
from . import ddpg as D

SIGMA_TRG, CLIP_TRG, POLICY_DELAY = 0.2, 0.5, 2        # input.jl:231; the paper's clip and delay
CRITIC2_SEED_OFFSET = 1000
BP = 128                                               # columns of one update pass (csrc/shems_ddpg.hip)


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


class TD3Agent(D.Agent):
    """The TD3 learner state on one GPU: an Agent and a second critic."""

    _CRITIC2_TENSORS = ("critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2", "losses2")
    _LEARNER_TENSORS = D.Agent._LEARNER_TENSORS + _CRITIC2_TENSORS

    def __init__(self, seed=1231, sigma_trg=SIGMA_TRG, clip_trg=CLIP_TRG, policy_delay=POLICY_DELAY, critic2_seed=None, **kw):
        hidden = tuple(int(h) for h in kw.get("hidden", (D.L1, D.L2)))
        if kw.get("wide") or D.is_wide(hidden):
            raise NotImplementedError(f"TD3: hidden sizes {hidden} run layer by layer (shems_wide_*), which has no twin-critic update")
        if kw.get("noise_type", "gn") == "pn":
            raise NotImplementedError("TD3: parameter noise (noise_type = 'pn') adapts between getData and the updates of replay(); "
                                      "the TD3 update is one call")
        if kw.get("tensors") is not None:
            raise NotImplementedError("TD3: a learner of a learner group keeps its state in the group's slab, which holds no second critic")
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
            raise NotImplementedError("TD3: the tiled working layout (use_tiled) holds the actor's and critic 1's layer-2 state only")
        return super().use_tiled(False)

    def evaluate(self, ring, tick=None, tau=None):
        raise NotImplementedError("TD3: evaluate() is the critic-only update of ONE critic; the twin critics have none")

    def enable_data_parallel(self, dist, native=None):
        raise NotImplementedError("TD3: data-parallel replicas do not exchange the second critic's gradient")

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

    def replay(self, ring, tick=None, exclude=None, publish=None, update_policy=None):
        """One TD3 update from `ring` (shems_td3_update).  update_policy: None = the schedule, is_policy_step(self.updates,
        self.policy_delay).  bp_critic advances on every update, bp_actor on policy steps; `updates` counts updates."""
        if exclude is not None or publish is not None:
            raise NotImplementedError("TD3: the pipelined forms of replay() (exclude / publish) belong to shems_ddpg_update")
        if self.batch > self.MAX_PASS_BATCH:
            raise NotImplementedError(f"TD3: BATCH_SIZE = {self.batch}; the twin-critic update holds at most {self.MAX_PASS_BATCH} columns")
        if self.noise_type == "pn":
            raise NotImplementedError("TD3: parameter noise (noise_type = 'pn')")
        if self.sync.world > 1:
            raise NotImplementedError("TD3: data-parallel replicas do not exchange the second critic's gradient")
        if self.tiled_mode or self._tiled_current:
            raise NotImplementedError("TD3: the tiled working layout (use_tiled)")
        if getattr(self, "_before_param_write", None) is not None:
            raise NotImplementedError("TD3: a learner of a learner group keeps its own working layout")
        self._same_device(None, ring)
        policy = is_policy_step(self.updates, self.policy_delay) if update_policy is None else bool(update_policy)
        a = self._td3_args()
        rs = ring.struct()
        tick = self.updates if tick is None else tick
        _capi.check(self.L.shems_td3_update(C.byref(a), C.byref(rs), len(ring), self.rng_seed, int(tick) & 0xFFFFFFFF, self.eta_crit,
                                            self.bp_critic[0], self.bp_critic[1], self.eta_act, self.bp_actor[0], self.bp_actor[1],
                                            1 if policy else 0, self._stream()))
        self.bp_critic = [self.bp_critic[0] * 0.9, self.bp_critic[1] * 0.999]
        if policy:
            self.bp_actor = [self.bp_actor[0] * 0.9, self.bp_actor[1] * 0.999]
        self.updates += 1

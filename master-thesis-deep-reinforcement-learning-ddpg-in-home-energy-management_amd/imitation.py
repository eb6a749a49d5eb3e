"""The actor trained by imitation of the foresight controller (this build's addition; the reference has no supervised step).

The foresight controller (foresight.py) knows the future rows; the DDPG actor sees nine numbers.  How much of the foresight return
can such an actor hold at all?  Three pieces answer it, all on the GPU:

  * demonstrations: the 23-column rows of a tracked pass plus one label per hour become (observation, action) pairs in a ring
    (shems_foresight_demos_dev, one launch; the definition: fs_demo_hour in csrc/shems_foresight_core.h).  The label is either the
    targets the foresight pass itself chose (from_foresight) or, for a pass of ANY controller, the best action of the audit at the
    states that pass actually visited (from_pass) -- the DAgger label;
  * the supervised update: ddpg.Agent.clone, loss = Flux.mse(actor(normalize(s)), a_demo) (shems_ddpg_clone_update, three launches);
  * dagger: round 0 clones the foresight pass, every later round runs the current actor, labels the states it visited and trains on.

A cloned actor with a freshly initialised critic forgets what cloning taught it: the first actor gradients of DDPG come from a critic
that knows nothing.  Three more pieces join the two (the definition: fs_transition_hour and fs_returns in the same header):

  * transitions: the rows of a DRL-mode pass become full replay slots (s, a, r, s', done) (shems_foresight_transitions_dev), either
    as the reference's `remember` would store them ("td") or with the discounted return-to-go of the pass as the reward and done = 1
    ("mc"): env and tracked policy are deterministic, so that return is the exact Q of the controller that made the pass, and a
    critic can be regressed on it without bootstrapping from itself;
  * the critic-only update: ddpg.Agent.evaluate (shems_ddpg_critic_update, three launches, the actor is left alone);
  * warm_start: dagger, one pass of the resulting actor, its transitions, and a number of critic-only updates on them.

The same for a learner group (group.LearnerGroup.clone / evaluate: every learner's update in four / five launches): GroupDemos and
GroupRings hold one ring per learner in one allocation with a constant stride, dagger_group and warm_start_group run the rounds for
all learners at once (one tracking launch and one audit per round; the passes go into the rings learner by learner).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, foresight
from .replay import ReplayRing


class Demos(ReplayRing):
    """A ring of demonstrations, shaped like the replay ring (ddpg.Agent.clone and min_max_buffer take it): zero-allocated, only s
    and a are ever written (r, s2 and done stay zero and are never read), and its length grows with what was written -- `pushed`
    counts the pairs, the next one goes to slot `pos`."""

    def __init__(self, capacity, device=None, tensors=None):
        super().__init__(capacity, device=device, tensors=tensors)


def ring_slab_floats(capacity):
    """(offsets, floats) of one learner's ring arrays inside a GroupDemos / GroupRings allocation: s [capacity][9], a [capacity][2],
    r [capacity], s2 [capacity][9], done [capacity] bytes, every array on a 16-byte boundary.  Host arithmetic only."""
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError(f"a ring needs capacity >= 1, not {capacity}")
    offs, off = {}, 0
    for name, n in (("s", capacity * _capi.NSTATE), ("a", capacity * _capi.NACTION), ("r", capacity), ("s2", capacity * _capi.NSTATE),
                    ("done", (capacity + 3) // 4)):
        offs[name] = (off, n)
        off = (off + n + 3) & ~3
    return offs, off


class GroupRings:
    """`count` replay rings of `capacity` slots as views of ONE allocation with a constant stride: ring l's arrays are ring 0's plus
    l * stride_bytes, which is what LearnerGroup.evaluate hands to shems_ddpg_group_critic_update_tp (rings[l], struct0(),
    stride_bytes).  rings[l] is an ordinary ReplayRing: imitation.transitions fills it, Agent.evaluate takes it.  Such a ring lives
    outside the learners' slabs: an "mc" ring of returns (done = 1 in every slot) must never be the ring bootstrapped training samples,
    so it is never the group's own."""
    ring_class = ReplayRing

    def __init__(self, count, capacity, device=None):
        import torch
        self.count, self.capacity = int(count), int(capacity)
        if self.count < 1:
            raise ValueError(f"a ring group needs count >= 1, not {count}")
        self.layout, self.floats = ring_slab_floats(self.capacity)
        self.stride_bytes = 4 * self.floats
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.slab = torch.zeros((self.count, self.floats), dtype=torch.float32, device=self.device)
        self.rings = []
        for l in range(self.count):
            v = lambda name: self.slab[l, self.layout[name][0]:self.layout[name][0] + self.layout[name][1]]
            tens = (v("s").view(self.capacity, _capi.NSTATE), v("a").view(self.capacity, _capi.NACTION), v("r"),
                    v("s2").view(self.capacity, _capi.NSTATE), v("done").view(torch.uint8)[:self.capacity])
            self.rings.append(self.ring_class(self.capacity, tensors=tens))

    def struct0(self):
        return self.rings[0].struct()

    def __len__(self):
        return self.count


class GroupDemos(GroupRings):
    """`count` Demos rings in one allocation (GroupRings' layout): learner l's demonstrations for LearnerGroup.clone.  Every imitation
    function that takes a Demos takes rings[l]."""
    ring_class = Demos


def _declare(L):
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.shems_foresight_demos_dev.argtypes = [vp, i64, vp, i32, C.POINTER(foresight.GridStruct), i32, vp, i32, vp, vp, vp,
                                            C.POINTER(_capi.Replay), i64, vp, vp]
    L.shems_foresight_demos_dev.restype = C.c_int
    L.shems_foresight_transitions_dev.argtypes = [vp, i64, vp, i32, i32, vp, i32, vp, i32, C.c_float, i32, vp, C.POINTER(_capi.Replay), i64,
                                                  vp, vp]
    L.shems_foresight_transitions_dev.restype = C.c_int
    return L


def _check_values(values, what):
    if isinstance(values, foresight.EnsembleValues):
        raise ValueError(f"{what}: the values were solved on a forecast ensemble (pass the Values of a solve on the true rows)")
    return values


def _write(values, results, problem_of_pass, demos, targets=None, best_action=None):
    """The demos call for n passes [n][T][23] with one label source (host arrays): one launch on PyTorch's current stream, one copy
    back of the status words.  Raises BoundsError naming the first refused pass and leaves the length alone; otherwise the length
    grows by n * T."""
    import torch
    res = np.ascontiguousarray(results, np.float64)
    n, T = int(res.shape[0]), values.nsteps
    if res.ndim != 3 or res.shape[1] != T or res.shape[2] != _capi.NRESULT:
        raise ValueError(f"results must be [n][{T}][{_capi.NRESULT}], not {tuple(res.shape)}")
    L = _declare(_capi.lib())
    dev = demos.s.device
    env = values._tables if hasattr(values._tables, "use_torch_stream") else None        # a ShemsBatch, or the uploaded tensor
    if env is not None:
        env.use_torch_stream()
        tab_ptr = env.view().tables
    else:
        tab_ptr = values._tables.data_ptr()
    d_res = torch.from_numpy(res).to(dev)
    d_po = torch.from_numpy(np.ascontiguousarray(problem_of_pass, np.int32)).to(dev) if problem_of_pass is not None else None
    d_tgt = torch.from_numpy(np.ascontiguousarray(targets, np.float32).reshape(n, T, 2)).to(dev) if targets is not None else None
    d_act = torch.from_numpy(np.ascontiguousarray(best_action, np.int32).reshape(n, T)).to(dev) if best_action is not None else None
    status = torch.empty(n, dtype=torch.int32, device=dev)
    g = values.grid.struct()
    rs = demos.struct()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _capi.check(L.shems_foresight_demos_dev(C.c_void_p(tab_ptr), int(values.total_rows), C.c_void_p(values.d_problems.data_ptr()),
                                            values.n_problems, C.byref(g), T, ptr(d_res), n, ptr(d_po), ptr(d_tgt), ptr(d_act), C.byref(rs),
                                            demos.pos, ptr(status), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    st = status.cpu().numpy()                                # the call's one synchronisation
    bad = np.nonzero(st)[0]
    if bad.size:
        e = int(bad[0])
        raise _capi.BoundsError(int(st[e]), f"imitation: pass {e}: a row does not sit on its problem's table rows, it names none of the "
                                f"{values.n_problems} problems, or an hour has no label (best_action -1); the ring's length is unchanged")
    demos.pushed += n * T


def from_foresight(env, values, demos, problem_of_env=None, which=-1):
    """The foresight controller's own pass as demonstrations: foresight.track from the envs' CURRENT state (reset them onto their
    problem's start row first), then every (env, hour) -- or those of env `which` alone -- goes into `demos` with the targets that
    pass chose.  `values`: whatever foresight.track takes (a forecast controller's targets are labels like any other).  Returns what
    foresight.track returns (totals, results, targets)."""
    ens = values if isinstance(values, foresight.EnsembleValues) else None
    inner = ens.values if ens is not None else values
    total, results, targets = foresight.track(env, values, problem_of_env, which=which)
    po = None if problem_of_env is None else np.asarray(problem_of_env, np.int32).reshape(env.n)
    if ens is not None and po is not None:
        po = po * ens.n_scen                                 # the first record of the problem: every scenario shares its truth
    if which >= 0:
        targets = targets[which:which + 1]
        po = None if po is None else po[which:which + 1]
    _write(inner, results, po, demos, targets=targets)
    return total, results, targets


def from_pass(values, results, demos, problem_of_pass=None):
    """The DAgger labels of passes of ANY controller: foresight.audit of the rows ([n][T][23] or [T][23]) against `values`, then every
    (pass, hour) goes into `demos` with the audit's best action at the state the pass was in.  Values solved on a forecast, and
    EnsembleValues, are refused as audit refuses them.  Returns the Audit."""
    _check_values(values, "from_pass")
    audit = foresight.audit(values, results, problem_of_pass)
    res = np.asarray(results, np.float64)
    _write(values, res[None] if res.ndim == 2 else res, problem_of_pass, demos, best_action=audit.best_action)
    return audit


def dagger(agent, env, values, demos, rounds, steps_per_round, tau=1.0):
    """Dataset aggregation on one data set: every pass starts from reset!(rng = -1) and runs values.nsteps hours; `values` is the
    perfect-foresight solve of env's table from row 1 (harness.foresight_values(env)).
      round 0          the foresight controller's pass (env 0's) goes into `demos`, the normalisation is set from it
                       (agent.min_max_buffer) and `steps_per_round` clone steps follow: plain behaviour cloning;
      round r >= 1     the CURRENT actor's pass (harness.inference), labelled by the audit at the states it visited (from_pass),
                       is appended, and `steps_per_round` clone steps follow on everything gathered so far.
    All device work goes on PyTorch's current stream.  Returns one dict per round: "return" (round 0: the foresight pass's, later:
    the return of the actor that round started with), "loss" (losses[1] after the round's last step) and "demos" (the ring's length)."""
    from . import harness
    rounds, steps = int(rounds), int(steps_per_round)
    if rounds < 1 or steps < 1:
        raise ValueError(f"dagger: {rounds} rounds x {steps} steps; at least one of each")
    _check_values(values, "dagger")
    out = []
    for r in range(rounds):
        if r == 0:
            env.use_torch_stream()
            env.reset_(-1)
            _, _, poe = foresight.problems_of_env(env, np.ones(env.n, np.int64))
            total, _, _ = from_foresight(env, values, demos, poe, which=0)
            agent.min_max_buffer(demos)
            ret = float(total[0])
        else:
            total, res = harness.inference(env, agent, track=1, num_steps=values.nsteps)
            _, _, poe = foresight.problems_of_env(env, np.ones(env.n, np.int64))
            from_pass(values, res, demos, poe[:1] if values.n_problems > 1 else None)
            ret = float(total[0])
        for _ in range(steps):
            agent.clone(demos, tau=tau)
        out.append({"return": ret, "loss": float(agent.losses[1].item()), "demos": len(demos)})
    return out


TRANSITION_MODES = {"td": 0, "mc": 1}                        # SHEMS_FS_TRANS_TD / SHEMS_FS_TRANS_MC


def default_tail(mode, gamma, T):
    """td: 1, every hour that has a successor.  mc: the smallest k with gamma^k <= 0.01, capped at T - 1 -- the hours whose return the
    end of the pass cuts short by more than a hundredth of its weight are dropped."""
    if mode == "td":
        return 1
    k, w = 1, float(gamma)
    while w > 0.01 and k < T - 1:
        k, w = k + 1, w * float(gamma)
    return k


def transitions(values, results, ring, problem_of_pass=None, mode="td", gamma=None, tail=None):
    """Full transitions (s, a, r, s', done) of n tracked passes ([n][T][23] or [T][23] host rows) into `ring` from its push position:
    one C call on PyTorch's current stream (shems_foresight_transitions_dev), one copy back of the status words.
      mode "td"   the slot holds (s, a, float32 reward, s', 0), the bytes `remember` would store: the ring can go straight on as the
                  replay ring of episode_ / run_episodes;
      mode "mc"   the slot holds (s, a, float32 G[t], s', 1) with G the discounted return-to-go of the pass in float64
                  (G[T - 1] = r[T - 1], G[t] = r[t] + gamma G[t + 1]): the update's target is G[t] itself.  Such slots must never meet
                  bootstrapped training (done = 1 would cut every target short): keep them in a ring of their own.
    tail: hours t >= T - tail give no transition (default_tail); n * (T - tail) must fit the capacity.  gamma: ddpg.GAMMA.
    `values`: a Values or an EnsembleValues, of which only the problems and the tables are read; problem_of_pass names the problem.
    The rows must come from DRL-mode passes (an actor's, the foresight controller's): a RULE-BASED pass records no targets (columns
    21 and 2 hold 0 and kWh set-points), its actions would be wrong, and nothing checks it.
    Raises BoundsError naming the first refused pass and leaves ring.pushed alone; otherwise ring.pushed grows by n * (T - tail).
    Returns the returns [n][T] float64 in "mc" mode, None in "td" mode."""
    import torch
    from . import ddpg
    if mode not in TRANSITION_MODES:
        raise ValueError(f"transitions: mode {mode!r} is neither 'td' nor 'mc'")
    ens = values if isinstance(values, foresight.EnsembleValues) else None
    inner = ens.values if ens is not None else values
    res = np.ascontiguousarray(results, np.float64)
    if res.ndim == 2:
        res = res[None]
    T = inner.nsteps
    if res.ndim != 3 or res.shape[1] != T or res.shape[2] != _capi.NRESULT:
        raise ValueError(f"results must be [n][{T}][{_capi.NRESULT}], not {tuple(res.shape)}")
    n = int(res.shape[0])
    gamma = ddpg.GAMMA if gamma is None else float(gamma)
    tail = default_tail(mode, gamma, T) if tail is None else int(tail)
    po = None if problem_of_pass is None else np.ascontiguousarray(problem_of_pass, np.int32).reshape(n)
    if ens is not None and po is not None:
        po = po * ens.n_scen                                 # the first record of the problem: every scenario shares its truth
    L = _declare(_capi.lib())
    dev = ring.s.device
    env = inner._tables if hasattr(inner._tables, "use_torch_stream") else None          # a ShemsBatch, or the uploaded tensor
    if env is not None:
        env.use_torch_stream()
        tab_ptr = env.view().tables
    else:
        tab_ptr = inner._tables.data_ptr()
    d_res = torch.from_numpy(res).to(dev)
    d_po = torch.from_numpy(po).to(dev) if po is not None else None
    d_ret = torch.empty((n, T), dtype=torch.float64, device=dev) if mode == "mc" else None
    status = torch.empty(n, dtype=torch.int32, device=dev)
    rs = ring.struct()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _capi.check(L.shems_foresight_transitions_dev(C.c_void_p(tab_ptr), int(inner.total_rows), C.c_void_p(inner.d_problems.data_ptr()),
                                                  inner.n_problems, T, ptr(d_res), n, ptr(d_po), TRANSITION_MODES[mode], gamma, tail,
                                                  ptr(d_ret), C.byref(rs), ring.pos, ptr(status),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    st = status.cpu().numpy()                                # the call's one synchronisation
    bad = np.nonzero(st)[0]
    if bad.size:
        e = int(bad[0])
        raise _capi.BoundsError(int(st[e]), f"transitions: pass {e}: a row does not sit on its problem's table rows, a reward is not finite, or "
                                f"it names none of the {inner.n_problems} problems; the ring's length is unchanged")
    ring.pushed += n * (T - tail)
    return d_ret.cpu().numpy() if d_ret is not None else None


def _refuse_n_step(what, learner):
    """The warm start seeds ONE-step transitions and fits the critic on them: an n-step learner (Agent / LearnerGroup(n_step > 1)), whose
    every update bootstraps with gamma^n, is refused by name before anything is trained."""
    n = int(getattr(learner, "n_step", 1))
    if n > 1:
        raise NotImplementedError(f"{what}: n_step = {n}: the warm start's transitions are one-step (s, a, r, s'), which this learner's "
                                  f"updates would bootstrap with gamma^{n}; nothing was trained")


def warm_start(agent, env, values, demos, ring, rounds, steps_per_round, critic_steps, mode="mc", tau=1.0):
    """A cloned actor AND a critic that knows it: dagger(agent, env, values, demos, rounds, steps_per_round, tau) as it stands, then
    one pass of the resulting actor (harness.inference), its transitions into `ring` in `mode`, and `critic_steps` critic-only updates
    (agent.evaluate) on that ring.  The normalisation is the one dagger set from the foresight pass; agent.min_max_buffer(ring) would
    run only if dagger had not set one.  Everything goes on PyTorch's current stream.
    With mode "td" the same ring can go straight on as the agent's replay ring for episode_ / run_episodes.  With "mc" its slots carry
    done = 1 and a return as the reward: bootstrapped training must never sample them (every target would be cut to r, with r a
    return), so the caller seeds a second "td" ring (transitions(..., mode="td")) for the fine-tuning.
    Returns dagger's per-round records followed by one dict {"critic_loss_first", "critic_loss_last", "transitions"}: losses[0]
    after the first and the last critic step, and the ring's length."""
    from . import harness
    _refuse_n_step("warm_start", agent)
    critic_steps = int(critic_steps)
    if critic_steps < 1:
        raise ValueError(f"warm_start: {critic_steps} critic steps; at least one")
    if mode not in TRANSITION_MODES:
        raise ValueError(f"warm_start: mode {mode!r} is neither 'td' nor 'mc'")
    out = dagger(agent, env, values, demos, rounds, steps_per_round, tau=tau)
    _, res = harness.inference(env, agent, track=1, num_steps=values.nsteps)
    _, _, poe = foresight.problems_of_env(env, np.ones(env.n, np.int64))
    transitions(values, res, ring, poe[:1] if values.n_problems > 1 else None, mode=mode, gamma=agent.gamma)
    first = last = None
    for k in range(critic_steps):
        agent.evaluate(ring)
        if k == 0 or k == critic_steps - 1:
            last = float(agent.losses[0].item())
            first = last if k == 0 else first
    return out + [{"critic_loss_first": first, "critic_loss_last": last, "transitions": len(ring)}]


OFFLINE_HEADER = ["update", "critic_loss", "actor_loss", "lambda", "mse"]


def offline(agent, ring, updates, record_every=1):
    """OFFLINE training: `updates` calls of agent.replay(ring) with no environment step, on transitions a tracked pass left in `ring`
    (transitions(..., mode="td")), with the behaviour-regularised actor loss holding the actor to the data (agent.bc, ddpg.BC).  The
    normalisation is the caller's (agent.min_max_buffer(ring) or set_norm).  Everything goes on PyTorch's current stream; after update
    u with u % record_every == 0, and after the last, (losses[0], losses[1], lambda, mse) are copied into a device table, which is
    read back in ONE copy at the end.  For a TD3Agent the last three columns are those of the latest policy step.
    Refused by name before anything is trained: agent.bc is None (without the term this is not offline training but replay() on a ring
    nobody refreshes); a ring that holds done = 1 slots -- an "mc" ring, by the rule warm_start documents: its rewards are returns and
    every bootstrapped target would be cut short; an empty ring.
    Returns the rows (update, losses[0], losses[1], lambda, mse) as a list of tuples."""
    if getattr(agent, "bc", None) is None:
        raise ValueError("offline: agent.bc is None: offline training needs the behaviour-regularised actor loss (ddpg.BC)")
    updates, record_every = int(updates), int(record_every)
    if updates < 1 or record_every < 1:
        raise ValueError(f"offline: updates = {updates}, record_every = {record_every}; both at least 1")
    n = len(ring)
    if n < 1:
        raise ValueError("offline: the ring is empty")
    if bool((ring.done[:n] != 0).any()):
        raise ValueError("offline: the ring holds done = 1 slots (an 'mc' ring of returns): bootstrapped training must never sample them; "
                         "seed a 'td' ring (transitions(..., mode='td'))")
    torch = agent.torch
    at = [u for u in range(updates) if u % record_every == 0 or u == updates - 1]
    table = torch.zeros((len(at), 4), dtype=torch.float32, device=agent.device)
    k = 0
    for u in range(updates):
        agent.replay(ring)
        if u == at[k]:
            table[k, 0:2].copy_(agent.losses)
            table[k, 2:3].copy_(agent.bc_lambda)
            table[k, 3:4].copy_(agent.bc_mse)
            k += 1
    rows = table.cpu().numpy()                               # the call's one copy back
    return [(int(u),) + tuple(float(x) for x in r) for u, r in zip(at, rows)]


def write_to_offline_file(rows, path):
    """offline's recorded rows as a CSV beside the imitation file."""
    import csv
    import os
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(OFFLINE_HEADER)
        for r in rows:
            w.writerow([int(r[0])] + [repr(float(x)) for x in r[1:]])
    return path


def _group_check(grp, env, demos, what):
    if env.n != grp.count:
        raise ValueError(f"{what}: the env batch holds {env.n} envs for a group of {grp.count} learners (one env per learner, env l on "
                         "learner l's table and config)")
    if len(demos.rings) != grp.count:
        raise ValueError(f"{what}: {len(demos.rings)} rings for a group of {grp.count} learners")


def _group_passes(grp, env, values):
    """Every learner's CURRENT actor through one harness.inference_many launch, env l with learner l's actor and normalisation."""
    from . import harness
    grp.flux_()
    o, n = grp.layout["actor"]
    lo, hi = grp.layout["s_min"][0], grp.layout["s_max"][0]
    return harness.inference_many(env, grp.slab[:, o:o + n], grp.slab[:, lo:lo + _capi.NSTATE], grp.slab[:, hi:hi + _capi.NSTATE],
                                  num_steps=values.nsteps)


def _group_losses(grp, k):
    """losses[k] of every learner, [count] float64 on the host (one copy)."""
    o = grp.layout["losses"][0]
    return grp.slab[:, o + k].cpu().numpy().astype(np.float64)


def dagger_group(grp, env, values, demos, rounds, steps_per_round, tau=1.0):
    """dagger for a learner group: `env` holds ONE env per learner (env l on learner l's table and config), `values` one problem per
    distinct config (harness.foresight_values(env)), `demos` a GroupDemos.
      round 0          the foresight pass of every env (one foresight.track), learner l's pass into demos.rings[l] with the targets it
                       chose; learner l's normalisation is what learners[l].min_max_buffer(demos.rings[l]) sets;
      round r >= 1     grp.flux_(), all current actors through ONE harness.inference_many launch, ONE foresight.audit over the count
                       passes, and pass l appended to demos.rings[l] with the audit's labels.
    The passes go into the rings learner by learner (count calls of shems_foresight_demos_dev per round); then `steps_per_round`
    grp.clone(demos, tau=tau) steps follow.  Returns one dict per round: "return" [count] (round 0: the foresight passes', later: of
    the actors the round started with), "loss_first" / "loss" [count] (losses[1] after the round's first and last step), "demos" (the
    rings' shared length) and "host_s" (wall time of the round's tracking, audit and demos calls, which synchronise)."""
    import time
    rounds, steps = int(rounds), int(steps_per_round)
    if rounds < 1 or steps < 1:
        raise ValueError(f"dagger_group: {rounds} rounds x {steps} steps; at least one of each")
    _check_values(values, "dagger_group")
    _group_check(grp, env, demos, "dagger_group")
    out = []
    for r in range(rounds):
        t0 = time.perf_counter()
        env.use_torch_stream()
        env.reset_(-1)
        _, _, poe = foresight.problems_of_env(env, np.ones(env.n, np.int64))
        po = (lambda l: poe[l:l + 1]) if values.n_problems > 1 else (lambda l: None)
        if r == 0:
            total, res, targets = foresight.track(env, values, poe, which=-1)
            for l in range(grp.count):
                _write(values, res[l:l + 1], po(l), demos.rings[l], targets=targets[l:l + 1])
                grp.learners[l].min_max_buffer(demos.rings[l])
        else:
            total, res = _group_passes(grp, env, values)
            audit = foresight.audit(values, res, poe if values.n_problems > 1 else None)
            for l in range(grp.count):
                _write(values, res[l:l + 1], po(l), demos.rings[l], best_action=audit.best_action[l:l + 1])
        host_s = time.perf_counter() - t0
        first = None
        for k in range(steps):
            grp.clone(demos, tau=tau)
            if k == 0:
                first = _group_losses(grp, 1)
        last = _group_losses(grp, 1) if steps > 1 else first
        out.append({"return": np.asarray(total, np.float64).copy(), "loss_first": first, "loss": last, "demos": len(demos.rings[0]),
                    "host_s": host_s})
    return out


def warm_start_group(grp, env, values, demos, ring, rounds, steps_per_round, critic_steps, mode="mc", tau=1.0):
    """warm_start for a learner group: dagger_group as it stands, then one pass of every resulting actor (one inference_many launch),
    imitation.transitions of pass l into ring.rings[l] (`ring`: a GroupRings; None: the group's own rings, "td" only, which then go
    straight on as the replay rings) in `mode`, and `critic_steps` grp.evaluate(ring) steps.
    An "mc" ring (done = 1, returns as rewards) must not be the ring bootstrapped training samples: the group's own rings are refused.
    Returns dagger_group's per-round records followed by one dict {"critic_loss_first", "critic_loss_last"} ([count] arrays:
    losses[0] after the first and the last critic step) and "transitions" (the rings' shared length)."""
    _refuse_n_step("warm_start_group", grp)
    if not getattr(grp, "has_evaluate", True):                 # (before dagger_group trains anything: a group without the critic-only update)
        raise NotImplementedError(f"warm_start_group: {type(grp).__name__} has no evaluate() -- the critic-only update of ONE critic -- so "
                                  "its critics cannot be fitted here; nothing was trained")
    critic_steps = int(critic_steps)
    if critic_steps < 1:
        raise ValueError(f"warm_start_group: {critic_steps} critic steps; at least one")
    if mode not in TRANSITION_MODES:
        raise ValueError(f"warm_start_group: mode {mode!r} is neither 'td' nor 'mc'")
    rings = grp.rings if ring is None else ring.rings          # None: the group's own rings ("td": they go straight on as the replay rings)
    _group_check(grp, env, grp if ring is None else ring, "warm_start_group")
    if mode == "mc" and any(a is b for a, b in zip(rings, grp.rings)):
        raise ValueError("warm_start_group: an 'mc' ring holds returns with done = 1 and must not be the group's training ring")
    out = dagger_group(grp, env, values, demos, rounds, steps_per_round, tau=tau)
    _, res = _group_passes(grp, env, values)
    _, _, poe = foresight.problems_of_env(env, np.ones(env.n, np.int64))
    for l in range(grp.count):
        transitions(values, res[l:l + 1], rings[l], poe[l:l + 1] if values.n_problems > 1 else None, mode=mode, gamma=grp.learners[l].gamma)
    first = last = None
    for k in range(critic_steps):
        grp.evaluate(ring)
        if k == 0 or k == critic_steps - 1:
            last = _group_losses(grp, 0)
            first = last if k == 0 else first
    return out + [{"critic_loss_first": first, "critic_loss_last": last, "transitions": len(rings[0])}]


IMITATION_HEADER = ["round", "return", "loss", "demos"]
WARMSTART_HEADER = ["critic_loss_first", "critic_loss_last"]


def write_to_warmstart_file(figures, path):
    """warm_start's critic figures (its last record) as a CSV beside the imitation file."""
    import csv
    import os
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(WARMSTART_HEADER)
        w.writerow([repr(float(figures[k])) for k in WARMSTART_HEADER])
    return path


def write_to_imitation_file(rounds, path):
    """dagger's per-round figures as a CSV beside the foresight results file."""
    import csv
    import os
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(IMITATION_HEADER)
        for k, r in enumerate(rounds):
            w.writerow([k, repr(float(r["return"])), repr(float(r["loss"])), int(r["demos"])])
    return path

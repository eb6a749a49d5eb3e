"""The training loop followed step by step against the CPU oracles (tests/train_ref.py; the follower itself is proven in
tests/test_train_follow_host.py).  Every case builds the workload bench.py times, runs it to t = 70 unfollowed and follows steps 70..75:
real transitions in the ring, targets that have left the online networks, non-zero ADAM moments of both networks, unboosted heads,
the ring's wrap-around and the episode boundary at t = 72 inside the stretch.

The comparisons that needed the tied-relu evaluation (tests/test_group_gpu.py) are deterministic -- seeds, shapes and summation
orders are fixed -- and committed per case in EXPECTED_TIES; the measured errors and run times are in profiles/NOTES.md."""
import importlib
import time

import numpy as np
import pytest

import util as U
from util import oracle_c
import train_ref as TR

pytestmark = pytest.mark.gpu

SEED = 7
T0, FOLLOWED = 70, 6
# case -> [(case, network, step[, learner][, update of the step])]
EXPECTED_TIES = {"host": [], "native-flux": [], "native-tiled": [], "native-tiled-1000": [], "host-2-updates": [],
                 "group-latency": [], "group-throughput": [], "group-latency-window-1": []}


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    return torch, S, D, G


class _Device:
    batch = 120

    def _learner(self, ag):
        # (through the accessors: on the tiled working layout reading a block first brings the Flux-order view up to date)
        return {k: getattr(ag, k).detach().cpu().numpy() for k in TR.LEARNER_KEYS}

    @staticmethod
    def _ring(ring):
        return {k: getattr(ring, k).cpu().numpy() for k in TR.RING_KEYS}

    def _env(self):
        env = self.wl.env
        return dict(obs=env.state, idx=env.idx, step=env.step)


class TrainAdapter(_Device):
    count = 1
    ws_idx, ws_y = TR.WS_IDX, TR.WS_Y
    shadow = None

    def __init__(self, wl, torch, S, D, shadow=False):
        self.wl, self.torch = wl, torch
        self.n = self.E = wl.n
        self.cap, self.updates = wl.ring.capacity, wl.updates
        self.env_seed = wl.env_seed
        self.act_seed = self.rng_seed = wl.agent.rng_seed
        self.table, self.profile = wl.tab, oracle_c.profile(98)
        if shadow:
            # the fused step once more, for the envs the window leaves out: a second learner loaded with the actor and the normalisation
            # of the state before the step, a second env batch set to the pre-act state, one act_step that writes its actions out
            ag2 = D.Agent(seed=1231, rng_seed=wl.agent.rng_seed)
            env2 = S.ShemsBatch(wl.n, wl.EP_LEN, [wl.tab], [S.make_config(98, 0, wl.tab.shape[0])], device=torch.cuda.current_device()).use_torch_stream()
            a_out = torch.empty((wl.n, 2), dtype=torch.float32, device="cuda")

            def launch(Lb, obs, idx, step, tick):
                ag2.set_params(actor=Lb["actor"], sync_targets=False)
                ag2.set_norm(Lb["s_min"], Lb["s_max"])
                env2.state, env2.idx, env2.step = obs, idx, step
                a_out.fill_(float("nan"))
                ag2.act_step(env2, train=True, tick=tick, a_out=a_out)
                torch.cuda.synchronize()
                env2.check_error()
                return a_out.cpu().numpy()
            self.shadow = launch

    def window(self, t):
        return self.wl.win, (t * self.wl.win) % self.wl.n

    def snapshot(self):
        wl, ag = self.wl, self.wl.agent
        self.torch.cuda.synchronize()
        return TR.Snap(learners=[self._learner(ag)], rings=[self._ring(wl.ring)], t=wl.t, episode=wl.episode, pushed=[wl.ring.pushed],
                       updates=ag.updates, bp_actor=list(ag.bp_actor), bp_critic=list(ag.bp_critic), rew32=wl.rew32.cpu().numpy(), **self._env())

    def step(self):
        wl, ag = self.wl, self.wl.agent
        mids = []
        if self.updates > 1:                          # the learner between the step's updates (host loop: replay() is called once per update)
            assert wl.loop == "host"
            real = ag.replay

            def spy(*a, **kw):
                real(*a, **kw)
                if len(mids) < self.updates - 1:
                    self.torch.cuda.synchronize()
                    mids.append([self._learner(ag)])
            ag.replay = spy
            try:
                wl.step()
            finally:
                del ag.replay
        else:
            wl.step()
        return mids


class GroupAdapter(_Device):
    updates = 1
    shadow = None

    def __init__(self, wl, torch):
        self.wl, self.torch = wl, torch
        g = wl.group
        self.count, self.E, self.n, self.cap = g.count, g.envs_per_learner, wl.n, g.capacity
        self.env_seed = wl.env_seed
        self.act_seed = g.learners[0].rng_seed        # the noise is keyed by the global env index under learner 0's key
        self.rng_seed = g.rng_seed                    # learner l samples with rng_seed + l
        self.table, self.profile = wl.tab, oracle_c.profile(98)
        lat = g.form == "latency"                     # the latency form runs the single learner's kernels: the same workspace per learner
        self.ws_idx, self.ws_y = (TR.WS_IDX, TR.WS_Y) if lat else (TR.WS_IDX_TP, None)

    def window(self, t):
        wc = self.wl.win
        return wc, (0 if wc == 1 else (t * wc) % self.E)

    def snapshot(self):
        wl, g = self.wl, self.wl.group
        g.flux_()
        self.torch.cuda.synchronize()
        a0 = g.learners[0]
        assert all(ag.bp_actor == a0.bp_actor and ag.bp_critic == a0.bp_critic and ag.updates == g.updates for ag in g.learners)
        return TR.Snap(learners=[self._learner(ag) for ag in g.learners], rings=[self._ring(r) for r in g.rings], t=wl.t, episode=wl.episode,
                       pushed=[r.pushed for r in g.rings], updates=g.updates, bp_actor=list(a0.bp_actor), bp_critic=list(a0.bp_critic),
                       rew32=None, **self._env())

    def step(self):
        self.wl.step()
        return []


def _expected_wraps(pushed0, win, cap):
    return [t for t in range(T0, T0 + FOLLOWED) if (pushed0 + t * win) % cap + win >= cap]


def _train_case(case, n, loop, updates=1, tiled=None, shadow=False, collect=False):
    torch, S, D, G = _mods()
    t0 = time.perf_counter()
    wl = D.TrainWorkload(S, torch, n, seed=SEED, updates=updates, loop=loop)
    assert wl.loop == loop and wl.win == min(n, 333) and wl.ring.capacity == 24000 and wl.t == 0
    if tiled is not None:
        assert wl.tiled == tiled
    pushed0 = wl.ring.pushed
    wraps = _expected_wraps(pushed0, wl.win, wl.ring.capacity)
    wl.steps(T0)
    assert wl.t == T0 and wl.ring.pushed == pushed0 + T0 * wl.win and wl.agent.updates == T0 * updates
    fol = TR.Follower(TrainAdapter(wl, torch, S, D, shadow=shadow), case, collect=collect).follow(FOLLOWED)
    wl.finish()
    assert fol.steps == list(range(T0, T0 + FOLLOWED)) and fol.boundaries == [72] and fol.wrapped == wraps, (fol.steps, fol.boundaries, fol.wrapped, wraps)
    print(f"{case}: {time.perf_counter() - t0:.2f} s, populate_memory pushed {pushed0}, ring wrapped at {wraps}")
    return fol, wl, pushed0


def _group_case(case, form, window=None, collect=False):
    torch, S, D, G = _mods()
    t0 = time.perf_counter()
    wl = G.GroupWorkload(S, torch, 3 * 128, 3, seed=SEED, form=form, window=window)
    g = wl.group
    assert g.form == form and g.capacity == 24000 and all(len(r) == g.capacity for r in g.rings)
    if form == "throughput":
        assert g.tiled
        g.store_grad = True
    win = wl.win
    assert win == (128 if window is None else window)
    # populate_memory leaves every ring full; the write position is moved so that the window of step 71 straddles the ring's end
    # (one transition per step: step 71 writes the last slot, step 72 -- the first of the next episode -- the first)
    pushed0 = 2 * g.capacity - 71 * win - max(1, win // 2)
    for r in g.rings:
        r.pushed = pushed0
    wraps = _expected_wraps(pushed0, win, g.capacity)
    assert wraps == [71]
    for _ in range(T0):
        wl.step()
    assert wl.t == T0 and g.updates == T0
    fol = TR.Follower(GroupAdapter(wl, torch), case, collect=collect).follow(FOLLOWED)
    wl.finish()
    assert fol.steps == list(range(T0, T0 + FOLLOWED)) and fol.boundaries == [72] and fol.wrapped == wraps, (fol.steps, fol.boundaries, fol.wrapped)
    print(f"{case}: {time.perf_counter() - t0:.2f} s")
    return fol, wl, pushed0


def test_host_loop_whole_batch_window():
    """n = 333: the window is the whole batch, which is ragged against every tile size.  populate_memory runs two rollouts of 333
    episodes (23 976 < 24 000), so the ring's end falls into step 72 -- the same step as the episode boundary."""
    fol, wl, pushed0 = _train_case("host", 333, "host")
    assert pushed0 == 2 * 333 * 72 and fol.wrapped == [72]
    fol.assert_case(EXPECTED_TIES["host"])


def test_native_loop_flux_order(monkeypatch):
    monkeypatch.setenv("SHEMS_AGENT_TILED", "0")
    fol, wl, pushed0 = _train_case("native-flux", 333, "native", tiled=False)
    assert fol.wrapped == [72]
    fol.assert_case(EXPECTED_TIES["native-flux"])


def test_native_loop_tiled(monkeypatch):
    """The default layout, followed as one-step calls: reading the blocks through the accessors between the calls leaves and re-enters
    the tiled regions at every step."""
    monkeypatch.delenv("SHEMS_AGENT_TILED", raising=False)
    fol, wl, pushed0 = _train_case("native-tiled", 333, "native", tiled=True)
    assert fol.wrapped == [72]
    fol.assert_case(EXPECTED_TIES["native-tiled"])


def test_native_loop_tiled_window_of_333_in_1000(monkeypatch):
    """Window 333 of 1000: pushed = 24 048 after populate_memory, step 71 straddles the ring's end, the rotation wraps the batch at
    t = 72 (offset 976); the 667 envs outside the window go through the shadow launch."""
    monkeypatch.delenv("SHEMS_AGENT_TILED", raising=False)
    fol, wl, pushed0 = _train_case("native-tiled-1000", 1000, "native", tiled=True, shadow=True)
    assert pushed0 == 24048 and fol.wrapped == [71] and (72 * 333) % 1000 == 976
    fol.assert_case(EXPECTED_TIES["native-tiled-1000"])


def test_host_loop_two_updates_per_step():
    fol, wl, pushed0 = _train_case("host-2-updates", 333, "host", updates=2)
    assert wl.agent.updates == 2 * (T0 + FOLLOWED) and fol.comparisons == 2 * 12 * FOLLOWED
    fol.assert_case(EXPECTED_TIES["host-2-updates"])


def test_follower_notices_a_wrong_loop_on_the_device():
    """Control on the device itself (the ten wrong compositions are proven on the CPU loop): the host loop with act(t) handed the actor
    from before replay(t - 1), then with replay() handed the update count + 1 as its tick, each after a faithful step that passes."""
    torch, S, D, G = _mods()
    wl = D.TrainWorkload(S, torch, 333, seed=SEED, loop="host")
    wl.steps(2)
    fol = TR.Follower(TrainAdapter(wl, torch, S, D), "control")
    stale = wl.agent.actor.clone()
    fol.step()
    real_act = wl._act
    wl._act = lambda tick: real_act(tick, actor=stale)
    with pytest.raises(TR.FollowError) as e:
        fol.step()
    assert e.value.check == "act", str(e.value)
    del wl._act
    fol.step()
    real_replay = wl.agent.replay
    wl.agent.replay = lambda ring: real_replay(ring, tick=wl.agent.updates + 1)
    with pytest.raises(TR.FollowError) as e:
        fol.step()
    assert e.value.check == "sampler", str(e.value)
    del wl.agent.replay
    fol.step()
    wl.finish()
    assert fol.steps == [2, 3, 4, 5, 6] and not fol.failures


@pytest.mark.parametrize("form", ["latency", "throughput"])
def test_group_whole_block_window(form):
    fol, wl, _ = _group_case("group-" + form, form)
    assert fol.comparisons == 3 * 12 * FOLLOWED
    fol.assert_case(EXPECTED_TIES["group-" + form])


def test_group_one_remembered_transition_per_step():
    """window = 1: household 0 of each block is the only one stored; inside an episode consecutive ring entries are one household's
    trajectory; the households that are not stored are held for idx and step only (their actions are not observable)."""
    fol, wl, pushed0 = _group_case("group-latency-window-1", "latency", window=1)
    cap = wl.group.capacity
    for ring in wl.group.rings:
        s, s2 = ring.s.cpu().numpy(), ring.s2.cpu().numpy()
        for t in range(T0, T0 + FOLLOWED - 1):
            same = bool((U.bits32(s2[(pushed0 + t) % cap]) == U.bits32(s[(pushed0 + t + 1) % cap])).all())
            assert same == (t + 1 != 72), t                     # (entry 72 starts the next episode from its seeded reset)
    fol.assert_case(EXPECTED_TIES["group-latency-window-1"])

"""GPU tests of multi-step (n-step) returns (include/shems_hip.h: shems_nstep_fold_dev, shems_nstep_group_fold_dev,
shems_nstep_from_episodes_dev).  "Ring" means s, a, r, s2, done as bytes.  Everything is held bit for bit: to the NumPy
twin (tests/nstep_ref.py, fed with the device's own staging read-backs where a real step runs in front), to the plain path for
n = 1, and -- for the updates -- to a plain learner whose gamma was set to nstep_gamma(gamma, n).  No tolerance is added anywhere."""
import ctypes as C
import importlib

import numpy as np
import pytest

import nstep_cases as NC
import nstep_ref as NR
import test_ddpg_gpu as TD
import util as U

pytestmark = pytest.mark.gpu
f32 = np.float32
RING_ARRAYS = ("s", "a", "r", "s2", "done")
T6, EPISODES = 6, 2


def _mods():
    torch = pytest.importorskip("torch")
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    return torch, U.pkg(), mod("ddpg"), mod("group"), mod("replay"), mod("td3")


def _upload(torch, ring, host):
    for k in RING_ARRAYS:
        getattr(ring, k).copy_(torch.from_numpy(np.ascontiguousarray(host[k])))


def _download(ring):
    return {k: getattr(ring, k).cpu().numpy().copy() for k in RING_ARRAYS}


def _sentinel_ring(torch, R, capacity, pushed=0):
    ring = R.ReplayRing(capacity)
    _upload(torch, ring, NR.new_ring(capacity))
    ring.pushed = pushed
    return ring


def _env(S, n, steps=T6):
    tab = S.tables.synthetic_table("train", 98)
    return S.ShemsBatch(n, steps, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()


# ------------------------------------------------------------------------------------------ 1. the fold on hand-made staging --
@pytest.mark.parametrize("name,case", NC.fold_cases())
def test_fold_on_hand_made_staging_equals_the_twin(name, case):
    """n in {1, 2, 3, 5, 16}, window in {1, 33, 64}, capacity 100 from position 90 (window 33 wraps mid-window), two episodes back to
    back, T = 6 and T = n: the ring and `pushed` equal the twin bit for bit, untouched slots keep the sentinel."""
    torch, S, D, G, R, T = _mods()
    stages = NC.staging(case)
    want, want_pushed = NC.fold_twin(case, stages)
    ring = _sentinel_ring(torch, R, case["capacity"], case["pos0"])
    nsw = R.NStepWindow(case["n"], case["window"], case["gamma"])
    assert nsw.gamma_n == float(NR.nstep_gamma(case["gamma"], case["n"])) and nsw.window == (0, case["window"], 0)
    for i, st in enumerate(stages):
        _upload(torch, nsw.stage, st)
        hour = i % case["T"]
        before = ring.pushed
        assert nsw.fold(ring, hour) == (hour >= case["n"] - 1)
        assert ring.pushed - before == (case["window"] if hour >= case["n"] - 1 else 0)
    torch.cuda.synchronize()
    assert ring.pushed == want_pushed == case["pos0"] + EPISODES * (case["T"] - case["n"] + 1) * case["window"]
    got = _download(ring)
    assert NC.ring_bytes(got) == NC.ring_bytes(want), name
    touched = min(case["capacity"], ring.pushed - case["pos0"])
    assert (got["done"] == NR.SENT_B).sum() >= case["capacity"] - touched and (got["r"] == NR.SENT_F).sum() == case["capacity"] - touched


# ------------------------------------------------------------------------------------------ 2. the fold behind the real step --
@pytest.mark.parametrize("window", [1, 33, 64])
@pytest.mark.parametrize("n", [1, 3])
def test_fold_behind_the_fused_step(n, window):
    """64 envs, two episodes of 6 hours: the staging ring is read back after every step and fed to the twin; the final ring equals the
    twin's.  n = 1: the ring also equals the plain path's (episode_'s logic with RingWindow(pos, window, 0)) bit for bit."""
    torch, S, D, G, R, T = _mods()
    ag = D.Agent(seed=5, n_step=n)
    env = _env(S, 64)
    ring = _sentinel_ring(torch, R, 100, 90)
    twin_ring, twin_pushed = NR.new_ring(100), 90
    fold = NR.Fold(n, window, ag.gamma)
    nsw = ag.nstep_window(window)
    assert nsw is ag.nstep_window(window) and nsw.n == n
    for ep in range(1, EPISODES + 1):
        env.reset_(17, episode=ep)
        for step in range(T6):
            ag.act_step(env, train=True, tick=ep * 4096 + step, ring=nsw.stage, window=D.RingWindow(*nsw.window))
            st = _download(nsw.stage)
            nsw.fold(ring, step)
            twin_pushed = fold.fold(st, twin_ring, twin_pushed, step)
    torch.cuda.synchronize()
    got = _download(ring)
    assert ring.pushed == twin_pushed == 90 + EPISODES * (T6 - n + 1) * window
    assert NC.ring_bytes(got) == NC.ring_bytes(twin_ring)
    assert not np.isnan(got["r"]).any() and (got["r"] != NR.SENT_F).sum() == min(100, ring.pushed - 90)
    if n == 1:
        plain, env2 = D.Agent(seed=5), _env(S, 64)
        ring2 = _sentinel_ring(torch, R, 100, 90)
        for ep in range(1, EPISODES + 1):
            env2.reset_(17, episode=ep)
            for step in range(T6):
                plain.act_step(env2, train=True, tick=ep * 4096 + step, ring=ring2, window=D.RingWindow(ring2.pos, window, 0))
                ring2.pushed += window
        torch.cuda.synchronize()
        assert NC.ring_bytes(_download(ring2)) == NC.ring_bytes(got) and ring2.pushed == ring.pushed
        env2.close()
    env.close()


# ------------------------------------------------------------------------------------------ 3. the bulk kernel --
@pytest.mark.parametrize("name,case", NC.bulk_cases())
def test_bulk_conversion_equals_the_twin(name, case):
    """Capacity 100, T = 6, n in {1, 3, 6}, episodes * m below and above the capacity (the skip rule shows in the second)."""
    torch, S, D, G, R, T = _mods()
    src_host = NC.bulk_source(case)
    want, want_pushed = NC.bulk_twin(case, src_host)
    src = R.ReplayRing(case["episodes"] * case["T"])
    _upload(torch, src, src_host)
    ring = _sentinel_ring(torch, R, case["capacity"], case["pos0"])
    R.nstep_from_episodes(src, case["episodes"], case["T"], case["n"], case["gamma"], ring)
    torch.cuda.synchronize()
    got = _download(ring)
    assert ring.pushed == want_pushed and NC.ring_bytes(got) == NC.ring_bytes(want), name
    m = case["T"] - case["n"] + 1
    assert ((got["r"] == NR.SENT_F).sum() == 0) == case["skips"] == (case["episodes"] * m > case["capacity"])


@pytest.mark.parametrize("n_envs", [32, 4])
def test_populate_through_the_new_path_leaves_populate_memorys_bytes(n_envs):
    """n = 1: populate_memory_nstep (scratch ring + bulk kernel) leaves Agent.populate_memory's bytes, for env.n >= the 17 episodes a
    ring of 100 needs and for env.n = 4, which takes several rounds."""
    torch, S, D, G, R, T = _mods()
    ag = D.Agent(seed=5)
    out = []
    for new in (False, True):
        env = _env(S, n_envs)
        ring = _sentinel_ring(torch, R, 100, 0)
        ag.populate_memory_nstep(env, ring, seed=9, n_step=1) if new else ag.populate_memory(env, ring, seed=9)
        torch.cuda.synchronize()
        out.append((NC.ring_bytes(_download(ring)), ring.pushed))
        env.close()
    assert out[0] == out[1] and out[0][1] >= 100


def test_populate_n_step_fills_the_ring_with_full_windows():
    """n = 3 through Agent.populate_memory: every slot is written, s' lies three hours behind s (the synthetic table's hour columns
    advance by one row per step) and r is the Horner return of the scratch ring's rewards -- held to the twin on the last round."""
    torch, S, D, G, R, T = _mods()
    ag, env = D.Agent(seed=5, n_step=3), _env(S, 32)
    ring = _sentinel_ring(torch, R, 100, 0)
    scratch = R.ReplayRing(32 * T6)
    ag.populate_memory_nstep(env, ring, seed=9, scratch=scratch)
    torch.cuda.synchronize()
    got, src = _download(ring), _download(scratch)
    assert ring.pushed == 100 and (got["r"] != NR.SENT_F).all()              # 25 episodes x 4 windows: one round of min(32, 25) envs
    want = NR.new_ring(100)
    assert NR.from_episodes(src, 25, T6, 3, ag.gamma, want, 0) == 100
    assert NC.ring_bytes(got) == NC.ring_bytes(want)
    env.close()


# ------------------------------------------------------------------------------------------ 4. the update's discount --
def _learner_bytes(torch, ag, names):
    return {k: getattr(ag, k).view(torch.int32).clone() for k in names}


@pytest.mark.parametrize("kind", ["ddpg", "td3", "per"])
def test_update_of_an_n_step_agent_is_the_plain_update_with_gamma_n(kind):
    """The same ring bytes and seeds: one replay() of an n_step = 3 agent leaves the bytes of a plain agent whose gamma was set to
    nstep_gamma(gamma, 3) -- and not those of a plain agent at gamma."""
    torch, S, D, G, R, T = _mods()
    _, _, _, ag0, ring, h = TD._setup()
    cls = T.TD3Agent if kind == "td3" else D.Agent
    agents = [cls(seed=11, n_step=3), cls(seed=11), cls(seed=11)]
    agents[1].gamma = R.nstep_gamma(agents[1].gamma, 3)
    assert agents[0].gamma == agents[2].gamma == D.GAMMA and agents[0].gamma_n == agents[1].gamma == agents[1].gamma_n
    names = agents[0]._LEARNER_TENSORS
    out = []
    for ag in agents:
        ag.set_params(actor=h["pa"], critic=h["pc"])
        ag.set_norm(h["s_min"], h["s_max"])
        rg = ring
        if kind == "per":
            rg = D.PrioritizedRing(ring.capacity)
            for k in RING_ARRAYS:
                getattr(rg, k).copy_(getattr(ring, k))
            rg.pushed, rg.covered = ring.pushed, ring.pushed - 500         # a fresh range, as behind a fold
            rg.prio.copy_(torch.from_numpy(np.random.default_rng(2).random(ring.capacity).astype(f32)))
        ag.replay(rg, tick=3)
        torch.cuda.synchronize()
        out.append(_learner_bytes(torch, ag, names))
        if kind == "per":
            out[-1]["prio"] = rg.prio.view(torch.int32).clone()
            assert rg.covered == rg.pushed
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), (kind, k)
    assert not torch.equal(out[0]["critic"], out[2]["critic"])


# ------------------------------------------------------------------------------------------ 5. groups --
L3, E32, GCAP, WC = 3, 32, 130, 5
GAMMAS = (0.99, 0.9, 0.95)


def _group_run(cls, n_step, form=None, tiled=None, hparams=None, follow=True, **kw):
    """populate_memory, min_max_buffer and two training episodes of 6 hours with window 5 (act_step, fold, replay -- episode_'s own
    sequence, opened so that every learner's staging ring can be read back).  Capacity 130: populate leaves the rings at position
    126, so the first push wraps mid-window.  Returns (group, twin rings, twin pushed)."""
    torch, S, D, G, R, T = _mods()
    grp = cls(L3, E32, seed=21, rng_seed=77, capacity=GCAP, form=form, tiled=tiled, hparams=hparams, n_step=n_step, **kw)
    env = _env(S, L3 * E32)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    torch.cuda.synchronize()
    twins = [_download(r) for r in grp.rings]
    pushed = [r.pushed for r in grp.rings]
    assert len(set(pushed)) == 1 and (n_step == 1 or pushed[0] % GCAP + WC > GCAP)
    folds = [NR.Fold(n_step, WC, grp.learners[l].gamma) for l in range(L3)]
    for ep in range(1, EPISODES + 1):
        env.reset_(31, episode=ep)
        for step in range(T6):
            win = (grp.rings[0].pos, *grp.ring_window(T6, WC))
            assert win[1:] == (WC, 0) or n_step == 1
            grp.act_step(env, train=True, tick=ep * 4096 + step, window=win)
            if n_step > 1:
                stages = [_download(grp.stage_of(l)) for l in range(L3)] if follow else None
                assert grp.nstep_fold(step) == (step >= n_step - 1)
                if follow:
                    pushed = [folds[l].fold(stages[l], twins[l], pushed[l], step) for l in range(L3)]
            grp.replay()
            grp.tick += 1
    torch.cuda.synchronize()
    env.close()
    return grp, twins, pushed


def _assert_rings(grp, twins, pushed, n_step):
    for l, ring in enumerate(grp.rings):
        assert ring.pushed == pushed[l], l
        assert NC.ring_bytes(_download(ring)) == NC.ring_bytes(twins[l]), l
    assert grp.rings[0].pushed == 256 + EPISODES * (T6 - n_step + 1) * WC


@pytest.mark.parametrize("form,tiled,records", [("throughput", True, True), ("throughput", False, True), ("latency", None, False)])
def test_group_rings_equal_the_twin(form, tiled, records):
    """3 learners x 32 households, n = 3, two episodes of 6 hours: learner l's ring equals the twin fed with that learner's staging
    read-backs and gamma_l; the device records' gamma equals nstep_gamma(gamma_l, 3) while learners[l].gamma stays gamma_l."""
    torch, S, D, G, R, T = _mods()
    hp = [{"gamma": g} for g in GAMMAS] if records else None
    grp, twins, pushed = _group_run(G.LearnerGroup, 3, form=form, tiled=tiled, hparams=hp)
    _assert_rings(grp, twins, pushed, 3)
    assert grp.form == form and grp.tiled == bool(tiled)
    if records:
        rec = (G.HParams * L3).from_buffer_copy(grp._hp_dev.cpu().numpy().tobytes())
        for l, g in enumerate(GAMMAS):
            assert rec[l].gamma == R.nstep_gamma(g, 3) and grp.learners[l].gamma == float(f32(g)) and grp.learners[l].gamma_n == rec[l].gamma
        assert grp._gamma1_dev.cpu().numpy().tolist() == [float(f32(g)) for g in GAMMAS]
        r = [_download(ring)["r"] for ring in grp.rings]
        assert not np.array_equal(r[0], r[1])
    else:
        assert grp._hp_dev is None and grp.learners[0]._ddpg_args().gamma == f32(R.nstep_gamma(D.GAMMA, 3))
    grp.flux_()
    assert all(torch.isfinite(grp.slab[:, grp.layout[k][0]:grp.layout[k][0] + grp.layout[k][1]]).all() for k in ("actor", "critic"))


@pytest.mark.parametrize("form,tiled", [("throughput", True), ("latency", None)])
def test_group_with_n_step_1_leaves_todays_bytes(form, tiled):
    """LearnerGroup(n_step=1) after populate and two episodes: the slab -- rings and parameters -- equals a LearnerGroup's that was
    not told about n_step, and nothing was carved."""
    torch, S, D, G, R, T = _mods()
    a, _, _ = _group_run(G.LearnerGroup, 1, form=form, tiled=tiled)
    env = _env(S, L3 * E32)
    b = G.LearnerGroup(L3, E32, seed=21, rng_seed=77, capacity=GCAP, form=form, tiled=tiled)
    b.populate_memory(env, seed=5)
    b.min_max_buffer()
    for ep in range(1, EPISODES + 1):
        b.episode_(env, train=True, rng_ep=31, episode=ep, window_count=WC)
    torch.cuda.synchronize()
    a.flux_(), b.flux_()
    assert a.layout == b.layout and a.slab_floats == b.slab_floats and not any(k.startswith("ns_") for k in a.layout)
    assert torch.equal(a.slab.view(torch.int32), b.slab.view(torch.int32))
    assert [r.pushed for r in a.rings] == [r.pushed for r in b.rings]
    env.close()


@pytest.mark.parametrize("kind", ["td3", "per"])
def test_td3_and_prioritized_groups_with_n_step_3(kind):
    torch, S, D, G, R, T = _mods()
    cls = T.TD3LearnerGroup if kind == "td3" else G.PrioritizedLearnerGroup
    grp, twins, pushed = _group_run(cls, 3)
    _assert_rings(grp, twins, pushed, 3)
    grp.flux_()
    params = [k for k in grp.layout if k.split("_")[0] in ("actor", "critic", "critic2", "m", "v") and grp.layout[k][1]]
    assert {"actor", "critic", "actor_t", "critic_t", "m_actor", "v_critic"} <= set(params) and ("critic2" in params) == (kind == "td3")
    for k in params:                               # (the workspaces hold integer words too: only parameters, targets and moments are held)
        o, cnt = grp.layout[k]
        assert torch.isfinite(grp.slab[:, o:o + cnt]).all(), k
    assert grp.updates == EPISODES * T6 and not torch.equal(grp.slab[0, :1000], torch.zeros_like(grp.slab[0, :1000]))
    assert list(grp.layout)[-8:] == ["ns_stage_s", "ns_stage_a", "ns_stage_r", "ns_stage_s2", "ns_stage_done", "ns_hist_s", "ns_hist_a", "ns_hist_r"]
    if kind == "per":
        assert grp.covered == grp.rings[0].pushed


# ------------------------------------------------------------------------------------------ 6. run_episodes --
def test_run_episodes_of_an_n_step_agent():
    torch, S, D, G, R, T = _mods()
    ag = D.Agent(seed=5, n_step=3)
    env = _env(S, 64)
    tab = S.tables.synthetic_table("eval", 98)
    env_eval = S.ShemsBatch(8, 1439, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    ring = D.ReplayRing(600)
    ag.populate_memory(env, ring, seed=9)
    ag.min_max_buffer(ring)
    base = ring.pushed
    total, score, best_run, best_actor = ag.run_episodes(env, env_eval, ring, 3, test_every=2, test_runs=8)
    window = min(64, 600 // T6)
    assert ring.pushed - base == 3 * (T6 - 3 + 1) * window and ag.updates == 3 * T6
    assert np.isfinite(total).all() and np.isfinite(score).all() and len(score) == 2 and best_run in (1, 3) and np.isfinite(best_actor).all()
    env.close(), env_eval.close()


def test_run_episodes_of_an_n_step_group():
    torch, S, D, G, R, T = _mods()
    grp = G.LearnerGroup(L3, E32, seed=21, rng_seed=77, capacity=GCAP, n_step=3)
    env = _env(S, L3 * E32)
    env_eval = G.eval_batch([S.tables.synthetic_table("eval", 98)], [0] * L3, L3, test_runs=8, maxsteps=1439, charger_ids=(98,))
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    base = grp.rings[0].pushed
    res = grp.run_episodes(env, env_eval, 3, test_every=2, test_runs=8, window_count=WC)
    assert [r.pushed - base for r in grp.rings] == [3 * (T6 - 3 + 1) * WC] * L3 and grp.updates == 3 * T6
    assert res.sweeps == 2 and torch.isfinite(res._total).all() and torch.isfinite(res._score_mean).all()
    env.close()

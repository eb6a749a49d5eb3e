"""GPU tests of the learner group's evaluation sweeps (LearnerGroup.run_episodes, shems_group_eval_best_dev): run_episodes against a
group driven by hand the way Agent.run_episodes drives one learner (DDPG.jl:244-298), for the latency, tiled throughput, per-learner
(hparams) and wide forms; sweeps leave no trace in the training state; the snapshot of a tiled group reads W2 from the tiles; the
compare is strict and the score is the ascending float64 sum."""
import ctypes as C
import importlib

import numpy as np
import pytest

import util as U
import ddpg_oracle as DO

pytestmark = pytest.mark.gpu
f32 = np.float32
E, CAP, NUM_EP, TEST_EVERY, TEST_RUNS = 32, 2400, 5, 2, 100
EVAL_IDS = (1, 98)


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    return torch, S, D, G


FORMS = {
    "latency": dict(count=3, kw=dict(form="latency")),
    "tiled": dict(count=4, kw=dict(form="throughput", tiled=True)),
    "hparams": dict(count=4, kw=dict(tiled=True, hparams=[{"hidden": (150, 300), "sigma": 0.2}, {}, {"hidden": (200, 400), "mu": 0.05},
                                                          {"batch": 64, "eta_act": 2e-4}])),
    "wide": dict(count=3, kw=dict(form="wide", hparams=[{"hidden": (300, 600), "batch": 150}, {"hidden": (200, 400)}, {"sigma": 0.15}])),
}
# the forms whose fused group step the existing tests hold byte-equal to the single-learner step (tests/test_group_gpu.py,
# tests/test_group_hparams_gpu.py): their eval scores must be the Agent's bit for bit.  The wide group step is held to act() + the
# oracle's step instead (tests/test_group_wide_gpu.py): its scores are compared to 1e-6 relative.
BITWISE = ("latency", "tiled", "hparams")


def _group(name):
    torch, S, D, G = _mods()
    spec = FORMS[name]
    L = spec["count"]
    tab = S.tables.synthetic_table("train", 98)
    env = S.ShemsBatch(L * E, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    grp = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=CAP, **spec["kw"])
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    return env, grp


def _eval_tables(S):
    return [S.tables.synthetic_table("eval", c) for c in EVAL_IDS]


def _grouped_eval(G, S, L):
    return G.eval_batch(_eval_tables(S), [l % len(EVAL_IDS) for l in range(L)], L, test_runs=TEST_RUNS, maxsteps=1439,
                        charger_ids=EVAL_IDS)


def _single_evals(S, L):
    tabs = _eval_tables(S)
    out = []
    for l in range(L):
        k = l % len(EVAL_IDS)
        out.append(S.ShemsBatch(TEST_RUNS, 1439, [tabs[k]], [S.make_config(EVAL_IDS[k], 0, tabs[k].shape[0])]).use_torch_stream())
    return out


def _ulp_close(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool((np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).all())


def _host_noise_sum(grp, G, D, episode):
    """Per env of the training batch: the sum over one training episode of act()'s noise mean (mu_l + sigma_l z, z keyed by the global
    env index), float32 in step order."""
    L = grp.count
    mu = np.array([ag.mu for ag in grp.learners], f32).repeat(E)
    sg = np.array([ag.sigma for ag in grp.learners], f32).repeat(E)
    acc = np.zeros(L * E, f32)
    for step in range(72):
        z = DO.gauss_noise(grp.rng_seed, (episode * 4096 + step) & 0xFFFFFFFF, L * E)
        n0, n1 = mu + sg * z[:, 0], mu + sg * z[:, 1]
        acc = (acc + f32(0.5) * (n0 + n1)).astype(f32)
    return acc


@pytest.mark.parametrize("name", list(FORMS))
def test_run_episodes_equals_the_hand_driven_reference(name):
    torch, S, D, G = _mods()
    env_a, ga = _group(name)
    env_b, gb = _group(name)
    L = ga.count
    n_sw = -(-NUM_EP // TEST_EVERY)
    evals = _single_evals(S, L)
    # ---- reference: the group trains, each learner is evaluated through its Agent (Agent.run_episodes' sweep) -----------------------
    total = np.zeros((L, NUM_EP), f32)
    noise = np.zeros((L, NUM_EP), f32)
    score_mean = np.zeros((L, n_sw))
    best_score, best_run = np.full(L, -100000.0), np.zeros(L, np.int64)
    best_actor, fired = [None] * L, set()
    for i in range(1, NUM_EP + 1):
        nacc = torch.zeros(L * E, dtype=torch.float32, device=ga.device)
        ret = ga.episode_(env_a, train=True, rng_ep=ga.seed, episode=i, noise_acc=nacc)
        total[:, i - 1] = ret.view(L, E).cpu().numpy().mean(1).astype(f32)
        noise[:, i - 1] = nacc.view(L, E).mean(1).cpu().numpy()
        if i == 1:                                   # every form accumulates act()'s noise mean by global env index
            np.testing.assert_allclose(nacc.cpu().numpy(), _host_noise_sum(ga, G, D, 1), rtol=0, atol=2e-5)
            assert float(nacc.abs().max()) > 0.05
        if i % TEST_EVERY != 1:
            continue
        k = -(-i // TEST_EVERY) - 1
        ga.flux_()
        for l, ag in enumerate(ga.learners):
            r = ag.episode_(evals[l], None, train=False, num_steps=72, rng_ep=D.SEED_INI, episode=0).cpu().numpy()
            s = 0.0
            for j in range(TEST_RUNS):
                s += float(r[j])
            s /= TEST_RUNS
            score_mean[l, k] = s
            if s > best_score[l]:
                best_score[l], best_run[l], best_actor[l] = s, i, ag.export_actor()
                fired.add((l, i))
    # ---- run_episodes ------------------------------------------------------------------------------------------------------------
    env_eval = _grouped_eval(G, S, L)
    assert env_eval.n == L * 128
    got_best, got_eval = {}, []
    res = gb.run_episodes(env_b, env_eval, NUM_EP, test_every=TEST_EVERY, test_runs=TEST_RUNS,
                          on_eval=lambda l, i, tr, sc: got_eval.append((l, i, tr, sc)),
                          on_best=lambda l, i, a, tr, sm: got_best.__setitem__((l, i), (a.copy(), tr.copy(), sm.copy())))
    assert res.sweeps == n_sw and res.sweep_ms > 0 and res.wall_ms > res.sweep_ms
    sm = res.score_mean
    assert sm.shape == (L, n_sw) and sm.dtype == np.float64
    if name in BITWISE:
        assert np.array_equal(sm.view(np.uint64), score_mean.view(np.uint64)), (name, sm, score_mean)
    else:
        np.testing.assert_allclose(sm, score_mean, rtol=1e-6, atol=0)
    assert np.array_equal(res.best_run, best_run)
    assert set(got_best) == fired
    for l in range(L):
        assert best_actor[l] is not None
        assert np.array_equal(res.best_actor(l).view(np.uint32), best_actor[l].view(np.uint32)), (name, l)
        a, tr, smr = got_best[(l, int(best_run[l]))]
        assert np.array_equal(a.view(np.uint32), best_actor[l].view(np.uint32))
        assert tr.shape == (int(best_run[l]),) and smr.shape == (-(-int(best_run[l]) // TEST_EVERY),)
        mn, mx = res.best_norm(l)
        assert np.array_equal(mn, gb.learners[l].s_min.cpu().numpy()) and np.array_equal(mx, gb.learners[l].s_max.cpu().numpy())
    assert len(got_eval) == L * n_sw
    assert _ulp_close(res.total_reward, total), (res.total_reward, total)
    assert _ulp_close(res.noise_mean, noise), (res.noise_mean, noise)
    assert res.total_reward.dtype == np.float32 and res.noise_mean.dtype == np.float32
    # on return flux_() has run: the learners' Agents show the last actor, and both groups trained the same
    assert gb._flux_valid
    ga.flux_()
    for l in range(L):
        assert np.array_equal(gb.learners[l].export_actor().view(np.uint32), ga.learners[l].export_actor().view(np.uint32))
    for e in [env_a, env_b, env_eval, *evals]:
        e.check_error()
        e.close()


@pytest.mark.parametrize("name", ["tiled", "wide"])
def test_sweeps_leave_no_trace(name):
    torch, S, D, G = _mods()
    out = []
    for te in (TEST_EVERY, 100):                     # sweeps at episodes 1, 3 and 5 / at episode 1 only
        env, grp = _group(name)
        env_eval = _grouped_eval(G, S, grp.count)
        res = grp.run_episodes(env, env_eval, NUM_EP, test_every=te, test_runs=TEST_RUNS)
        assert res.sweeps == (3 if te == TEST_EVERY else 1)
        torch.cuda.synchronize()
        out.append((grp.slab.clone(), grp.tick, grp.updates, [(r.pos, r.pushed) for r in grp.rings], grp._flux_valid, grp._tiled_valid,
                    [(list(a.bp_actor), list(a.bp_critic), a.updates) for a in grp.learners], res.total_reward, res.noise_mean))
        env.close()
        env_eval.close()
    (s1, *h1, t1, n1), (s2, *h2, t2, n2) = out
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))       # networks, targets, moments, tiles, workspace, rings
    assert h1 == h2
    assert np.array_equal(t1, t2) and np.array_equal(n1, n2)


def _eval_best(grp, returns, runs, episode, score, best_score, best_run, improved, best, stride, t=None, e_eval=128):
    d, g = grp.learners[0]._ddpg_args(), grp.struct()
    g.envs_per_learner = e_eval
    l1, l2 = grp.hidden if grp.form == "wide" else (0, 0)
    p = lambda x: C.c_void_p(x.data_ptr())
    return grp.L.shems_group_eval_best_dev(C.byref(d), C.byref(g), C.byref(t) if t is not None else None, l1, l2, p(returns), runs, episode,
                                          p(score), p(best_score), p(best_run), p(improved), p(best), stride, grp._stream())


def test_tiled_snapshot_reads_w2_from_the_tiles():
    torch, S, D, G = _mods()
    env, grp = _group("tiled")
    L = grp.count
    for i in (1, 2):
        grp.episode_(env, train=True, rng_ep=3, episode=i)
    assert not grp._flux_valid and grp._tiled_valid
    stale = grp.slab[:, grp.layout["actor"][0]:grp.layout["actor"][0] + grp.layout["actor"][1]].clone()
    na = grp.layout["actor"][1]
    row = ((na + 3) & ~3) + 32
    best = torch.zeros((L, row), dtype=torch.float32, device=grp.device)
    kw = dict(score=torch.zeros(L, dtype=torch.float64, device=grp.device),
              best_score=torch.full((L,), -100000.0, dtype=torch.float64, device=grp.device),
              best_run=torch.zeros(L, dtype=torch.int32, device=grp.device), improved=torch.zeros(L, dtype=torch.uint8, device=grp.device))
    ret = torch.zeros(L * 128, dtype=torch.float64, device=grp.device)
    assert _eval_best(grp, ret, TEST_RUNS, 2, best=best, stride=row * 4, t=grp.w2t_struct(), **kw) == 0, grp.L.shems_last_error()
    torch.cuda.synchronize()
    assert not grp._flux_valid and grp._tiled_valid                      # the launch leaves the layout flags alone
    assert bool((kw["improved"] == 1).all())
    grp.flux_()
    fresh = grp.slab[:, grp.layout["actor"][0]:grp.layout["actor"][0] + na]
    assert not torch.equal(stale, fresh)                                 # the Flux-order W2 was stale before flux_()
    assert torch.equal(best[:, :na].view(torch.int32), fresh.view(torch.int32))
    for l, ag in enumerate(grp.learners):
        assert np.array_equal(best[l, :na].cpu().numpy().view(np.uint32), ag.actor.cpu().numpy().view(np.uint32))
        o = (na + 3) & ~3
        assert torch.equal(best[l, o:o + 9], ag.s_min) and torch.equal(best[l, o + 16:o + 25], ag.s_max)
    env.close()


def test_compare_is_strict_and_the_score_is_the_ascending_sum():
    torch, S, D, G = _mods()
    env, grp = _group("latency")
    L, dev = grp.count, grp.device
    na = grp.layout["actor"][1]
    row = ((na + 3) & ~3) + 32
    runs = 3
    r = np.full((L, 128), 1e300)                     # envs runs .. 127 are padding: never read
    r[0, :runs] = [1.0, 1e16, -1e16]                 # ascending: (1 + 1e16) - 1e16 = 0; any other order gives 1 or 1/3
    r[1, :runs] = -100000.0                          # equals the initial best: not an improvement
    r[2, :runs] = [-99999.0, -99998.5, -99999.25]
    ret = torch.as_tensor(r.ravel(), device=dev)
    sentinel = np.array([0x7FC00123], np.uint32).view(f32)[0]
    best = torch.full((L, row), float(sentinel), dtype=torch.float32, device=dev)
    score = torch.zeros(L, dtype=torch.float64, device=dev)
    best_score = torch.full((L,), -100000.0, dtype=torch.float64, device=dev)
    best_run = torch.zeros(L, dtype=torch.int32, device=dev)
    improved = torch.full((L,), 7, dtype=torch.uint8, device=dev)
    kw = dict(score=score, best_score=best_score, best_run=best_run, improved=improved, best=best, stride=row * 4)
    assert _eval_best(grp, ret, runs, 5, **kw) == 0
    host = []
    for l in range(L):
        s = 0.0
        for j in range(runs):
            s += float(r[l, j])
        host.append(s / runs)
    assert np.array_equal(score.cpu().numpy().view(np.uint64), np.array(host).view(np.uint64))
    assert host[0] == 0.0 and host[1] == -100000.0
    assert improved.cpu().tolist() == [1, 0, 1]
    assert best_run.cpu().tolist() == [5, 0, 5]
    assert best_score.cpu().tolist() == [host[0], -100000.0, host[2]]
    b = best.cpu().numpy().view(np.uint32)
    assert (b[1] == 0x7FC00123).all()                                    # no improvement: the old bytes stay
    for l in (0, 2):
        assert np.array_equal(b[l, :na], grp.learners[l].actor.cpu().numpy().view(np.uint32))
    # the same returns again: equal scores, nothing improves, nothing is rewritten
    before = best.clone()
    grp.learners[0].actor.add_(1.0)
    assert _eval_best(grp, ret, runs, 9, **kw) == 0
    assert improved.cpu().tolist() == [0, 0, 0] and best_run.cpu().tolist() == [5, 0, 5]
    assert torch.equal(best.view(torch.int32), before.view(torch.int32))
    env.close()

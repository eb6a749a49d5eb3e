"""GPU tests of learner groups with per-learner hyper-parameters (shems_group_hparams): uniform records give the bits of the shared
entry points, learners stay independent, every learner is held to the float64 oracle with its own batch / gamma / tau / eta, the
action noise follows each learner's mu / sigma, and zero-padded smaller networks stay padded."""
import importlib

import numpy as np
import pytest

import util as U
import ddpg_oracle as DO
import test_group_gpu as TG

pytestmark = pytest.mark.gpu
f32 = np.float32


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    return torch, S, D, G


def _env(S, n):
    tab = S.tables.synthetic_table("train", 98)
    return S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()


def _group(L, E, cap=2400, hparams=None, tiled=None, form="throughput"):
    torch, S, D, G = _mods()
    env = _env(S, L * E)
    grp = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=cap, form=None if hparams is not None else form, tiled=tiled, hparams=hparams)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    env.reset_(9, episode=1)
    return env, grp


def _run(env, grp, steps=2, window=None):
    """act/step + update, `steps` times; returns the actions and returns of every step (host arrays)."""
    torch = grp.torch
    grp.store_grad = True
    out = []
    for t in range(steps):
        a = torch.empty((grp.n_envs, 2), dtype=torch.float32, device="cuda")
        ret = torch.zeros(grp.n_envs, dtype=torch.float64, device="cuda")
        grp.act_step(env, train=True, tick=10 + t, a_out=a, returns_acc=ret, window=(grp.rings[0].pos, *grp.ring_window(72, window)))
        grp.tick += 1
        grp.replay(tick=20 + t)
        out.append((a.cpu().numpy(), ret.cpu().numpy()))
    grp.flux_()
    torch.cuda.synchronize()
    env.check_error()
    return out


def _same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


# (learners, envs per learner, tiled) -> the fused-step form the dispatcher picks (group_act_kernel_name): every group form is covered
FORMS = [(16, 32, False, "shems::k_actg<1, 4, 2, 3>"), (16, 128, False, "shems::k_actg<1, 4, 2, 3>"), (160, 32, False, "shems::k_actg<1, 4, 2, 2>"),
         (520, 32, False, "shems::k_actg<1, 8, 1, 3>"), (256, 64, False, "shems::k_act<2, 4, 2>"), (256, 128, False, "shems::k_act<4, 4, 2>"),
         (1, 16384, False, "shems::k_act2"), (16, 64, True, "shems::k_act<1, 4, 2>"), (256, 64, True, "shems::k_act<2, 4, 2>"),
         (256, 128, True, "shems::k_act<4, 4, 2>")]


@pytest.mark.parametrize("window", [1, None])
@pytest.mark.parametrize("L,E,tiled,form", FORMS)
def test_uniform_records_equal_the_shared_entry_points_bitwise(L, E, tiled, form, window):
    torch, S, D, G = _mods()
    assert G.group_act_kernel_name(L * E, E, tiled) == form
    cap = 400 if L * E > 8192 else 2400
    env_a, ga = _group(L, E, cap=cap, tiled=tiled)
    env_b, gb = _group(L, E, cap=cap, tiled=tiled, hparams=[{}] * L)          # every record = today's defaults
    assert gb.form == "throughput" and gb.tiled == tiled
    ra, rb = _run(env_a, ga, window=window), _run(env_b, gb, window=window)
    for (aa, ret_a), (ab, ret_b) in zip(ra, rb):
        assert _same_bits(aa, ab) and _same_bits(ret_a, ret_b)
    assert _same_bits(env_a.state, env_b.state)
    # networks, targets, moments, gradients, losses, workspace and rings of every learner
    assert torch.equal(ga.slab.view(torch.int32), gb.slab.view(torch.int32))


def _records3():
    return [dict(batch=17, gamma=0.95, tau=5e-3, eta_act=5e-4, eta_crit=5e-3, sigma=0.3, mu=0.05),
            dict(batch=100, gamma=0.999, tau=1e-3, eta_act=1e-5, eta_crit=1e-4, sigma=0.2, hidden=(200, 400)),
            dict(batch=128, gamma=0.99, tau=1e-3, eta_act=1e-4, eta_crit=1e-3, sigma=0.1)]


@pytest.mark.parametrize("tiled", [True, False])
def test_learners_stay_independent(tiled):
    """Learner l of a group cycling three records equals learner l of a group that gives record l % 3 to every learner."""
    torch, S, D, G = _mods()
    recs = _records3()
    L, E = 9, 64
    env_h, gh = _group(L, E, tiled=tiled, hparams=[recs[l % 3] for l in range(L)])
    rh = _run(env_h, gh)
    for k in range(3):
        env_k, gk = _group(L, E, tiled=tiled, hparams=[recs[k]] * L)
        rk = _run(env_k, gk)
        for l in range(k, L, 3):
            assert torch.equal(gh.slab[l].view(torch.int32), gk.slab[l].view(torch.int32)), (k, l)
            sl = slice(l * E, (l + 1) * E)
            for (ah, reth), (ak, retk) in zip(rh, rk):
                assert _same_bits(ah[sl], ak[sl]) and _same_bits(reth[sl], retk[sl]), (k, l)


def _tied_units(p, x, in_dim, out_dim):
    """TG._tied_units without the hidden units of a zero-padded network that are exactly zero for every sample: both sides switch
    those off (relu(0) = 0), they are no ties."""
    _, (_, z1, _, z2, _, _) = DO.mlp_forward(p, x, in_dim, out_dim, out_dim == 2, keep=True, dtype=np.float64)
    out = []
    for z, off in ((z1, in_dim * 250), (z2, in_dim * 250 + 250 + 250 * 500)):
        for u in np.unique(np.where(np.abs(z) < TG.TIE)[1]):
            col = z[:, u]
            if not col.any():
                continue
            out.append((off + int(u), float(np.sign(col[np.argmin(np.abs(col))]) or 1.0)))
    return out


def _blocks_or_tie(TD, g, evaluate, nets, in_dim, out_dim, what):
    """TG._assert_blocks_or_the_other_relu_decision with _tied_units above."""
    base = {k: v[0] for k, v in nets.items()}
    try:
        return TD._assert_blocks(g, evaluate(base), in_dim, out_dim, what), False
    except AssertionError:
        tied = [(name, i, sg) for name, (p, x, i_d, o_d) in nets.items() for i, sg in _tied_units(p, x, i_d, o_d)]
        if not tied or len(tied) > 3:
            raise
        flipped = {k: v.astype(np.float64) for k, v in base.items()}
        for name, i, sg in tied:
            flipped[name][i] -= sg * 4 * TG.TIE
        return TD._assert_blocks(g, evaluate(flipped), in_dim, out_dim, what + " (tied relus decided the other way)"), True


def _hp_vs_float64(records, check=None, ticks=(3, 4), tiled=None):
    """_throughput_vs_float64 of tests/test_group_gpu.py with learner l's batch / gamma / tau / eta from records[l]."""
    import test_ddpg_gpu as TD
    torch, S, D, G = _mods()
    L = len(records)
    env, grp = _group(L, 128, cap=2400, hparams=records, tiled=tiled)
    grp.store_grad = True
    rng = np.random.default_rng(5)
    check = list(range(L)) if check is None else sorted(set(int(l) for l in check))
    host, ties = {}, []
    for l, ag in enumerate(grp.learners):
        pa, pc = ag.actor.cpu().numpy().copy(), ag.critic.cpu().numpy().copy()
        pa[128000:129000] *= 30.0
        pc[128250:128750] *= 30.0
        pa[2250:2500] = rng.normal(0, 0.05, 250); pc[2750:3000] = rng.normal(0, 0.05, 250)
        ag.set_params(actor=pa, critic=pc)
        ring = grp.rings[l]
        ring.done.copy_(torch.from_numpy((rng.random(ring.capacity) < 0.05).astype(np.uint8)))
        if l in check:
            h = grp.hparams[l]
            host[l] = dict(pa=pa, pc=pc, pat=pa.copy(), pct=pc.copy(), s=ring.s.cpu().numpy(), a=ring.a.cpu().numpy(), r=ring.r.cpu().numpy(),
                           s2=ring.s2.cpu().numpy(), done=ring.done.cpu().numpy(), s_min=ag.s_min.cpu().numpy(), s_max=ag.s_max.cpu().numpy(),
                           opt_c=DO.Adam(len(pc), f32(h["eta_crit"])), opt_a=DO.Adam(len(pa), f32(h["eta_act"])),
                           batch=h["batch"], gamma=f32(h["gamma"]), tau=f32(h["tau"]))
    for tick in ticks:
        grp.replay(tick=tick)
        grp.flux_()
        torch.cuda.synchronize()
        for l in check:
            ag, h = grp.learners[l], host[l]
            idx = DO.sample_indices(grp.rng_seed + l, tick, h["batch"], len(grp.rings[l]))
            Lr = DO.Learner(h["pa"], h["pc"], h["s_min"], h["s_max"])
            s, a, r, s2, done = (h[k][idx] for k in ("s", "a", "r", "s2", "done"))
            s2n = DO.normalize(s2, h["s_min"], h["s_max"])
            q2 = DO.critic_forward(h["pct"], s2n, DO.actor_forward(h["pat"], s2n))
            y = (r + h["gamma"] * (f32(1) - done.astype(f32)) * q2).astype(f32)          # DDPG.jl:133 with the learner's gamma
            gc64, lc64 = Lr.critic_grad(s, a, y, dtype=np.float64)
            gc = ag.grad_critic.cpu().numpy()
            sn = DO.normalize(s, h["s_min"], h["s_max"])

            def crit_eval(P):
                return DO.Learner(h["pa"], P["critic"], h["s_min"], h["s_max"]).critic_grad(s, a, y, dtype=np.float64)[0]
            _, tie = _blocks_or_tie(TD, gc, crit_eval, {"critic": (h["pc"], np.concatenate([sn, a], 1), 11, 1)}, 11, 1,
                                                                  f"critic gradient of learner {l}, tick {tick}")
            if tie:
                ties.append(("critic", l, tick))
            losses = ag.losses.cpu().numpy()
            assert abs(losses[0] - lc64) < 1e-4 * max(1.0, abs(lc64)), (l, tick)
            pc1 = h["opt_c"].step(h["pc"], gc)
            crit = ag.critic.cpu().numpy()
            np.testing.assert_allclose(crit, pc1, rtol=0, atol=1e-7)
            np.testing.assert_allclose(ag.critic_t.cpu().numpy(), DO.soft_update(h["pct"], crit, h["tau"]), rtol=0, atol=1e-7)
            np.testing.assert_allclose(ag.m_critic.cpu().numpy(), h["opt_c"].m, rtol=1e-6, atol=1e-12)
            np.testing.assert_allclose(ag.v_critic.cpu().numpy(), h["opt_c"].v, rtol=1e-6, atol=1e-15)
            Lr.critic = crit
            ga64, la64 = Lr.actor_grad(s, dtype=np.float64)
            ga = ag.grad_actor.cpu().numpy()
            a_pi = DO.actor_forward(h["pa"], sn, dtype=np.float64)

            def act_eval(P):
                return DO.Learner(P["actor"], P["critic"], h["s_min"], h["s_max"]).actor_grad(s, dtype=np.float64)[0]
            _, tie = _blocks_or_tie(TD, ga, act_eval, {"actor": (h["pa"], sn, 9, 2),
                                                                                     "critic": (crit, np.concatenate([sn, a_pi], 1), 11, 1)},
                                                                  9, 2, f"actor gradient of learner {l}, tick {tick}")
            if tie:
                ties.append(("actor", l, tick))
            assert abs(losses[1] - la64) < 1e-4 * max(1.0, abs(la64)), (l, tick)
            pa1 = h["opt_a"].step(h["pa"], ga)
            act = ag.actor.cpu().numpy()
            np.testing.assert_allclose(act, pa1, rtol=0, atol=1e-7)
            np.testing.assert_allclose(ag.actor_t.cpu().numpy(), DO.soft_update(h["pat"], act, h["tau"]), rtol=0, atol=1e-7)
            np.testing.assert_allclose(ag.m_actor.cpu().numpy(), h["opt_a"].m, rtol=1e-6, atol=1e-12)
            np.testing.assert_allclose(ag.v_actor.cpu().numpy(), h["opt_a"].v, rtol=1e-6, atol=1e-15)
            h["pa"], h["pc"], h["pat"], h["pct"] = act, crit, ag.actor_t.cpu().numpy(), ag.critic_t.cpu().numpy()
            h["opt_c"].m, h["opt_c"].v = ag.m_critic.cpu().numpy().astype(h["opt_c"].m.dtype), ag.v_critic.cpu().numpy().astype(h["opt_c"].v.dtype)
            h["opt_a"].m, h["opt_a"].v = ag.m_actor.cpu().numpy().astype(h["opt_a"].m.dtype), ag.v_actor.cpu().numpy().astype(h["opt_a"].v.dtype)
    end = grp.layout["grad_actor"][0]
    assert bool(torch.isfinite(grp.slab[:, :end]).all())
    print("per-learner hyper-parameters vs float64: ties set aside", ties)
    return ties, grp


def _mixed_records(L):
    batches, gammas, taus = (17, 100, 120, 128), (0.95, 0.99, 0.999), (1e-3, 5e-3)
    etas, sigmas = ((1e-5, 1e-4), (5e-4, 5e-3), (1e-4, 1e-3)), (0.1, 0.2, 0.3)
    return [dict(batch=batches[l % 4], gamma=gammas[l % 3], tau=taus[l % 2], eta_act=etas[(l // 2) % 3][0], eta_crit=etas[(l // 2) % 3][1],
                 sigma=sigmas[(l // 3) % 3]) for l in range(L)]


# (learners, tiled) -> [(network, learner, tick)] of the committed seeds
EXPECTED_TIES = {(11, True): [], (11, False): [], (48, True): [], (400, True): [("actor", 223, 4)]}


@pytest.mark.parametrize("L,tiled", [(11, True), (11, False), (48, True)])       # 11: the narrow launch shapes; 48: the wide ones
def test_per_learner_hparams_match_float64_oracle_per_block(L, tiled):
    ties, _ = _hp_vs_float64(_mixed_records(L), tiled=tiled)
    assert ties == EXPECTED_TIES[(L, tiled)], ties


def test_benched_width_cycling_the_36_runnable_tuned_points():
    torch, S, D, G = _mods()
    recs, points, skipped = G.tuned_grid(G.TUNED_RUNNABLE)
    assert len(points) == 36 and not skipped
    L = 400
    check = (0, L - 1, L // 2, 37, 101, 166, 223, 289, 310, 371)
    ties, grp = _hp_vs_float64([recs[l % 36] for l in range(L)], check=check)
    assert grp.n_envs == 400 * 128
    assert ties == EXPECTED_TIES[(400, True)], ties


def test_per_learner_noise_follows_each_learners_mu_and_sigma():
    torch, S, D, G = _mods()
    recs = [dict(sigma=s, mu=m) for s, m in ((0.1, 0.0), (0.3, 0.0), (0.2, -0.1), (0.0, 0.2))] * 4
    env, grp = _group(16, 64, hparams=recs)
    n, E = grp.n_envs, grp.envs_per_learner
    obs = env.state
    a = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    grp.act_step(env, train=True, tick=5, a_out=a)
    a = a.cpu().numpy()
    zn = DO.gauss_noise(grp.rng_seed, 5, n)
    for l, ag in enumerate(grp.learners):
        sl = slice(l * E, (l + 1) * E)
        clean = DO.act(ag.actor.cpu().numpy(), obs[sl], ag.s_min.cpu().numpy(), ag.s_max.cpu().numpy(), False, dtype=np.float64)
        ref = np.clip(clean + (f32(recs[l]["mu"]) + f32(recs[l]["sigma"]) * zn[sl]), -1, 1)
        assert np.abs(a[sl] - ref).max() < 2e-5, l
        assert ag.sigma == pytest.approx(recs[l]["sigma"]) and ag.mu == pytest.approx(recs[l]["mu"])


def test_padded_learners_stay_padded_and_export_unpadded():
    torch, S, D, G = _mods()
    hid = [(150, 300), (200, 400), (250, 500)] * 6
    env, grp = _group(18, 64, hparams=[dict(hidden=h, batch=64) for h in hid])
    for ep in range(3):
        grp.episode_(env, num_steps=12, rng_ep=3, episode=ep + 1)
    grp.flux_()
    torch.cuda.synchronize()
    for l, ag in enumerate(grp.learners):
        assert ag.hidden == hid[l]
        for net, (i, o) in (("actor", (9, 2)), ("critic", (11, 1))):
            pad = D.pad_net(np.ones(D.net_size(i, o, hid[l]), np.float32), i, o, hid[l]) == 0
            for k in (net, net + "_t", "m_" + net, "v_" + net):
                x = getattr(ag, k).cpu().numpy()
                assert not x[pad].any(), (l, k)
                if hid[l] != (250, 500):
                    assert pad.any()
        ea, ec = ag.export_actor(), ag.export_critic()
        assert ea.size == D.net_size(9, 2, hid[l]) and ec.size == D.net_size(11, 1, hid[l])
        assert _same_bits(D.pad_net(ea, 9, 2, hid[l]), ag.actor.cpu().numpy())
        assert _same_bits(D.pad_net(ec, 11, 1, hid[l]), ag.critic.cpu().numpy())

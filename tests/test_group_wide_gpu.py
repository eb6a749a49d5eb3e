"""GPU tests of the wide learner-group form (LearnerGroup(form="wide"), shems_wide_group_update / shems_wide_act_step_group_dev): the
layer-by-layer path of csrc/shems_wide.hip with a learner dimension.  Per learner it is bit-identical to the single-learner wide path at
a pass width of 128, every learner is held to the float64 oracle with its own hidden size, batch (up to 256), gamma, tau and eta, the
fused step to act() + the C oracle's step, padding stays exact, learners stay independent, and the tuned grid's 81 points train as
one group."""
import importlib

import numpy as np
import pytest

import util as U
from util import oracle_c
import ddpg_oracle as DO

pytestmark = pytest.mark.gpu
f32 = np.float32
HID = (300, 600)
BLOCK_TOL = 2e-6


@pytest.fixture
def wide_oracle(monkeypatch):
    monkeypatch.setattr(DO, "L1", HID[0])
    monkeypatch.setattr(DO, "L2", HID[1])
    return DO


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    return torch, S, D, G


def _env(S, n):
    tab = S.tables.synthetic_table("train", 98)
    return S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()


def _group(L, E, cap=2400, hparams=None, hidden=None):
    torch, S, D, G = _mods()
    env = _env(S, L * E)
    grp = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=cap, form="wide", hparams=hparams, hidden=hidden)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    env.reset_(9, episode=1)
    return env, grp


def _same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def _boost(ag, rng, hid):
    """Lift the 3e-3 heads of learner `ag` (its own units only: the padding stays zero) so tanh and every gradient path are exercised."""
    pa, pc = ag.export_actor(), ag.export_critic()
    h2 = hid[1]
    pa[-(2 * h2 + 2):-2] *= 40.0
    pa[-2:] = [0.3, -0.2]
    pc[-(h2 + 1):-1] *= 30.0
    ag.set_params(actor=pa, critic=pc)


def _pad_mask(D, hid, i, o):
    return D.pad_net_to(np.ones(D.net_size(i, o, hid), f32), i, o, hid, HID) == 0


def test_wide_group_equals_the_single_learner_wide_path_bitwise():
    torch, S, D, G = _mods()
    L = 4
    env, grp = _group(L, 64)
    assert grp.hidden == HID and not grp.tiled and grp.max_batch == 128
    rng = np.random.default_rng(3)
    for ag in grp.learners:
        assert ag.wide and ag.hidden == HID
        ag.batch = 120
        _boost(ag, rng, HID)
    singles = []
    for l, ag in enumerate(grp.learners):
        one = D.Agent(seed=grp.seed + l, rng_seed=grp.rng_seed + l, hidden=HID)
        one.batch = 120
        one.set_params(actor=ag.actor.cpu().numpy(), critic=ag.critic.cpu().numpy())
        one.set_norm(ag.s_min.cpu().numpy(), ag.s_max.cpu().numpy())
        ring = D.ReplayRing(grp.capacity)
        src = grp.rings[l]
        for t, v in ((ring.s, src.s), (ring.a, src.a), (ring.r, src.r), (ring.s2, src.s2), (ring.done, src.done)):
            t.copy_(v)
        ring.pushed = src.pushed
        assert len(ring) == len(src)
        singles.append((one, ring))
    for tick in (0, 1, 2):
        grp.replay(tick=tick)
        for one, ring in singles:
            one.replay(ring, tick=tick)
    torch.cuda.synchronize()
    for l, ag in enumerate(grp.learners):
        one = singles[l][0]
        for k in ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic"):
            assert torch.equal(getattr(ag, k).view(torch.int32), getattr(one, k).view(torch.int32)), (l, k)


def _mixed_records():
    hid = [(300, 600), (250, 500), (200, 400), (150, 300)]
    batch = [50, 120, 128, 150, 200, 256, 128, 150]
    return [dict(hidden=hid[l % 4], batch=batch[l], gamma=(0.95, 0.99, 0.999)[l % 3], tau=(1e-3, 5e-3)[l % 2],
                 eta_act=(1e-4, 5e-4, 1e-5)[l % 3], eta_crit=(1e-3, 5e-3, 1e-4)[l % 3], sigma=0.1 + 0.05 * (l % 3), mu=0.02 * (l % 2))
            for l in range(8)]


def _blocks(g, g64, in_dim, out_dim, what):
    errs = {}
    for name, lo, hi in DO.blocks(in_dim, out_dim):
        ref = np.abs(g64[lo:hi]).max()
        if ref == 0:                             # a block of a padded network's extra units: exactly zero on both sides
            assert not g[lo:hi].any(), (what, name)
            continue
        errs[name] = float(np.abs(g[lo:hi] - g64[lo:hi]).max() / ref)
    assert all(e < BLOCK_TOL for e in errs.values()), (what, errs)
    return errs


def _learner_tick_matches_float64(grp, l, ag, h, tick):
    """Learner l of `grp` after its update at `tick`: every gradient block against float64 (_blocks), the losses, ADAM + soft update
    and the moments element-wise from its own gradient; then `h` (the learner's host copy) is advanced to the kernel's state.  Returns
    the block errors."""
    errs = {}
    idx = DO.sample_indices(grp.rng_seed + l, tick, h["batch"], len(grp.rings[l]))
    Lr = DO.Learner(h["pa"], h["pc"], h["s_min"], h["s_max"])
    s, a, r, s2, done = (h[k][idx] for k in ("s", "a", "r", "s2", "done"))
    s2n = DO.normalize(s2, h["s_min"], h["s_max"])
    q2 = DO.critic_forward(h["pct"], s2n, DO.actor_forward(h["pat"], s2n))
    y = (r + h["gamma"] * (f32(1) - done.astype(f32)) * q2).astype(f32)
    gc64, lc64 = Lr.critic_grad(s, a, y, dtype=np.float64)
    gc = ag.grad_critic.cpu().numpy()
    errs["critic"] = _blocks(gc, gc64, 11, 1, f"critic gradient of learner {l}, tick {tick}")
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
    errs["actor"] = _blocks(ga, ga64, 9, 2, f"actor gradient of learner {l}, tick {tick}")
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
    return errs


def test_mixed_records_match_float64_per_learner_and_block(wide_oracle):
    torch, S, D, G = _mods()
    recs = _mixed_records()
    env, grp = _group(len(recs), 64, hparams=recs)
    assert grp.hidden == HID and grp.max_batch == 256
    rng = np.random.default_rng(5)
    host = {}
    for l, ag in enumerate(grp.learners):
        _boost(ag, rng, recs[l]["hidden"])
        ring = grp.rings[l]
        ring.done.copy_(torch.from_numpy((rng.random(ring.capacity) < 0.05).astype(np.uint8)))
        h = grp.hparams[l]
        pa, pc = ag.actor.cpu().numpy(), ag.critic.cpu().numpy()
        host[l] = dict(pa=pa, pc=pc, pat=pa.copy(), pct=pc.copy(), s=ring.s.cpu().numpy(), a=ring.a.cpu().numpy(), r=ring.r.cpu().numpy(),
                       s2=ring.s2.cpu().numpy(), done=ring.done.cpu().numpy(), s_min=ag.s_min.cpu().numpy(), s_max=ag.s_max.cpu().numpy(),
                       opt_c=DO.Adam(len(pc), f32(h["eta_crit"])), opt_a=DO.Adam(len(pa), f32(h["eta_act"])),
                       batch=h["batch"], gamma=f32(h["gamma"]), tau=f32(h["tau"]))
    for tick in (3, 4):
        grp.replay(tick=tick)
        torch.cuda.synchronize()
        for l, ag in enumerate(grp.learners):
            _learner_tick_matches_float64(grp, l, ag, host[l], tick)
    assert bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())     # (ws holds int32 slot indices)


@pytest.mark.parametrize("train", [False, True])
def test_fused_group_step_equals_act_then_oracle_step_and_fills_each_ring(wide_oracle, train):
    torch, S, D, G = _mods()
    recs = [dict(hidden=h, sigma=sg, mu=mu) for h, sg, mu in (((300, 600), 0.1, 0.0), ((200, 400), 0.3, 0.05), ((250, 500), 0.2, -0.1),
                                                               ((150, 300), 0.0, 0.2))]
    L, E = len(recs), 64
    env, grp = _group(L, E, hparams=recs)
    rng = np.random.default_rng(11)
    for l, ag in enumerate(grp.learners):
        _boost(ag, rng, recs[l]["hidden"])
    n = grp.n_envs
    tab = S.tables.synthetic_table("train", 98)
    ref = oracle_c.Batch(n, 72, tab, oracle_c.profile(98))
    ref.set_state(env.state, env.idx)
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    ret = torch.zeros(n, dtype=torch.float64, device="cuda")
    wc = 16
    for t in range(3):
        pre = env.state
        pos = grp.rings[0].pos
        win = (pos, wc, (t * wc) % E)
        grp.act_step(env, train=train, tick=7 + t, a_out=a_out, returns_acc=ret, window=win)
        env.check_error()
        a = a_out.cpu().numpy()
        zn = DO.gauss_noise(grp.rng_seed, 7 + t, n)
        for l, ag in enumerate(grp.learners):
            sl = slice(l * E, (l + 1) * E)
            clean = DO.act(ag.actor.cpu().numpy(), pre[sl], ag.s_min.cpu().numpy(), ag.s_max.cpu().numpy(), False, dtype=np.float64)
            want = np.clip(clean + (f32(recs[l]["mu"]) + f32(recs[l]["sigma"]) * zn[sl]), -1, 1) if train else clean
            assert np.abs(a[sl] - want).max() < 5e-6, (l, t)
        rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
        assert rc == 0
        assert (U.bits32(env.state) == U.bits32(o_ref)).all()
        for l in range(L):                       # the window rotates inside each learner's block and pushes into its own ring
            rel = (np.arange(E) - win[2]) % E
            sel = np.where(rel < wc)[0]
            slots = (pos + rel[sel]) % grp.capacity
            ring = grp.rings[l]
            g = l * E + sel
            assert (U.bits32(ring.s.cpu().numpy()[slots]) == U.bits32(pre[g])).all(), (l, t)
            assert (U.bits32(ring.s2.cpu().numpy()[slots]) == U.bits32(o_ref[g])).all(), (l, t)
            assert (U.bits32(ring.a.cpu().numpy()[slots]) == U.bits32(a[g])).all(), (l, t)
            assert (ring.r.cpu().numpy()[slots] == r_ref[g].astype(np.float32)).all(), (l, t)
    env.close()


def test_padding_stays_exact_exports_are_own_size_and_learners_independent():
    torch, S, D, G = _mods()
    hid = [(150, 300), (200, 400), (250, 500), (300, 600)] * 2
    recs = [dict(hidden=h, batch=(64, 150)[l % 2]) for l, h in enumerate(hid)]
    L, E = len(recs), 32
    runs = []
    for perturb in (False, True):
        env, grp = _group(L, E, hparams=recs)
        if perturb:
            ag = grp.learners[2]
            pa = ag.export_actor()
            pa[:50] += 0.01
            ag.set_params(actor=pa, sync_targets=False)
        for ep in range(2):
            grp.episode_(env, num_steps=6, rng_ep=3, episode=ep + 1)
        torch.cuda.synchronize()
        runs.append(grp)
    grp, other = runs
    for l, ag in enumerate(grp.learners):
        assert ag.hidden == hid[l] and ag.whidden == HID
        for net, (i, o) in (("actor", (9, 2)), ("critic", (11, 1))):
            pad = _pad_mask(D, hid[l], i, o)
            for k in (net, net + "_t", "m_" + net, "v_" + net, "grad_" + net):
                assert not getattr(ag, k).cpu().numpy()[pad].any(), (l, k)
            assert pad.any() == (hid[l] != HID)
        ea, ec = ag.export_actor(), ag.export_critic()
        assert ea.size == D.net_size(9, 2, hid[l]) and ec.size == D.net_size(11, 1, hid[l])
        assert _same_bits(D.pad_net_to(ea, 9, 2, hid[l], HID), ag.actor.cpu().numpy())
        assert _same_bits(D.pad_net_to(ec, 11, 1, hid[l], HID), ag.critic.cpu().numpy())
        same = torch.equal(grp.slab[l].view(torch.int32), other.slab[l].view(torch.int32))
        assert same == (l != 2), l


def test_the_whole_tuned_grid_trains_as_one_group():
    torch, S, D, G = _mods()
    recs, points, skipped = G.tuned_grid(range(81), wide=True)
    assert len(recs) == 81 and not skipped
    L, E, cap = 81, 32, 2400
    env, grp = _group(L, E, cap=cap, hparams=recs)
    assert grp.hidden == HID and grp.max_batch == 150
    pushed0 = [ring.pushed for ring in grp.rings]
    for ep in range(2):
        grp.episode_(env, num_steps=4, rng_ep=3, episode=ep + 1, window_count=8)
    torch.cuda.synchronize()
    env.check_error()
    assert bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())     # (ws holds int32 slot indices)
    assert grp.updates == 8
    for l, (ag, ring) in enumerate(zip(grp.learners, grp.rings)):
        assert len(ring) == cap and ring.pushed == pushed0[l] + 8 * 8
        assert ag.updates == 8 and ag.batch == recs[l]["batch"]
        for net, (i, o) in (("actor", (9, 2)), ("critic", (11, 1))):
            pad = _pad_mask(D, ag.hidden, i, o)
            assert not getattr(ag, net).cpu().numpy()[pad].any(), l


def test_cross_check_against_the_tuned_group_at_250_500(monkeypatch):
    """The same records (batch <= 128) in a form="wide" group at (250, 500) and in the tuned throughput group: two float32
    implementations with different summation orders, within the block tolerance after each of 2 updates."""
    torch, S, D, G = _mods()
    monkeypatch.setattr(DO, "L1", 250)
    monkeypatch.setattr(DO, "L2", 500)
    recs = [dict(hidden=h, batch=b, gamma=g) for h, b, g in (((250, 500), 120, 0.99), ((200, 400), 64, 0.95), ((150, 300), 128, 0.999),
                                                             ((250, 500), 17, 0.9))]
    L, E = len(recs), 64
    env_w, gw = _group(L, E, hparams=recs, hidden=(250, 500))
    env_t = _env(S, L * E)
    gt = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=2400, hparams=recs)
    gt.populate_memory(env_t, seed=5)
    gt.min_max_buffer()
    gt.store_grad = True
    assert gw.form == "wide" and gt.form == "throughput"
    for l in range(L):
        for k in ("actor", "critic", "s_min", "s_max"):
            assert torch.equal(getattr(gw.learners[l], k), getattr(gt.learners[l], k)), (l, k)
        assert torch.equal(gw.rings[l].s, gt.rings[l].s)
    for tick in (0, 1):
        gw.replay(tick=tick)
        gt.replay(tick=tick)
        gt.flux_()
        torch.cuda.synchronize()
        for l in range(L):
            aw, at = gw.learners[l], gt.learners[l]
            for net, (i, o) in (("critic", (11, 1)), ("actor", (9, 2))):
                gwv, gtv = getattr(aw, "grad_" + net).cpu().numpy(), getattr(at, "grad_" + net).cpu().numpy()
                for name, lo, hi in DO.blocks(i, o):
                    ref = np.abs(gtv[lo:hi]).max()
                    if ref == 0:
                        assert not gwv[lo:hi].any(), (l, net, name)
                        continue
                    tol = 2 * BLOCK_TOL if tick == 0 else 1e-4       # the second update starts from slightly different parameters
                    assert np.abs(gwv[lo:hi] - gtv[lo:hi]).max() / ref < tol, (tick, l, net, name)
            np.testing.assert_allclose(aw.critic.cpu().numpy(), at.critic.cpu().numpy(), rtol=0, atol=2 * 5e-3 * (tick + 1))

"""TD3 for learner groups on the GPU: td3.TD3LearnerGroup / shems_td3_group_update_tp (csrc/shems_gupd.hip) against the NumPy twin
(tests/td3_ref.py) and float64, per learner, each stage from the device's own previous stage.

Cases, seeds and ticks live in tests/group_td3_cases.py (tests/test_group_td3_host.py proves on the CPU that they meet the coverage
and tie conditions asserted here).  Bounds: a~' 1e-5 and y, q'1, q'2 rtol = atol = 2e-5 (tests/test_td3_gpu.py's); every Flux.params
block of a gradient BLOCK_TOL = 2e-6 of its float64 max-abs; losses 1e-4 max(1, |loss|); ADAM, targets and moments from the kernel's own
gradient with tests/test_group_gpu.py:_throughput_vs_float64's bounds (atol 1e-7; moments rtol 1e-6)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ddpg_oracle as DO
import group_td3_cases as K
import td3_ref as TR
import util as U

pytestmark = pytest.mark.gpu

BLOCK_TOL = 2e-6
E, CAP = K.E, K.CAP
DDPG_SIDE = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic", "losses")
ACTOR_SIDE = ("actor", "actor_t", "m_actor", "v_actor", "grad_actor")
CRITIC1 = ("critic", "critic_t", "m_critic", "v_critic", "grad_critic")
CRITIC2 = ("critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2")
TD3_ARRAYS = DDPG_SIDE + CRITIC2 + ("losses2",)
TL_T = 3                               # the target's array of a tile: [32 tiles][m | v | p | target][64 x 64]


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    return torch, S, mod("ddpg"), mod("group"), mod("td3")


def _fill(torch, grp, l, reward=None):
    d = K.learner_data(l)
    ag, ring = grp.learners[l], grp.rings[l]
    up = lambda t, v: t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    ag.set_norm(d["s_min"], d["s_max"])
    for k in ("s", "a", "r", "s2", "done"):
        up(getattr(ring, k), d[k] if (k != "r" or reward is None) else reward(d))
    ring.pushed = CAP
    return d, up


def _group(L, batch=120, tiled=None, hparams=None, sigma=K.SIGMA, clip=K.CLIP, delay=2, same_critics=False, lift=True, reward=None):
    """An L-learner TD3 group on tests/group_td3_cases.py's data.  same_critics: critic 2 (and its target) a copy of critic 1."""
    torch, S, D, G, T = _mods()
    grp = T.TD3LearnerGroup(L, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=CAP, tiled=tiled, hparams=hparams, sigma_trg=sigma, clip_trg=clip,
                            policy_delay=delay)
    grp.store_grad = True
    for l, ag in enumerate(grp.learners):
        d, up = _fill(torch, grp, l, reward)
        grp.set_params(l, actor=d["pa"], critic=d["pc"], critic2=d["pc"] if same_critics else d["pc2"])
        up(ag.actor_t, d["pa_t"] if lift else d["pa_t_plain"])
        up(ag.critic_t, d["pc_t"])
        up(grp.critic2_t_of(l), d["pc_t"] if same_critics else d["pc2_t"])
        if hparams is None:
            ag.batch = batch
    if grp.tiled:
        grp.flux_changed()
    return torch, grp


def _ddpg_group(L, batch=120, tiled=None, hparams=None, lift=True):
    torch, S, D, G, T = _mods()
    grp = G.LearnerGroup(L, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=CAP, form="throughput", tiled=tiled, hparams=hparams)
    grp.store_grad = True
    for l, ag in enumerate(grp.learners):
        d, up = _fill(torch, grp, l)
        ag.set_params(actor=d["pa"], critic=d["pc"])
        up(ag.actor_t, d["pa_t"] if lift else d["pa_t_plain"])
        up(ag.critic_t, d["pc_t"])
        if hparams is None:
            ag.batch = batch
    if grp.tiled:
        grp.flux_changed()
    return torch, grp


def _bits(grp, name):
    o, n = grp.layout[name]
    return grp.slab[:, o:o + n].contiguous().view(grp.torch.int32).clone()


def _side(grp, names):
    grp.flux_()
    return {k: _bits(grp, k) for k in names}


def _np(grp, l, name):
    o, n = grp.layout[name]
    return grp.slab[l, o:o + n].cpu().numpy()


# --------------------------------------------------------------------------------- 1. the degenerate case leaves DDPG's bits --
@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("L", [2, 48])
def test_degenerate_case_leaves_the_bits_of_the_ddpg_group(L, tiled, records):
    """sigma_trg = 0, every critic 2 a copy of its critic 1 (targets too), d = 1, three updates: the DDPG side holds LearnerGroup.replay()'s
    bytes from the same state, ring, seed and ticks, and critic 2's arrays and losses2 equal critic 1's -- every summation order of the
    new launches is an old one."""
    hp = [{"batch": 120} for _ in range(L)] if records else None
    torch, ref = _ddpg_group(L, tiled=tiled, hparams=hp)
    torch, grp = _group(L, tiled=tiled, hparams=hp, sigma=0.0, delay=1, same_critics=True)
    assert grp.tiled == tiled and ref.tiled == tiled and grp.form == "throughput"
    assert grp.slab_floats > ref.slab_floats and all(grp.layout[k] == ref.layout[k] for k in ref.layout)
    for t in range(3):
        ref.replay(tick=t)
        grp.replay(tick=t)
    torch.cuda.synchronize()
    a, b = _side(grp, TD3_ARRAYS), _side(ref, DDPG_SIDE)
    for k in DDPG_SIDE:
        assert torch.equal(a[k], b[k]), k
    for k1, k2 in zip(CRITIC1, CRITIC2):
        assert torch.equal(a[k2], a[k1]), k2
    assert torch.equal(a["losses2"][:, 0], a["losses"][:, 0])
    assert grp.updates == ref.updates == 3
    for x, y in zip(grp.learners, ref.learners):
        assert x.bp_actor == y.bp_actor and x.bp_critic == y.bp_critic and x.updates == 3
    assert float(grp.learners[L - 1].grad_critic[:3000].abs().max()) > 0 and float(grp.learners[L - 1].grad_actor[:2500].abs().max()) > 0


# ------------------------------------------------------------------ 2. every stage against the twin / float64, per learner --
def _host_state(l, eta_crit=DO.ETA_CRIT, eta_act=DO.ETA_ACT):
    d = K.learner_data(l)
    n = len(d["pc"])
    return dict(pa=d["pa"].copy(), pa_t=d["pa_t"].copy(), pc=d["pc"].copy(), pc_t=d["pc_t"].copy(), pc2=d["pc2"].copy(), pc2_t=d["pc2_t"].copy(),
                opt_c=DO.Adam(n, eta_crit), opt_c2=DO.Adam(n, eta_crit), opt_a=DO.Adam(len(d["pa"]), eta_act))


def _blocks_or_the_other_relu_decision(g, evaluate, nets, in_dim, out_dim, what):
    """tests/test_group_gpu.py's: evaluate(params by net name) -> float64 gradient; a failing block is evaluated again with every tied
    relu (|z| < K.TIE) decided the other way and must pass.  Returns (per-block errors, tie used?)."""
    import test_ddpg_gpu as TD
    base = {k: v[0] for k, v in nets.items()}
    try:
        return TD._assert_blocks(g, evaluate(base), in_dim, out_dim, what, tol=BLOCK_TOL), False
    except AssertionError:
        tied = [(name, i, sg) for name, (p, x, i_d, o_d) in nets.items() for i, sg in K.tied_units(p, x, i_d, o_d)]
        if not tied or len(tied) > 3:
            raise
        flipped = {k: v.astype(np.float64) for k, v in base.items()}
        for name, i, sg in tied:
            flipped[name][i] -= sg * 4 * K.TIE
        return TD._assert_blocks(g, evaluate(flipped), in_dim, out_dim, what + " (tied relus decided the other way)", tol=BLOCK_TOL), True


def _check_update(grp, l, h, tick, B, policy, gamma=DO.GAMMA, tau=DO.TAU, worst=None):
    """Learner l's last update (already on the device, Flux order current) from the host copy `h` of the state it started from; `h` then
    takes the device's bytes.  Returns the ties set aside."""
    d = K.learner_data(l)
    ag = grp.learners[l]
    s, a, r, s2, done = K.minibatch(l, tick, B)
    tw = K.twin_of(h["pa"], h["pa_t"], h["pc"], h["pc_t"], h["pc2"], h["pc2_t"], d["s_min"], d["s_max"])
    tg = tw.targets(r, s2, done, K.RNG_SEED + l, tick)
    what = f"learner {l}, tick {tick}, B={B}, policy={policy}"
    # a~' against the twin with key seed + l; q'1, q'2 and y from the device's own a~'
    a_dev = grp.a_smooth(l).cpu().numpy()[:, :B].T.copy()
    err_a = float(np.abs(a_dev - tg["a_smooth"]).max())
    assert np.isfinite(grp.a_smooth(l).cpu().numpy()).all()                      # pad columns too
    tg2 = tw.targets(r, s2, done, K.RNG_SEED + l, tick, a_smooth=a_dev)
    y_ref = TR.target_y(r, done, tg2["q1"], tg2["q2"], gamma)
    y_dev = grp.y_target(l).cpu().numpy()[:B].copy()
    q1_dev, q2_dev = grp.q_target1(l).cpu().numpy()[:B], grp.q_target2(l).cpu().numpy()[:B]
    print(f"{what}: max |a~' - twin| {err_a:.2e}, |y - twin| {np.abs(y_dev - y_ref).max():.2e}, |q'1| {np.abs(q1_dev - tg2['q1']).max():.2e}, "
          f"|q'2| {np.abs(q2_dev - tg2['q2']).max():.2e}")
    assert err_a <= 1e-5, what
    assert (np.abs(a_dev) <= 1).all() and (np.abs(a_dev) == 1).any() == (np.abs(tg["a_smooth"]) == 1).any()
    np.testing.assert_allclose(q1_dev, tg2["q1"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(q2_dev, tg2["q2"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(y_dev, y_ref, rtol=2e-5, atol=2e-5)
    sn = DO.normalize(s, d["s_min"], d["s_max"])
    x = np.concatenate([sn, a], 1)
    ties = []
    for name, p0, pt0, opt, loss, sfx in (("critic", h["pc"], h["pc_t"], h["opt_c"], float(ag.losses[0]), ""),
                                          ("critic2", h["pc2"], h["pc2_t"], h["opt_c2"], float(grp.losses2[l]), "2")):
        g = _np(grp, l, "grad_critic" + sfx)

        def crit_eval(P):
            return DO.Learner(h["pa"], P[name], d["s_min"], d["s_max"]).critic_grad(s, a, y_dev, dtype=np.float64)[0]
        e, tie = _blocks_or_the_other_relu_decision(g, crit_eval, {name: (p0, x, 11, 1)}, 11, 1, f"{name} gradient, {what}")
        if tie:
            ties.append((name, l, tick))
        _, l64 = DO.Learner(h["pa"], p0, d["s_min"], d["s_max"]).critic_grad(s, a, y_dev, dtype=np.float64)
        print(f"{what}: {name} block errors {e}, loss {loss!r} vs float64 {l64!r}")
        assert abs(loss - l64) < 1e-4 * max(1.0, abs(l64)), (what, name)
        p1 = opt.step(p0, g)                                                     # ADAM from the kernel's own gradient
        crit, crit_t = _np(grp, l, name), _np(grp, l, name + "_t")
        np.testing.assert_allclose(crit, p1, rtol=0, atol=1e-7)
        np.testing.assert_allclose(_np(grp, l, "m_critic" + sfx), opt.m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(_np(grp, l, "v_critic" + sfx), opt.v, rtol=1e-6, atol=1e-15)
        if policy:
            np.testing.assert_allclose(crit_t, DO.soft_update(pt0, crit, np.float32(tau)), rtol=0, atol=1e-7)
            assert not np.array_equal(crit_t, pt0)
        else:
            assert np.array_equal(U.bits32(crit_t), U.bits32(pt0)), f"{name}_t moved off a policy step ({what})"
        opt.m, opt.v = _np(grp, l, "m_critic" + sfx).astype(opt.m.dtype), _np(grp, l, "v_critic" + sfx).astype(opt.v.dtype)
        for k, v in e.items():
            if worst is not None:
                worst[name + "_" + k] = max(worst.get(name + "_" + k, 0.0), v)
        h["pc" + sfx], h["pc" + sfx + "_t"] = crit.copy(), crit_t.copy()
    if policy:                                                                   # the actor through the device's UPDATED critic 1
        ga = _np(grp, l, "grad_actor")
        crit = h["pc"]
        a_pi = DO.actor_forward(h["pa"], sn, dtype=np.float64)

        def act_eval(P):
            return DO.Learner(P["actor"], P["critic"], d["s_min"], d["s_max"]).actor_grad(s, dtype=np.float64)[0]
        e, tie = _blocks_or_the_other_relu_decision(ga, act_eval, {"actor": (h["pa"], sn, 9, 2), "critic": (crit, np.concatenate([sn, a_pi], 1), 11, 1)},
                                                    9, 2, f"actor gradient, {what}")
        if tie:
            ties.append(("actor", l, tick))
        _, la64 = DO.Learner(h["pa"], crit, d["s_min"], d["s_max"]).actor_grad(s, dtype=np.float64)
        print(f"{what}: actor block errors {e}, loss {float(ag.losses[1])!r} vs float64 {la64!r}")
        assert abs(float(ag.losses[1]) - la64) < 1e-4 * max(1.0, abs(la64)), what
        pa1 = h["opt_a"].step(h["pa"], ga)
        act, act_t = _np(grp, l, "actor"), _np(grp, l, "actor_t")
        np.testing.assert_allclose(act, pa1, rtol=0, atol=1e-7)
        np.testing.assert_allclose(act_t, DO.soft_update(h["pa_t"], act, np.float32(tau)), rtol=0, atol=1e-7)
        np.testing.assert_allclose(_np(grp, l, "m_actor"), h["opt_a"].m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(_np(grp, l, "v_actor"), h["opt_a"].v, rtol=1e-6, atol=1e-15)
        h["opt_a"].m, h["opt_a"].v = _np(grp, l, "m_actor").astype(h["opt_a"].m.dtype), _np(grp, l, "v_actor").astype(h["opt_a"].v.dtype)
        for k, v in e.items():
            if worst is not None:
                worst["actor_" + k] = max(worst.get("actor_" + k, 0.0), v)
        h["pa"], h["pa_t"] = act.copy(), act_t.copy()
    else:
        assert np.array_equal(U.bits32(_np(grp, l, "actor")), U.bits32(h["pa"])) and np.array_equal(U.bits32(_np(grp, l, "actor_t")), U.bits32(h["pa_t"]))
    return ties


@pytest.mark.parametrize("L,batch,policy", K.STAGE_CASES)
def test_every_stage_against_the_twin_and_float64(L, batch, policy):
    """Two updates in a row (the second on the advanced powers), learners 0 and L - 1."""
    ticks = K.ticks_of((L, batch, policy))
    for l in K.checked(L):                                                       # on the twin first
        K.assert_coverage(l, ticks[0], batch)
    torch, grp = _group(L, batch)
    assert grp.tiled
    host = {l: _host_state(l) for l in K.checked(L)}
    ties, worst = [], {}
    for tick in ticks:
        grp.replay(tick=tick, update_policy=policy)
        grp.flux_()
        torch.cuda.synchronize()
        for l in K.checked(L):
            ties += _check_update(grp, l, host[l], tick, batch, policy, worst=worst)
    print(f"L={L} B={batch} policy={policy}: worst per-block errors {worst}; ties {ties}")
    assert ties == K.EXPECTED_TIES[(L, batch, policy)], ties
    end = grp.layout["losses2"][0] + 1
    assert bool(torch.isfinite(grp.slab[:, grp.layout["critic2"][0]:end]).all())
    assert grp.updates == 2
    for ag in grp.learners:
        assert abs(ag.bp_critic[0] - 0.9 ** 3) < 1e-15 and (abs(ag.bp_actor[0] - 0.9 ** 3) < 1e-15 if policy else ag.bp_actor == [0.9, 0.999])


# --------------------------------------------------------------------------------------------------- 3. the non-policy step --
@pytest.mark.parametrize("records", [False, True])
def test_non_policy_step_moves_the_critics_and_nothing_else(records):
    hp = [{"batch": 17}, {"batch": 17}] if records else None
    torch, grp = _group(2, 17, hparams=hp)
    for ag in grp.learners:                       # not live off a policy step: made visible
        ag.grad_actor.fill_(-3.0); ag.m_actor.fill_(0.25); ag.v_actor.fill_(0.5)
        ag.losses[1] = 42.0
    grp.flux_changed()
    grp._use_tiled()
    keep = ACTOR_SIDE + ("critic_t", "critic2_t")
    before = _side(grp, keep + ("critic", "critic2", "m_critic", "m_critic2", "v_critic", "v_critic2"))
    tiles = lambda name: _bits(grp, name).view(2, 32, 4, 64 * 64)
    ta0, tc0, tc20 = tiles("w2t_actor"), tiles("w2t_critic")[:, :, TL_T], tiles("w2t_critic2")[:, :, TL_T]
    for tick in K.TICKS:
        grp.replay(tick=tick, update_policy=False)
    torch.cuda.synchronize()
    assert torch.equal(ta0, tiles("w2t_actor"))
    assert torch.equal(tc0, tiles("w2t_critic")[:, :, TL_T]) and torch.equal(tc20, tiles("w2t_critic2")[:, :, TL_T])
    after = _side(grp, tuple(before))
    for k in keep:
        assert torch.equal(before[k], after[k]), k
    for k in ("critic", "critic2", "m_critic", "m_critic2", "v_critic", "v_critic2"):
        assert not torch.equal(before[k], after[k]), k
    o = grp.layout["losses"][0]
    assert (grp.slab[:, o + 1].cpu().numpy() == 42.0).all() and np.isfinite(grp.slab[:, o].cpu().numpy()).all()
    assert np.isfinite(grp.losses2.cpu().numpy()).all()
    assert grp.updates == 2 and all(ag.bp_actor == [0.9, 0.999] and abs(ag.bp_critic[0] - 0.9 ** 3) < 1e-15 for ag in grp.learners)


# ------------------------------------------------------------------------------------------------------------ 4. the schedule --
@pytest.mark.parametrize("delay,n,want", [(2, 4, [False, True, False, True]), (1, 3, [True, True, True]), (3, 4, [False, False, True, False])])
def test_schedule_by_update_policy_none(delay, n, want):
    torch, grp = _group(2, 17, delay=delay)
    moved = []
    for t in range(n):
        before = _side(grp, ("actor",))["actor"]
        grp.replay(tick=t)
        moved.append(not torch.equal(before, _side(grp, ("actor",))["actor"]))
    assert moved == want
    k = sum(want)
    assert grp.updates == n
    for ag in grp.learners:
        assert ag.updates == n
        assert abs(ag.bp_critic[0] - 0.9 ** (n + 1)) < 1e-15 and abs(ag.bp_critic[1] - 0.999 ** (n + 1)) < 1e-15
        assert abs(ag.bp_actor[0] - 0.9 ** (k + 1)) < 1e-15 and abs(ag.bp_actor[1] - 0.999 ** (k + 1)) < 1e-15


# ------------------------------------------------------------------------------------------------- 5. layouts and records --
def _two_updates(L=2, batch=17, **kw):
    torch, grp = _group(L, batch, delay=2, **kw)
    for t in K.TICKS:                             # d = 2 from update 0: a non-policy step, then a policy step
        grp.replay(tick=t)
    torch.cuda.synchronize()
    pub = grp.slab[:, grp.layout["ws2"][0] + 31112:grp.layout["ws2"][0] + 31112 + 5 * 128].contiguous().view(torch.int32).clone()
    return grp, dict(_side(grp, TD3_ARRAYS), pub=pub)


def test_tiled_and_flux_order_leave_the_same_bits():
    gt, tiled = _two_updates(tiled=True)
    gf, flux = _two_updates(tiled=False)
    assert gt.tiled and not gf.tiled
    for k in tiled:
        assert gt.torch.equal(tiled[k], flux[k]), k
    assert not gt.torch.equal(tiled["critic2"], tiled["critic2_t"])


@pytest.mark.parametrize("tiled", [True, False])
def test_uniform_records_leave_the_bits_of_the_shared_entry_point(tiled):
    gs, shared = _two_updates(tiled=tiled)
    gr, rec = _two_updates(tiled=tiled, hparams=[{"batch": 17}, {"batch": 17}])
    assert gr._hp_dev is not None and gs._hp_dev is None and 0.0 in gr._hp_variants      # (the records with tau = 0 were built)
    for k in shared:
        assert gs.torch.equal(shared[k], rec[k]), k


def test_two_learners_with_their_own_batch_eta_and_gamma_meet_their_own_float64():
    for l, rec in enumerate(K.RECORD_CASE):
        K.assert_coverage(l, K.TICKS[0], rec["batch"])
    torch, grp = _group(2, hparams=K.RECORD_CASE)
    host = {l: _host_state(l, eta_crit=float(np.float32(K.RECORD_CASE[l]["eta_crit"]))) for l in range(2)}
    ties = []
    for tick, policy in zip(K.TICKS, (False, True)):
        grp.replay(tick=tick, update_policy=policy)
        grp.flux_()
        torch.cuda.synchronize()
        for l, rec in enumerate(K.RECORD_CASE):
            ties += _check_update(grp, l, host[l], tick, rec["batch"], policy, gamma=np.float32(rec["gamma"]))
    assert ties == []


# --------------------------------------------------------------------------------------- 6. determinism and isolation --
def test_two_runs_leave_the_same_bytes_and_a_learner_does_not_depend_on_the_others():
    g1, a = _two_updates()
    g2, b = _two_updates()
    g3, c = _two_updates(L=3)
    for k in a:
        assert g1.torch.equal(a[k], b[k]), k
        assert g1.torch.equal(a[k], c[k][:2]), k


# ---------------------------------------------------------------------------------------------------------- 7. losses fall --
def test_training_on_a_fixed_ring_reduces_both_critic_losses_of_every_learner():
    """The learnable reward of tests/test_td3_gpu.py (a function of the stored state and action), d = 2, 160 updates: the mean loss of
    the last four updates is below half that of the first four, for both critics of every learner."""
    reward = lambda d: (0.4 * (d["s"][:, 4] - d["s"][:, 3]) + d["a"][:, 1] - 0.5 * d["s"][:, 0]).astype(np.float32)
    torch, grp = _group(2, 120, sigma=0.2, clip=0.5, delay=2, lift=False, reward=reward)
    n_up = 160
    first, last = np.zeros((2, 2)), np.zeros((2, 2))
    o = grp.layout["losses"][0]
    for t in range(n_up):
        grp.replay(tick=t % 4)
        if t < 4 or t >= n_up - 4:
            l = np.stack([grp.slab[:, o].cpu().numpy(), grp.losses2.cpu().numpy()], 1) / 4
            if t < 4:
                first += l
            else:
                last += l
    print("critic losses [learner][critic], first and last four updates:", first, last)
    assert np.isfinite(last).all() and (last < 0.5 * first).all(), (first, last)
    assert grp.updates == n_up
    grp.flux_()
    for k in TD3_ARRAYS:
        oo, n = grp.layout[k]
        assert bool(torch.isfinite(grp.slab[:, oo:oo + n]).all()), k


# -------------------------------------------------------------------------------------------------------- 8. training runs --
def test_run_episodes_and_the_inherited_calls_on_a_td3_group():
    """16 x 32 TD3 group: populate_memory, min_max_buffer, ring_window, two episodes of run_episodes with one evaluation sweep (episode_
    calls the overridden replay), eval_scores; clone leaves both critics' bytes."""
    torch, S, D, G, T = _mods()
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    L = 16
    tab = S.tables.synthetic_table("train")
    env = S.ShemsBatch(L * E, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    grp = T.TD3LearnerGroup(L, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=2400)
    assert grp.form == "throughput" and grp.tiled
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    assert grp.ring_window(72)[0] >= 1
    etab = S.tables.synthetic_table("eval")
    env_eval = G.eval_batch([etab], [0] * L, L, test_runs=32, maxsteps=72)
    res = grp.run_episodes(env, env_eval, 2, test_every=100, test_runs=32)
    torch.cuda.synchronize()
    assert res.sweeps == 1 and grp.updates == 2 * 72
    assert all(ag.updates == 144 and abs(ag.bp_actor[0] - 0.9 ** 73) < 1e-12 for ag in grp.learners)
    best_run = res._best_run.cpu().numpy()
    assert best_run.shape == (L,) and (best_run == 1).all()
    for k in TD3_ARRAYS:
        o, n = grp.layout[k]
        assert bool(torch.isfinite(grp.slab[:, o:o + n]).all()), k
    scores = grp.eval_scores(env_eval, test_runs=32)
    assert scores.shape == (L,) and np.isfinite(scores).all()
    # clone trains the actor alone: both critic sides keep their bytes
    demos = I.GroupDemos(L, 64)
    for l, dm in enumerate(demos.rings):
        d = K.learner_data(l)
        dm.s.copy_(torch.from_numpy(np.ascontiguousarray(d["s"][:64]))); dm.a.copy_(torch.from_numpy(np.ascontiguousarray(d["a"][:64])))
        dm.pushed = 64
    before = _side(grp, CRITIC1 + CRITIC2 + ("actor",))
    grp.clone(demos, tick=0)
    after = _side(grp, CRITIC1 + CRITIC2 + ("actor",))
    for k in CRITIC1 + CRITIC2:
        assert torch.equal(before[k], after[k]), k
    assert not torch.equal(before["actor"], after["actor"]) and grp.clones == 1
    with pytest.raises(NotImplementedError, match="evaluate"):
        grp.evaluate()
    env.close()
    env_eval.close()


def test_dagger_group_on_a_td3_group_trains_the_actors_alone():
    """imitation.dagger_group (two rounds of five supervised steps, S1-sized data as tests/test_group_imitation_gpu.py) on a TD3 group of
    4: both critic sides -- Flux-order arrays and tiles -- keep their bytes, every actor moves, and TD3 updates follow on the result."""
    torch, S, D, G, T = _mods()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    I, F, H = mod("imitation"), mod("foresight"), mod("harness")
    T1 = 30
    tab = U.tables_mod().profile_table(98, "eval")
    cfgs = [S.make_config(98, 0, tab.shape[0]), S.make_config(98, 0, tab.shape[0], disc_weight=0.1, disc_pot=1.0)]
    env = S.ShemsBatch(4, T1, [tab], cfgs, np.array([0, 1, 0, 1], np.uint16)).use_torch_stream()
    val = H.foresight_values(env, F.Grid(9, 5, 5, 3))
    torch, grp = _group(4, 30)
    assert grp.tiled
    grp._use_tiled()                              # the tiles as training would hold them
    names = CRITIC1 + CRITIC2 + ("w2t_critic", "w2t_critic2", "losses2")
    before = _side(grp, names + ("actor",))
    loss0 = _bits(grp, "losses")[:, 0]
    demos = I.GroupDemos(4, 128)
    out = I.dagger_group(grp, env, val, demos, 2, 5)
    torch.cuda.synchronize()
    assert len(out) == 2 and [r["demos"] for r in out] == [T1, 2 * T1] and grp.clones == 10 and grp.updates == 0
    for r in out:
        assert r["loss"].shape == (4,) and np.isfinite(r["loss"]).all() and np.isfinite(r["return"]).all()
    after = _side(grp, names + ("actor",))
    for k in names:
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(loss0, _bits(grp, "losses")[:, 0])
    assert all(not torch.equal(before["actor"][l], after["actor"][l]) for l in range(4))
    assert all(ag.bp_critic == [0.9, 0.999] and abs(ag.bp_actor[0] - 0.9 ** 11) < 1e-15 for ag in grp.learners)
    for t in range(2):                            # d = 2: a non-policy step, then a policy step, on the cloned actors
        grp.replay(tick=t)
    torch.cuda.synchronize()
    moved = _side(grp, TD3_ARRAYS)
    for k in ("critic", "critic2", "actor"):
        assert not torch.equal(moved[k], after[k]), k
    for k in TD3_ARRAYS:
        o, n = grp.layout[k]
        assert bool(torch.isfinite(grp.slab[:, o:o + n]).all()), k
    assert grp.updates == 2
    env.close()


# ------------------------------------------------------------------------------------------------------------ 9. refusals --
def test_c_abi_refusals_launch_nothing():
    torch, S, D, G, T = _mods()
    torch, grp = _group(2, 17, hparams=[{"batch": 17}, {"batch": 17}])
    grp._use_tiled()
    torch.cuda.synchronize()
    snap = grp.slab.clone()
    ERR = S._capi.ERR_ARG
    a0 = grp.learners[0]
    ptr = lambda name: grp.slab.data_ptr() + 4 * grp.layout[name][0]

    def call(t3=None, ring=None, g=None, w="tiled", w2="tiled", hp="own", hold="own", policy=1, flags=0, bp=0.9, length=CAP):
        t3 = grp._td3_args() if t3 is None else t3
        ring = grp._ring0() if ring is None else ring
        g = grp.struct() if g is None else g
        w = C.byref(grp.w2t_struct()) if w == "tiled" else w
        w2 = C.c_void_p(ptr("w2t_critic2")) if w2 == "tiled" else w2
        hp = grp._hp_ptr() if hp == "own" else hp
        hold = grp._hold_ptr() if hold == "own" else hold
        return grp.L.shems_td3_group_update_tp(C.byref(t3), C.byref(ring), C.byref(g), w, w2, hp, hold, length, K.RNG_SEED, 3, a0.eta_crit, bp, 0.999,
                                               a0.eta_act, 0.9, 0.999, policy, flags, grp._stream())

    def args(**kw):
        t3 = grp._td3_args()
        for k, v in kw.items():
            setattr(t3, k, v)
        return t3

    # what shems_ddpg_group_update_tp refuses
    t3 = grp._td3_args(); t3.d.critic_t = None
    assert call(t3) == ERR and b"NULL buffer" in grp.L.shems_last_error()
    assert call(g=G.Group(0, 0, grp.slab_floats * 4, E)) == ERR and call(g=G.Group(2, 0, grp.slab_floats * 4 + 4, E)) == ERR
    assert call(length=0) == ERR and call(length=CAP + 1) == ERR and call(bp=1.0) == ERR and call(flags=2) == ERR
    t3 = grp._td3_args(); t3.d.actor = t3.d.actor + 4
    assert call(t3) == ERR
    t3 = grp._td3_args(); t3.d.batch = 129
    assert call(t3, hp=None, hold=None) == ERR and b"batch" in grp.L.shems_last_error()
    # critic 2: NULL, misaligned, overlapping critic 1
    for k in ("critic2", "critic2_t", "m_critic2", "v_critic2", "ws2", "losses2"):
        assert call(args(**{k: None})) == ERR, k
    assert call(args(grad_critic2=None), flags=1) == ERR
    assert call(args(critic2=ptr("critic2") + 4)) == ERR and call(args(ws2=ptr("ws2") + 8)) == ERR
    assert call(args(critic2=ptr("critic"))) == ERR and b"overlaps" in grp.L.shems_last_error()
    assert call(args(critic2_t=ptr("critic_t"))) == ERR and call(args(m_critic2=ptr("m_critic") + 16 * 100)) == ERR
    assert call(args(ws2=ptr("ws"))) == ERR
    # the tiled regions: one without the other, overlapping critic 1's
    assert call(w=None) == ERR and call(w2=None) == ERR
    assert call(w2=C.c_void_p(ptr("w2t_critic"))) == ERR and b"overlaps critic 1" in grp.L.shems_last_error()
    assert call(w2=C.c_void_p(ptr("w2t_actor") - 64)) == ERR and b"overlaps the actor" in grp.L.shems_last_error()
    assert call(w2=C.c_void_p(ptr("w2t_critic2") + 4)) == ERR and b"16-byte aligned" in grp.L.shems_last_error()
    # losses2 / ws2 inside critic 1's side
    assert call(args(losses2=ptr("losses"))) == ERR and b"losses2 overlaps" in grp.L.shems_last_error()
    assert call(args(losses2=ptr("losses") + 4)) == ERR and call(args(losses2=ptr("losses2") + 2)) == ERR
    assert call(args(ws2=ptr("ws") + 16 * 1000)) == ERR and b"ws2 overlaps" in grp.L.shems_last_error()
    assert call(args(grad_critic2=ptr("grad_critic2") + 4), flags=1) == ERR
    # d_hp_hold missing when it is needed (and not needed on a policy step)
    assert call(hold=None, policy=0) == ERR and b"d_hp_hold" in grp.L.shems_last_error()
    # sigma_trg, clip_trg, update_policy
    for bad in (-0.1, float("nan"), float("inf")):
        assert call(args(sigma_trg=bad)) == ERR and call(args(clip_trg=bad)) == ERR
    assert call(policy=2) == ERR and call(policy=-1) == ERR
    assert grp.L.shems_td3_group_update_tp(None, None, None, None, None, None, None, CAP, 1, 1, 1e-3, 0.9, 0.999, 1e-3, 0.9, 0.999, 1, 0, None) == ERR
    torch.cuda.synchronize()
    assert torch.equal(grp.slab.view(torch.int32), snap.view(torch.int32))          # the canary: nothing was launched
    assert call(hold=None, policy=1) == 0                                           # a policy step reads no d_hp_hold
    torch.cuda.synchronize()
    assert not torch.equal(grp.slab.view(torch.int32), snap.view(torch.int32))


def test_python_refusals_name_their_reason():
    torch, S, D, G, T = _mods()
    torch, grp = _group(2, 17)
    with pytest.raises(NotImplementedError, match="evaluate"):
        grp.evaluate()
    grp.learners[0].batch = 129
    with pytest.raises(NotImplementedError, match="batch 129"):
        grp.replay()
    grp.learners[0].batch = 17
    with pytest.raises(ValueError, match="critic2 has"):
        grp.set_params(0, critic2=np.zeros(17, np.float32))
    with pytest.raises(NotImplementedError, match="learner group"):
        T.TD3Agent(tensors={})
    # warm_start_group needs evaluate(): refused before its DAgger stage trains anything
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    torch.cuda.synchronize()
    snap = grp.slab.clone()
    with pytest.raises(NotImplementedError, match="evaluate"):
        I.warm_start_group(grp, None, None, None, None, 2, 5, 5)
    assert torch.equal(grp.slab.view(torch.int32), snap.view(torch.int32)) and grp.clones == 0
    # a generator of records is walked once
    g2 = T.TD3LearnerGroup(2, E, capacity=CAP, hparams=({"batch": 17} for _ in range(2)))
    assert [h["batch"] for h in g2.hparams] == [17, 17]
    assert grp.updates == 0


# ---------------------------------------------------------------------------------------- 10. no effect on DDPG groups --
# slab_floats of a DDPG LearnerGroup(2, 32, capacity=128, form="throughput") on the parent commit
PARENT_SLAB_FLOATS = {True: 4243932, False: 3195356}


@pytest.mark.parametrize("tiled", [True, False])
def test_a_ddpg_group_keeps_the_parents_layout(tiled):
    torch, S, D, G, T = _mods()
    grp = G.LearnerGroup(2, E, seed=K.SEED, capacity=CAP, form="throughput", tiled=tiled)
    assert grp.slab_floats == PARENT_SLAB_FLOATS[tiled]
    assert list(grp.layout)[-1] == "ring_done" and "critic2" not in grp.layout
    assert grp.layout["actor"] == (0, D.N_ACTOR) and grp.layout["ws"][1] == 1902568
    td3 = T.TD3LearnerGroup(2, E, seed=K.SEED, capacity=CAP, tiled=tiled)
    assert all(td3.layout[k] == grp.layout[k] for k in grp.layout)
    assert td3.layout["critic2"][0] == grp.slab_floats

"""GPU tests of the TD3 update (shems_td3_update, td3.TD3Agent) against the NumPy twin (tests/td3_ref.py) and float64.

Every case is one learner on the ring of tests/test_ddpg_gpu.py:_setup (24 000 slots).  The bounds are the project's: a~' 1e-5 absolute
(the act path's); y from the device's a~' rtol = atol = 2e-5; every gradient block of both critics (from the device's y) and
of the actor (through the device's updated critic 1) BLOCK_TOL = 2e-6 of its float64 max-abs; ADAM and the soft update from the
kernel's own gradient atol 1e-7, moments rtol 1e-6; losses 1e-4 max(1, |ref|).  Each stage is checked from the device's own previous
stage, as test_ddpg_gpu.test_one_update_matches_oracle does."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import ddpg_oracle as DO
import td3_ref as TR
import test_ddpg_gpu as TD
import util as U

pytestmark = pytest.mark.gpu

BLOCK_TOL = TD.BLOCK_TOL
TIE = 1e-7                       # a relu whose float64 pre-activation is this close to zero may be decided either way (test_warmstart_gpu)
SEED, TICK = 11, 3
SIGMA, CLIP = 0.5, 0.5
LEARNER_ARRAYS = ("actor", "actor_t", "critic", "critic_t", "critic2", "critic2_t", "m_actor", "v_actor", "m_critic", "v_critic", "m_critic2",
                  "v_critic2", "grad_actor", "grad_critic", "grad_critic2", "losses", "losses2")


def _T():
    return importlib.import_module(U.PKG_NAME + ".td3")


def _params(h, seed, boost, lift):
    """critic 2 from init_params(seed + 1000) with critic 1's head boost and b1 noise; the actor's b3 lifted to (1.5, -1.5) so that
    a~' reaches the clamp."""
    pa, pc = h["pa"].copy(), h["pc"].copy()
    pc2 = DO.init_params(seed + 1000, 11, 1, 1)
    pc2[128250:128750] *= boost
    pc2[2750:3000] = pc[2750:3000]
    if lift:
        pa[129000:129002] = (1.5, -1.5)
    return pa, pc, pc2


def _setup(batch=120, seed=SEED, boost=30.0, lift=True, sigma=SIGMA, clip=CLIP, delay=2, same_critics=False):
    torch, S, D, ag0, ring, h = TD._setup(seed=seed, boost=boost)
    T = _T()
    pa, pc, pc2 = _params(h, seed, boost, lift)
    if same_critics:
        pc2 = pc.copy()
    ag = T.TD3Agent(seed=seed, sigma_trg=sigma, clip_trg=clip, policy_delay=delay)
    ag.set_params(actor=pa, critic=pc, critic2=pc2)
    ag.set_norm(h["s_min"], h["s_max"])
    ag.batch = batch
    h = dict(h, pa=pa, pc=pc, pc2=pc2)
    return torch, S, D, T, ag, ring, h, ag0


def _minibatch(h, batch, seed=SEED, tick=TICK):
    idx = DO.sample_indices(seed, tick, batch, 24000)
    s, a, r, s2, done = (h[k][idx] for k in ("s", "a", "r", "s2", "done"))
    return s, a, r, s2, done.astype(bool)


_TWIN_CACHE = {}


def _twin_targets(h, batch):
    """(twin, its target stage) for the standard case at this batch; the stage arrays are computed once per batch and read only."""
    tw = TR.Twin(h["pa"], h["pc"], h["pc2"], h["s_min"], h["s_max"], SIGMA, CLIP)
    if batch not in _TWIN_CACHE:
        s, a, r, s2, done = _minibatch(h, batch)
        tg = tw.targets(r, s2, done, SEED, TICK)
        for v in tg.values():
            v.setflags(write=False)
        _TWIN_CACHE[batch] = tg
    return tw, _TWIN_CACHE[batch]


def _assert_coverage(tg, batch):
    """The case exercises what TD3 adds -- asserted on the twin before the device is looked at."""
    raw = np.float32(SIGMA) * tg["z"]
    clipped = int((np.abs(raw) > CLIP).sum())
    clamped = int((np.abs(tg["a_t"] + tg["eps"]) > 1).sum())
    pick1, pick2 = int((tg["q1"] <= tg["q2"]).sum()), int((tg["q2"] < tg["q1"]).sum())
    print(f"batch {batch}: clipped eps {clipped}, clamped a~' {clamped}, min picks {pick1} / {pick2}, "
          f"smallest |q'1 - q'2| {np.abs(tg['q1'] - tg['q2']).min():.2e}")
    # Batch 1 is the single column 0 of (SEED, TICK): its draw is what it is -- 0.5 z = (-0.244, -0.015), no clip, no clamp, one argmin -- so
    # the three conditions are asked of the batches that have the columns to meet them (17: 10 clipped, 12 clamped, 7 / 10).
    if batch >= 17:
        assert clipped >= 1 and clamped >= 1 and (np.abs(tg["a_smooth"]) == 1).any()
        assert pick1 >= 1 and pick2 >= 1


def _tied_units(p, x):
    _, (_, z1, _, z2, _, _) = DO.mlp_forward(p, x, 11, 1, False, keep=True, dtype=np.float64)
    out = []
    for z, off in ((z1, 11 * 250), (z2, 11 * 250 + 250 + 250 * 500)):
        for u in np.unique(np.where(np.abs(z) < TIE)[1]):
            col = z[:, u]
            out.append((off + int(u), float(np.sign(col[np.argmin(np.abs(col))]) or 1.0)))
    return out


def _assert_critic_blocks(g, learner, s, a, y, what, expect_ties=()):
    """Every block within BLOCK_TOL of float64; a block that fails on a tied relu is compared again with that unit decided the other
    way, and the list of such units is asserted exactly."""
    g64, _ = learner.critic_grad(s, a, y, dtype=np.float64)
    try:
        errs = TD._assert_blocks(g, g64, 11, 1, what)
        tied = []
    except AssertionError:
        x = np.concatenate([DO.normalize(s, learner.s_min, learner.s_max), a], 1)
        tied = _tied_units(learner.critic, x)
        if not tied or len(tied) > 3:
            raise
        keep = learner.critic
        flipped = keep.astype(np.float64)
        for i, sg in tied:
            flipped[i] -= sg * 4 * TIE
        learner.critic = flipped
        try:
            g64, _ = learner.critic_grad(s, a, y, dtype=np.float64)
        finally:
            learner.critic = keep
        errs = TD._assert_blocks(g, g64, 11, 1, what + " (tied relus decided the other way)")
    assert [i for i, _ in tied] == list(expect_ties), (what, tied)
    return errs


def _check_target_stage(ag, tw, tg, h, batch):
    """a~' against the twin; q'1, q'2 and y from the device's a~'.  Returns the device's y."""
    s, a, r, s2, done = _minibatch(h, batch)
    a_dev = ag.a_smooth.cpu().numpy()[:, :batch].T.copy()
    err_a = float(np.abs(a_dev - tg["a_smooth"]).max())
    print(f"batch {batch}: max |a~' - twin| = {err_a:.2e}")
    assert err_a <= 1e-5
    assert (np.abs(a_dev) <= 1).all() and (np.abs(a_dev) == 1).any() == (np.abs(tg["a_smooth"]) == 1).any()
    tg2 = tw.targets(r, s2, done, SEED, TICK, a_smooth=a_dev)
    y_dev = ag.y_target.cpu().numpy()[:batch].copy()
    np.testing.assert_allclose(ag.q_target1.cpu().numpy()[:batch], tg2["q1"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(ag.q_target2.cpu().numpy()[:batch], tg2["q2"], rtol=2e-5, atol=2e-5)
    print(f"batch {batch}: max |y - twin(a~' of the device)| = {np.abs(y_dev - tg2['y']).max():.2e}")
    np.testing.assert_allclose(y_dev, tg2["y"], rtol=2e-5, atol=2e-5)
    # the y critic 1's head left in the DDPG workspace is the same y (WS_Y, tests/test_ddpg_gpu.py)
    assert np.array_equal(ag.ws[128 * 22:128 * 23].cpu().numpy()[:batch], y_dev)
    return y_dev


def _check_critics(ag, tw, h, batch, y_dev, policy):
    """Gradients of both critics from the device's y; ADAM, moments and the soft update (or the untouched target) from the kernel's
    own gradient."""
    s, a, r, s2, done = _minibatch(h, batch)
    out = {}
    for name, learner, p0, suffix, loss in (("critic", tw.L, h["pc"], "", ag.losses[0].item()), ("critic2", tw.L2, h["pc2"], "2", ag.losses2[0].item())):
        g = getattr(ag, "grad_critic" + suffix).cpu().numpy()
        out[name] = _assert_critic_blocks(g, learner, s, a, y_dev, f"{name} gradient B={batch}")
        _, l_ref = learner.critic_grad(s, a, y_dev)
        assert abs(loss - l_ref) < 1e-4 * max(1.0, abs(l_ref)), (name, loss, l_ref)
        opt = DO.Adam(len(g), DO.ETA_CRIT)
        p1 = opt.step(p0, g)
        crit = getattr(ag, name).cpu().numpy()
        np.testing.assert_allclose(crit, p1, rtol=0, atol=1e-7)
        np.testing.assert_allclose(getattr(ag, "m_critic" + suffix).cpu().numpy(), opt.m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(getattr(ag, "v_critic" + suffix).cpu().numpy(), opt.v, rtol=1e-6, atol=1e-15)
        tgt = getattr(ag, name + "_t").cpu().numpy()
        if policy:
            np.testing.assert_allclose(tgt, DO.soft_update(p0, crit), rtol=0, atol=1e-7)
            assert not np.array_equal(tgt, p0)
        else:
            assert np.array_equal(tgt, p0), name + "_t moved off a policy step"
    print(f"batch {batch}: per-block critic gradient errors {out}")


@pytest.mark.parametrize("batch", [1, 17, 120, 128])
def test_policy_step_matches_the_twin_and_float64(batch):
    torch, S, D, T, ag, ring, h, _ = _setup(batch)
    tw, tg = _twin_targets(h, batch)
    _assert_coverage(tg, batch)
    assert (ag.sample_indices(TICK, len(ring)) == DO.sample_indices(SEED, TICK, batch, 24000)).all()
    ag.replay(ring, tick=TICK, update_policy=True)
    torch.cuda.synchronize()
    y_dev = _check_target_stage(ag, tw, tg, h, batch)
    _check_critics(ag, tw, h, batch, y_dev, policy=True)
    # the actor through the device's UPDATED critic 1 (DDPG.jl:137-140)
    s = _minibatch(h, batch)[0]
    L = tw.L
    L.critic = ag.critic.cpu().numpy()
    ga = ag.grad_actor.cpu().numpy()
    ga64, _ = L.actor_grad(s, dtype=np.float64)
    print(f"batch {batch}: per-block actor gradient errors", TD._assert_blocks(ga, ga64, 9, 2, f"actor gradient B={batch}"))
    _, la_ref = L.actor_grad(s)
    assert abs(ag.losses[1].item() - la_ref) < 1e-4 * max(1.0, abs(la_ref))
    opt_a = DO.Adam(len(ga), DO.ETA_ACT)
    pa1 = opt_a.step(h["pa"], ga)
    act = ag.actor.cpu().numpy()
    np.testing.assert_allclose(act, pa1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.actor_t.cpu().numpy(), DO.soft_update(h["pa"], act), rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.m_actor.cpu().numpy(), opt_a.m, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(ag.v_actor.cpu().numpy(), opt_a.v, rtol=1e-6, atol=1e-15)
    assert ag.updates == 1 and ag.bp_critic == [0.9 * 0.9, 0.999 * 0.999] and ag.bp_actor == [0.9 * 0.9, 0.999 * 0.999]


@pytest.mark.parametrize("batch", [17, 120])
def test_non_policy_step_moves_the_critics_and_nothing_else(batch):
    torch, S, D, T, ag, ring, h, _ = _setup(batch)
    tw, tg = _twin_targets(h, batch)
    _assert_coverage(tg, batch)
    ag.grad_actor.fill_(-3.0)
    ag.losses[1] = 42.0
    ag.m_actor.fill_(0.25)
    ag.v_actor.fill_(0.5)
    before = {k: getattr(ag, k).clone() for k in ("actor", "actor_t", "m_actor", "v_actor", "grad_actor", "losses")}
    ag.replay(ring, tick=TICK, update_policy=False)
    torch.cuda.synchronize()
    y_dev = _check_target_stage(ag, tw, tg, h, batch)
    _check_critics(ag, tw, h, batch, y_dev, policy=False)
    for k in ("actor", "actor_t", "m_actor", "v_actor", "grad_actor"):
        assert np.array_equal(U.bits32(getattr(ag, k).cpu().numpy()), U.bits32(before[k].cpu().numpy())), k
    assert U.bits32(ag.losses.cpu().numpy())[1] == U.bits32(before["losses"].cpu().numpy())[1]
    assert ag.updates == 1 and ag.bp_critic == [0.9 * 0.9, 0.999 * 0.999] and ag.bp_actor == [0.9, 0.999]


def test_schedule_and_beta_powers_over_four_updates():
    """d = 2: updates 1 and 3 (0-based) are policy steps.  Each critic step follows the oracle's ADAM from the kernel's own previous
    parameters with the powers advanced every update; the actor's with its powers advanced on policy steps only."""
    torch, S, D, T, ag, ring, h, _ = _setup(120, seed=5, delay=2)
    opt_c, opt_c2, opt_a = DO.Adam(D.N_CRITIC, DO.ETA_CRIT), DO.Adam(D.N_CRITIC, DO.ETA_CRIT), DO.Adam(D.N_ACTOR, DO.ETA_ACT)
    pc, pc2, pa = h["pc"].copy(), h["pc2"].copy(), h["pa"].copy()
    moved = []
    for t in range(4):
        a_before = ag.actor.clone()
        ag.replay(ring, tick=t)
        pc = opt_c.step(pc, ag.grad_critic.cpu().numpy())
        pc2 = opt_c2.step(pc2, ag.grad_critic2.cpu().numpy())
        crit, crit2 = ag.critic.cpu().numpy(), ag.critic2.cpu().numpy()
        np.testing.assert_allclose(crit, pc, rtol=0, atol=2e-7)
        np.testing.assert_allclose(crit2, pc2, rtol=0, atol=2e-7)
        pc, pc2 = crit, crit2
        moved.append(not torch.equal(a_before, ag.actor))
        if T.is_policy_step(t, 2):
            pa = opt_a.step(pa, ag.grad_actor.cpu().numpy())
            act = ag.actor.cpu().numpy()
            np.testing.assert_allclose(act, pa, rtol=0, atol=2e-7)
            pa = act
    assert moved == [False, True, False, True]
    assert ag.updates == 4 and abs(ag.bp_critic[0] - 0.9 ** 5) < 1e-15 and abs(ag.bp_critic[1] - 0.999 ** 5) < 1e-15
    assert abs(ag.bp_actor[0] - 0.9 ** 3) < 1e-15 and abs(ag.bp_actor[1] - 0.999 ** 3) < 1e-15
    assert abs(opt_a.bp[0] - ag.bp_actor[0]) < 1e-15 and abs(opt_c.bp[0] - ag.bp_critic[0]) < 1e-15


def test_td3_degenerates_to_ddpg_bit_for_bit():
    """sigma_trg = 0, critic 2 and its target byte copies of critic 1's, d = 1, three updates: every array Agent.replay leaves, and
    critic 2's equal critic 1's.  Pins the summation orders of the new launches to the existing ones."""
    torch, S, D, T, ag, ring, h, ag0 = _setup(120, seed=17, lift=False, sigma=0.0, delay=1, same_critics=True)
    ag0.set_params(actor=h["pa"], critic=h["pc"])
    assert torch.equal(ag.critic2, ag.critic) and torch.equal(ag.critic2_t, ag.critic_t)
    for t in range(3):
        ag0.replay(ring, tick=t)
        ag.replay(ring, tick=t)
    torch.cuda.synchronize()
    for k in ("actor", "actor_t", "critic", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic", "losses"):
        assert torch.equal(getattr(ag, k), getattr(ag0, k)), k
    for k in ("critic", "critic_t", "m_critic", "v_critic", "grad_critic"):
        assert torch.equal(getattr(ag, k.replace("critic", "critic2")), getattr(ag, k)), k
    assert torch.equal(ag.losses2, ag.losses[:1])
    assert ag.updates == ag0.updates == 3 and ag.bp_actor == ag0.bp_actor and ag.bp_critic == ag0.bp_critic
    assert float(ag.grad_critic[:3000].abs().max()) > 0 and float(ag.grad_actor[:2500].abs().max()) > 0


def test_two_runs_leave_the_same_bytes():
    out = []
    for _ in range(2):
        torch, S, D, T, ag, ring, h, _ = _setup(120, delay=2)
        for t in range(3):
            ag.replay(ring, tick=t)
        torch.cuda.synchronize()
        out.append(dict({k: getattr(ag, k).cpu().numpy() for k in LEARNER_ARRAYS}, ws2=ag.ws2[:5 * 128].cpu().numpy()))
    for k in out[0]:
        assert np.array_equal(U.bits32(out[0][k]), U.bits32(out[1][k])), k


def test_training_on_a_fixed_ring_reduces_both_critic_losses():
    torch, S, D, T, ag, ring, h, _ = _setup(120, seed=2, boost=1.0, lift=False, sigma=0.2, clip=0.5, delay=2)
    r = (0.4 * (h["s"][:, 4] - h["s"][:, 3]) + h["a"][:, 1] - 0.5 * h["s"][:, 0]).astype(np.float32)
    ring.r.copy_(torch.from_numpy(r))
    first, last = np.zeros(2), np.zeros(2)
    n_up = 160
    for t in range(n_up):
        ag.replay(ring, tick=t % 4)
        if t < 4 or t >= n_up - 4:
            l = np.array([ag.losses[0].item(), ag.losses2[0].item()]) / 4
            if t < 4:
                first += l
            else:
                last += l
    print("critic losses, first and last four updates:", first, last)
    assert np.isfinite(last).all() and (last < 0.5 * first).all(), (first, last)
    assert ag.updates == n_up
    for k in LEARNER_ARRAYS:
        assert torch.isfinite(getattr(ag, k)).all(), k


def test_c_abi_refusals():
    torch, S, D, T, ag, ring, h, ag0 = _setup(120)
    rs = ring.struct()
    snap = {k: getattr(ag, k).clone() for k in LEARNER_ARRAYS}

    def call(a, policy=1):
        return ag.L.shems_td3_update(C.byref(a), C.byref(rs), len(ring), SEED, TICK, ag.eta_crit, 0.9, 0.999, ag.eta_act, 0.9, 0.999, policy, ag._stream())

    def args(**kw):
        a = ag._td3_args()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    a = args()
    a.d.batch = 129
    assert call(a) == S._capi.ERR_ARG
    for bad in (-0.1, float("nan"), float("inf")):
        assert call(args(sigma_trg=bad)) == S._capi.ERR_ARG and call(args(clip_trg=bad)) == S._capi.ERR_ARG
    assert call(args(critic2=ag.critic.data_ptr())) == S._capi.ERR_ARG
    assert call(args(critic2_t=ag.critic_t.data_ptr())) == S._capi.ERR_ARG
    assert call(args(m_critic2=ag.m_critic.data_ptr())) == S._capi.ERR_ARG
    assert call(args(grad_critic2=ag.grad_critic.data_ptr() + 4 * 1000)) == S._capi.ERR_ARG
    assert call(args(critic2=None)) == S._capi.ERR_ARG and call(args(ws2=None)) == S._capi.ERR_ARG
    assert call(args(critic2=ag.critic2.data_ptr() + 4)) == S._capi.ERR_ARG          # misaligned
    assert call(args(), policy=2) == S._capi.ERR_ARG and call(args(), policy=-1) == S._capi.ERR_ARG
    assert "update_policy" in ag.L.shems_last_error().decode()
    # a learner whose layer-2 state lives in the tiled regions: every Flux-order entry point answers SHEMS_ERR_STATE
    ag0.use_tiled(True)
    ag0.replay(ring, tick=0)
    assert ag0._tiled_current
    a = args()
    a.d = ag0._ddpg_args(raw=True)
    assert call(a) == S._capi.ERR_STATE
    ag0.use_tiled(False)
    torch.cuda.synchronize()
    for k in LEARNER_ARRAYS:                                   # nothing was launched on this learner
        assert torch.equal(getattr(ag, k), snap[k]), k
    assert call(args()) == S._capi.OK                          # and the unmodified record runs
    torch.cuda.synchronize()


def test_python_refusals_name_their_reason():
    torch, S, D, T, ag, ring, h, _ = _setup(120)
    for kw, word in ((dict(hidden=(300, 600)), "hidden sizes"), (dict(wide=True), "hidden sizes"), (dict(noise_type="pn"), "parameter noise"),
                     (dict(tensors={}), "learner group")):
        with pytest.raises(NotImplementedError, match=word):
            T.TD3Agent(seed=1, **kw)
    ag.batch = 129
    with pytest.raises(NotImplementedError, match="BATCH_SIZE = 129"):
        ag.replay(ring)
    ag.batch = 120
    with pytest.raises(NotImplementedError, match="data-parallel"):
        ag.enable_data_parallel(None)
    with pytest.raises(NotImplementedError, match="tiled"):
        ag.use_tiled(True)
    with pytest.raises(NotImplementedError, match="evaluate"):
        ag.evaluate(ring)
    ag._before_param_write = lambda: None
    with pytest.raises(NotImplementedError, match="learner group"):
        ag.replay(ring)
    del ag._before_param_write
    with pytest.raises(NotImplementedError, match="pipelined"):
        ag.replay(ring, exclude=(0, 10))
    assert ag.updates == 0
    # snapshot / restore cover the second critic; set_params(critic2=...) checks the size
    snap = ag.snapshot()
    ag.replay(ring, tick=0)
    ag.replay(ring, tick=1)
    assert not torch.equal(ag.critic2, snap[0]["critic2"]) and ag.updates == 2
    ag.restore(snap)
    assert ag.updates == 0 and ag.bp_critic == [0.9, 0.999]
    for k in LEARNER_ARRAYS:
        assert torch.equal(getattr(ag, k), snap[0][k]), k
    with pytest.raises(ValueError, match="critic2"):
        ag.set_params(critic2=np.zeros(7, np.float32))


def test_training_loop_runs_td3():
    """TD3Agent.episode_ / run_episodes are the Agent's: two episodes of 72 steps on 256 envs make 144 updates, 72 of them policy steps."""
    torch = pytest.importorskip("torch")
    S, T = U.pkg(), _T()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    tab = S.tables.synthetic_table("train", 98)
    mk = lambda n: S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    env, env_eval = mk(256), mk(100)
    ag = T.TD3Agent(seed=1231)
    ring = D.ReplayRing(24000)
    ag.populate_memory(env, ring)
    ag.min_max_buffer(ring)
    for ep in (1, 2):
        ret = ag.episode_(env, ring, train=True, rng_ep=7, episode=ep)
        assert ret.shape == (256,) and torch.isfinite(ret).all()
    assert ag.updates == 144 and abs(ag.bp_critic[0] - 0.9 ** 145) < 1e-12 and abs(ag.bp_actor[0] - 0.9 ** 73) < 1e-12
    for k in LEARNER_ARRAYS:
        assert torch.isfinite(getattr(ag, k)).all(), k
    total, score, best_run, best_actor = ag.run_episodes(env, env_eval, ring, 2, test_every=100, test_runs=100)
    assert total.shape == (2,) and np.isfinite(total).all() and best_run == 1
    assert best_actor is not None and best_actor.shape == (D.N_ACTOR,) and np.isfinite(best_actor).all()
    assert ag.updates == 288


def test_entry_script_trains_td3_under_a_case_of_its_own(tmp_path):
    """SHEMS_ALGO=td3 writes its files under the suffixed case.  With the variable unset the case and every file name are DDPG's: the
    run itself is tests/test_main_entry.py's, unchanged; here the case string is compared."""
    pytest.importorskip("torch")
    M = importlib.import_module(U.PKG_NAME + ".main")
    base = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
            "SHEMS_SYNTHETIC_DATA": "1"}
    ddpg_case = M.config_from_env(base).case
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_ALGO"):            # refused by name before any device work or file
        M.main(dict(base, SHEMS_ALGO="td4"), cwd=str(tmp_path / "nowhere"), log=lambda *_: None)
    assert os.getcwd() == cwd0 and not (tmp_path / "nowhere").exists()
    try:
        cfg, written = M.main(dict(base, SHEMS_ALGO="td3:2:0.2"), cwd=str(tmp_path), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    assert cfg.case == ddpg_case + "_td3-d2-s0.2-c0.5"
    stem = f"DDPG_Shems_Charger_v1_72_2_250_500_{cfg.case}_1231"
    for f in (f"out/bson/{stem}_actor_2.bson", f"out/bson/{stem}_scores_2.bson", f"out/bson/temp/{stem}_actor_1.bson"):
        assert (tmp_path / f).exists(), f
    assert len(written) == 2 and all(cfg.case in w for w in written)
    assert not [p for p in (tmp_path / "out").rglob("*") if p.is_file() and p.suffix in (".bson", ".csv") and "results" in p.name and "_td3-" not in p.name]
    assert M.config_from_env(base).case == ddpg_case and "td3" not in ddpg_case and M.algo_from_env(base) == ("ddpg", None)

"""GPU tests of the behaviour-regularised actor update (shems_ddpg_update_bc / shems_td3_update_bc, ddpg.BC) against the NumPy twin
(tests/bc_ref.py) in float64.

Every case is one learner on the ring of tests/test_ddpg_gpu.py:_setup (24 000 slots), seed 11, tick 3, for both learners (ddpg.Agent,
td3.TD3Agent on a policy step).  Each stage is checked from the device's own previous stage: q_m through the device's a_pi and updated
critic, rtol = atol = 2e-5 (the bound y has); Qbar and lambda from the device's q_m, rtol 1e-5 (the fp32 bound (n - 1) 2^-24 for 128
non-negative terms in any order, and one division); every actor gradient block BLOCK_TOL = 2e-6 of its float64 max-abs, evaluated with
the device's lambda; ADAM and the soft update from the kernel's own gradient atol 1e-7, moments rtol 1e-6; the losses 1e-4 max(1, |ref|).

The critics' output bias is lifted by Q_LIFT = 0.1 (targets too).  The critic's own ADAM step of this update moves every q_m by about
-0.1, so that through the UPDATED critic of _setup's parameters all q_m are negative (-0.16 .. -0.07 on the CPU oracle, Qbar = |mean q| =
0.11): the case would not tell mean|q| from |mean q|.  With the lift the oracle gives, for 17 / 120 / 128 columns, 10 / 84 / 91 negative
q_m, Qbar = 0.018 .. 0.021 against |mean q| = 0.009 .. 0.014 and term max-abs ratios of 10 .. 12 -- both learners alike; a bias moves no
gradient path.  _assert_coverage asserts the conditions on the twin with the device's updated critic."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bc_ref as BR
import ddpg_oracle as DO
import test_ddpg_gpu as TD
import test_td3_gpu as T3
import util as U

pytestmark = pytest.mark.gpu

BLOCK_TOL = TD.BLOCK_TOL
TIE = T3.TIE
SEED, TICK = 11, 3
BATCHES = [1, 17, 120, 128]
WS_AT, WS_API, WS_D3A = 18 * 128, 24 * 128, 28 * 128       # csrc/shems_ddpg.hip: the stored actions, a_pi, the error at the actor's output
Q_LIFT = 0.1
AGENT_ARRAYS = ("actor", "actor_t", "critic", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic", "losses")


def _setup(learner, batch, bc, seed=SEED):
    """(torch, S, D, agent, ring, host arrays) -- a ddpg.Agent or a td3.TD3Agent (its b3 not lifted: a_pi stays off the clamp)."""
    if learner == "ddpg":
        torch, S, D, ag, ring, h = TD._setup(seed=seed)
    else:
        torch, S, D, _, ag, ring, h, _ = T3._setup(batch, seed=seed, lift=False)
    pc = h["pc"].copy()
    pc[-1] += Q_LIFT                                           # b3 of the critic (of both critics); sync_targets lifts the targets
    if learner == "ddpg":
        ag.set_params(critic=pc)
        h = dict(h, pc=pc)
    else:
        pc2 = h["pc2"].copy()
        pc2[-1] += Q_LIFT
        ag.set_params(critic=pc, critic2=pc2)
        h = dict(h, pc=pc, pc2=pc2)
    ag.batch = batch
    ag.bc = bc
    return torch, S, D, ag, ring, h


def _update(ag, ring, tick=TICK, policy=True):
    if hasattr(ag, "critic2"):
        ag.replay(ring, tick=tick, update_policy=policy)
    else:
        ag.replay(ring, tick=tick)


def _minibatch(h, batch, tick=TICK, seed=SEED):
    idx = DO.sample_indices(seed, tick, batch, 24000)
    return h["s"][idx], h["a"][idx]


def _tied(p, x, in_dim, out_dim):
    _, (_, z1, _, z2, _, _) = DO.mlp_forward(p, x, in_dim, out_dim, out_dim == 2, keep=True, dtype=np.float64)
    out = []
    for z, off in ((z1, in_dim * 250), (z2, in_dim * 250 + 250 + 250 * 500)):
        for u in np.unique(np.where(np.abs(z) < TIE)[1]):
            col = z[:, u]
            out.append((off + int(u), float(np.sign(col[np.argmin(np.abs(col))]) or 1.0)))
    return out


def _assert_actor_blocks(g, L, s, a, lam, weight, what):
    """Every block within BLOCK_TOL of float64.  The project's tied-relu rule: a block that fails while a relu of the actor or of the
    critic has a float64 pre-activation within TIE of zero is compared again with those units (at most 3) decided the other way."""
    g64 = BR.actor_grad(L, s, a, lam, weight)[0]
    try:
        return TD._assert_blocks(g, g64, 9, 2, what)
    except AssertionError:
        sn = DO.normalize(s, L.s_min, L.s_max)
        a_pi = DO.mlp_forward(L.actor, sn, 9, 2, True, dtype=np.float64)
        ta, tc = _tied(L.actor, sn, 9, 2), _tied(L.critic, np.concatenate([sn.astype(np.float64), a_pi], 1), 11, 1)
        if not (ta or tc) or len(ta) + len(tc) > 3:
            raise
        keep = L.actor, L.critic
        fa, fc = L.actor.astype(np.float64), L.critic.astype(np.float64)
        for i, sg in ta:
            fa[i] -= sg * 4 * TIE
        for i, sg in tc:
            fc[i] -= sg * 4 * TIE
        L.actor, L.critic = fa, fc
        try:
            g64 = BR.actor_grad(L, s, a, lam, weight)[0]
        finally:
            L.actor, L.critic = keep
        print(what, "tied relus decided the other way:", ta, tc)
        return TD._assert_blocks(g, g64, 9, 2, what + " (tied relus decided the other way)")


def _assert_coverage(L, s, a, batch, bc):
    """The case exercises what the term adds -- asserted on the twin, with the device's updated critic, before the record is read."""
    a_pi, q, da, _ = BR.actor_parts(L, s, a)
    qbar = float(BR.q_abs_mean(q))
    lam = bc.alpha / max(qbar, 1e-8) if bc.normalise else bc.alpha
    t_q, t_bc = lam * da, bc.weight * (a_pi - a) / batch
    ratio = float(np.abs(t_q).max() / max(np.abs(t_bc).max(), 1e-300))
    print(f"batch {batch}: Qbar {qbar:.4g}, |mean q| {abs(float(q.mean())):.4g}, negative q {int((q < 0).sum())} of {batch}, lambda {lam:.4g}, "
          f"term max-abs ratio {ratio:.3g}")
    if batch >= 17:
        assert (q < 0).any() and (q > 0).any() and qbar != abs(float(q.mean()))
        assert qbar > 1e-3
        assert 0.01 <= ratio <= 100.0


@pytest.mark.parametrize("learner", ["ddpg", "td3"])
@pytest.mark.parametrize("batch", BATCHES)
def test_update_matches_float64_stage_by_stage(learner, batch):
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    bc = D.BC(2.5, 1.0, True)
    torch, S, D, ag, ring, h = _setup(learner, batch, bc)
    s, a = _minibatch(h, batch)
    _update(ag, ring)
    torch.cuda.synchronize()
    L = DO.Learner(h["pa"], h["pc"], h["s_min"], h["s_max"])
    L.critic = ag.critic.cpu().numpy()                        # the critic as updated by this same update (critic 1 for TD3)
    _assert_coverage(L, s, a, batch, bc)
    ws = ag.ws.cpu().numpy()
    out = ag.bc_out.cpu().numpy()
    assert np.array_equal(ws[WS_AT:WS_AT + 256].reshape(2, 128)[:, :batch].T, a)
    # q_m through the device's a_pi and the updated critic
    a_dev = ws[WS_API:WS_API + 256].reshape(2, 128)[:, :batch].T.astype(np.float64)
    sn = DO.normalize(s, L.s_min, L.s_max).astype(np.float64)
    q64 = DO.mlp_forward(L.critic, np.concatenate([sn, a_dev], 1), 11, 1, False, dtype=np.float64)[:, 0]
    q_dev = out[4:4 + batch]
    print(f"{learner} batch {batch}: max |q - float64| = {np.abs(q_dev - q64).max():.2e}")
    np.testing.assert_allclose(q_dev, q64, rtol=2e-5, atol=2e-5)
    assert np.array_equal(ag.bc_q.cpu().numpy(), out[4:])
    # Qbar and lambda from the device's q_m
    qbar_ref = float(np.abs(q_dev.astype(np.float64)).sum() / batch)
    lam_ref = 2.5 / max(qbar_ref, 1e-8)
    print(f"{learner} batch {batch}: Qbar {out[1]:.6g} (ref {qbar_ref:.6g}), lambda {out[0]:.6g} (ref {lam_ref:.6g})")
    np.testing.assert_allclose(out[1], qbar_ref, rtol=1e-5, atol=0)
    np.testing.assert_allclose(out[0], lam_ref, rtol=1e-5, atol=0)
    assert ag.bc_lambda.item() == out[0] and ag.bc_q_abs_mean.item() == out[1] and ag.bc_mse.item() == out[3]
    # every actor gradient block, evaluated with the device's lambda
    lam_dev = float(out[0])
    ga = ag.grad_actor.cpu().numpy()
    print(f"{learner} batch {batch}: per-block actor gradient errors", _assert_actor_blocks(ga, L, s, a, lam_dev, 1.0, f"{learner} actor gradient B={batch}"))
    d3 = ws[WS_D3A:WS_D3A + 256].reshape(2, 128)
    assert not d3[:, batch:].any(), "pad columns reached d3"
    # ADAM and the soft update from the kernel's own gradient
    opt_a = DO.Adam(len(ga), DO.ETA_ACT)
    pa1 = opt_a.step(h["pa"], ga)
    act = ag.actor.cpu().numpy()
    np.testing.assert_allclose(act, pa1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.actor_t.cpu().numpy(), DO.soft_update(h["pa"], act), rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.m_actor.cpu().numpy(), opt_a.m, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(ag.v_actor.cpu().numpy(), opt_a.v, rtol=1e-6, atol=1e-15)
    # the losses
    _, loss_ref, _, nmq_ref, mse_ref = BR.actor_grad(L, s, a, lam_dev, 1.0)
    print(f"{learner} batch {batch}: loss_act {ag.losses[1].item():.6g} (ref {loss_ref:.6g}), -mean q {out[2]:.6g} ({nmq_ref:.6g}), mse {out[3]:.6g} ({mse_ref:.6g})")
    for got, ref in ((ag.losses[1].item(), loss_ref), (out[2], nmq_ref), (out[3], mse_ref)):
        assert abs(got - ref) <= 1e-4 * max(1.0, abs(ref)), (got, ref)
    assert ag.updates == 1 and ag.bp_actor == [0.9 * 0.9, 0.999 * 0.999]


@pytest.mark.parametrize("learner", ["ddpg", "td3"])
def test_unit_lambda_and_no_pull_leaves_the_plain_update_bit_for_bit(learner):
    """normalise = 0, alpha = 1, weight = 0: three updates leave Agent.replay's (TD3Agent.replay's, over non-policy and policy steps)
    bytes in every learner array and in the losses.  Pins the summation orders and the contraction of the new head to head_actor's."""
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    torch, S, D, ag, ring, h = _setup(learner, 120, D.BC(1.0, 0.0, False), seed=17)
    _, _, _, ag0, ring0, _ = _setup(learner, 120, None, seed=17)
    arrays = T3.LEARNER_ARRAYS if learner == "td3" else AGENT_ARRAYS
    policies = []
    for t in range(3):
        policies.append(learner == "ddpg" or T3._T().is_policy_step(ag.updates, ag.policy_delay))
        ag0.replay(ring0, tick=t)
        ag.replay(ring, tick=t)
    torch.cuda.synchronize()
    assert policies == ([True] * 3 if learner == "ddpg" else [False, True, False])
    for k in arrays:
        assert np.array_equal(U.bits32(getattr(ag, k).cpu().numpy()), U.bits32(getattr(ag0, k).cpu().numpy())), k
    assert float(ag.grad_actor[:2500].abs().max()) > 0 and ag.bc_lambda.item() == 1.0
    assert ag.updates == ag0.updates == 3 and ag.bp_actor == ag0.bp_actor and ag.bp_critic == ag0.bp_critic


@pytest.mark.parametrize("batch", [17, 120])
def test_zero_alpha_is_the_cloning_gradient(batch):
    """alpha = 0, weight = 1: lambda is 0 whatever Qbar is, and the actor's gradient blocks meet the float64 cloning gradient
    d mse(a_pi, a) / d theta at BLOCK_TOL."""
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    torch, S, D, ag, ring, h = _setup("ddpg", batch, D.BC(0.0, 1.0, True))
    s, a = _minibatch(h, batch)
    _update(ag, ring)
    torch.cuda.synchronize()
    out = ag.bc_out.cpu().numpy()
    assert out[0] == 0.0 and out[1] > 1e-3
    L = DO.Learner(h["pa"], h["pc"], h["s_min"], h["s_max"])
    sn = DO.normalize(s, L.s_min, L.s_max)
    a_pi, ca = DO.mlp_forward(L.actor, sn, 9, 2, True, keep=True, dtype=np.float64)
    g64, _ = DO.mlp_backward(L.actor, ca, (a_pi - a) / batch, 9, 2, True, dtype=np.float64)
    print(f"batch {batch}: per-block errors against the cloning gradient", TD._assert_blocks(ag.grad_actor.cpu().numpy(), g64, 9, 2, f"cloning gradient B={batch}"))
    mse = float(np.mean((a_pi - a) ** 2))
    assert abs(ag.losses[1].item() - mse) <= 1e-4 * max(1.0, mse) and abs(out[3] - mse) <= 1e-4 * max(1.0, mse)


@pytest.mark.parametrize("learner", ["ddpg", "td3"])
def test_two_runs_leave_the_same_bytes(learner):
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    runs = []
    for _ in range(2):
        torch, S, D, ag, ring, h = _setup(learner, 120, D.BC())
        for t in range(3):
            ag.replay(ring, tick=t)
        torch.cuda.synchronize()
        arrays = T3.LEARNER_ARRAYS if learner == "td3" else AGENT_ARRAYS
        runs.append(dict({k: getattr(ag, k).cpu().numpy() for k in arrays}, out=ag.bc_out.cpu().numpy()))
    for k in runs[0]:
        assert np.array_equal(U.bits32(runs[0][k]), U.bits32(runs[1][k])), k
    assert runs[0]["out"][0] > 0 and runs[0]["out"][3] > 0


def test_off_a_td3_policy_step_the_record_and_the_actor_keep_their_bytes():
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    torch, S, D, ag, ring, h = _setup("td3", 120, D.BC())
    ag.bc_out.fill_(-7.0)
    ag.grad_actor.fill_(-3.0)
    ag.losses[1] = 42.0
    before = {k: getattr(ag, k).clone() for k in ("actor", "actor_t", "m_actor", "v_actor", "grad_actor", "losses", "bc_out")}
    c0 = ag.critic.clone()
    _update(ag, ring, policy=False)
    torch.cuda.synchronize()
    for k in ("actor", "actor_t", "m_actor", "v_actor", "grad_actor", "bc_out"):
        assert np.array_equal(U.bits32(getattr(ag, k).cpu().numpy()), U.bits32(before[k].cpu().numpy())), k
    assert ag.losses[1].item() == 42.0 and not torch.equal(ag.critic, c0)
    assert ag.updates == 1 and ag.bp_actor == [0.9, 0.999]


def test_c_abi_refusals_launch_nothing():
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    torch, S, D, ag, ring, h = _setup("ddpg", 120, D.BC())
    _, _, _, t3, ring3, _ = _setup("td3", 120, D.BC())
    L = S._capi.declare_bc()
    ERR_ARG, ERR_STATE = S._capi.ERR_ARG, S._capi.ERR_STATE
    rs, rs3 = ring.struct(), ring3.struct()
    for x in (ag, t3):
        x.bc_out.fill_(-7.0)
    snap = {k: getattr(ag, k).clone() for k in AGENT_ARRAYS + ("ws", "bc_out")}
    snap3 = {k: getattr(t3, k).clone() for k in T3.LEARNER_ARRAYS + ("ws", "ws2", "bc_out")}

    def rec(x, **kw):
        b = x.bc.struct(x.bc_out.data_ptr())
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(b, d=None):
        d = ag._ddpg_args() if d is None else d
        return L.shems_ddpg_update_bc(C.byref(d), C.byref(rs), len(ring), SEED, TICK, 0, 0, ag.eta_crit, 0.9, 0.999, ag.eta_act, 0.9, 0.999, None,
                                      C.byref(b) if b is not None else None, ag._stream())

    def call3(b, policy=1):
        a = t3._td3_args()
        return L.shems_td3_update_bc(C.byref(a), C.byref(rs3), len(ring3), SEED, TICK, t3.eta_crit, 0.9, 0.999, t3.eta_act, 0.9, 0.999, policy,
                                     C.byref(b) if b is not None else None, t3._stream())

    for fn, x in ((call, ag), (call3, t3)):
        assert fn(None) == ERR_ARG and fn(rec(x, out=None)) == ERR_ARG
        assert fn(rec(x, out=x.bc_out.data_ptr() + 4)) == ERR_ARG                         # misaligned
        for ptr in (x.ws.data_ptr(), x.ws.data_ptr() + 16 * 1000, x.losses.data_ptr(), x.actor.data_ptr(), x.critic_t.data_ptr() + 16 * 50,
                    x.m_critic.data_ptr(), x.grad_actor.data_ptr()):
            assert fn(rec(x, out=ptr)) == ERR_ARG
        assert "overlaps" in L.shems_last_error().decode()
        for bad in (-0.1, float("nan"), float("inf")):
            assert fn(rec(x, alpha=bad)) == ERR_ARG and fn(rec(x, weight=bad)) == ERR_ARG
        assert fn(rec(x, normalise=2)) == ERR_ARG and fn(rec(x, normalise=-1)) == ERR_ARG
        assert fn(rec(x, reserved=1)) == ERR_ARG
    assert call3(rec(t3, out=t3.ws2.data_ptr())) == ERR_ARG and call3(rec(t3, out=t3.critic2.data_ptr())) == ERR_ARG
    assert call3(rec(t3, alpha=-1.0), policy=0) == ERR_ARG                                # checked off a policy step too
    # whatever the plain entry points refuse
    d = ag._ddpg_args()
    d.batch = 129
    assert call(rec(ag), d) == ERR_ARG
    assert call3(rec(t3), policy=2) == ERR_ARG
    # a learner on the tiled layout: there is no tiled behaviour-regularised gradient launch
    _, _, _, ag0, ring0, _ = _setup("ddpg", 120, None)
    ag0.use_tiled(True)
    ag0.replay(ring0, tick=0)
    assert ag0._tiled_current
    assert call(rec(ag), ag0._ddpg_args(raw=True)) == ERR_STATE
    ag0.use_tiled(False)
    torch.cuda.synchronize()
    for k, v in snap.items():                                  # nothing was launched: every array and the record under its sentinel
        assert torch.equal(getattr(ag, k), v), k
    for k, v in snap3.items():
        assert torch.equal(getattr(t3, k), v), k
    assert call(rec(ag)) == S._capi.OK and call3(rec(t3)) == S._capi.OK              # and the unmodified records run
    torch.cuda.synchronize()
    assert ag.bc_out[0].item() > 0 and t3.bc_out[0].item() > 0


def test_python_refusals_name_their_reason_and_never_run_without_the_term():
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    torch, S, D, ag, ring, h = _setup("ddpg", 120, D.BC())
    with pytest.raises(ValueError, match="not a ddpg.BC"):
        ag.bc = (2.5, 1.0)
    pr = D.PrioritizedRing(64)
    with pytest.raises(NotImplementedError, match="PrioritizedRing"):
        ag.replay(pr)
    ag.batch = 129
    with pytest.raises(NotImplementedError, match="BATCH_SIZE = 129"):
        ag.replay(ring)
    ag.batch = 120
    for attr, val, word in (("noise_type", "pn", "parameter noise"), ("fused", False, "split form"), ("wide", True, "wide network")):
        old = getattr(ag, attr)
        setattr(ag, attr, val)
        with pytest.raises(NotImplementedError, match=word):
            ag.replay(ring)
        setattr(ag, attr, old)
    ag.sync.world = 2
    with pytest.raises(NotImplementedError, match="data-parallel"):
        ag.replay(ring)
    ag.sync.world = 1
    ag.use_tiled(True)
    with pytest.raises(NotImplementedError, match="tiled"):
        ag.replay(ring)
    ag.use_tiled(False)
    ag._before_param_write = lambda: None
    with pytest.raises(NotImplementedError, match="learner group"):
        ag.replay(ring)
    del ag._before_param_write
    with pytest.raises(NotImplementedError, match="replay_given"):
        ag.replay_given(ring, None, None)
    assert ag.updates == 0
    _, _, _, t3, ring3, _ = _setup("td3", 120, D.BC())
    with pytest.raises(NotImplementedError, match="pipelined"):
        t3.replay(ring3, exclude=(0, 10))
    with pytest.raises(NotImplementedError, match="PrioritizedRing"):
        t3.replay(pr)
    assert t3.updates == 0
    # snapshot / restore carry bc; a decayed weight is the caller's one line
    snap = ag.snapshot()
    ag.bc = D.BC(2.5, 0.5)
    ag.replay(ring, tick=0)
    assert ag.updates == 1 and ag.bc.weight == 0.5
    ag.restore(snap)
    assert ag.bc == D.BC() and ag.updates == 0
    ag.bc = None
    ag.replay(ring, tick=0)                                    # bc = None: the plain update
    assert ag.updates == 1


def test_offline_training_on_a_foresight_pass_pulls_the_actor_to_the_data():
    """200 updates of imitation.offline on the "td" ring of one synthetic foresight pass: every array stays finite, mse(a_pi, a) falls
    (every update draws its own 24 columns of the 29 slots, so the first ten recorded values are compared with the last ten), and every
    recorded lambda is alpha / max(Qbar, 1e-8) of that update's Qbar (one fp32 division: within 4 units of the last place).
    alpha = 0.025, a hundredth of the paper's: the agent's critic is untrained, and under the normalisation an untrained critic's term
    at the actor's output is about ten times the pull's at alpha = 2.5 (the twin's ratios, _assert_coverage), so there the critic decides
    the sign of ADAM's step and the mse rises (measured: 0.85 -> 1.73); at a hundredth the pull is ten times the critic's term, which
    is the regime the assertion is about.  Everything else is the agent's default."""
    import test_imitation_gpu as TI
    S, F, I, D, H = TI._mods()
    import torch
    c = TI._s1()
    ring = D.ReplayRing(c["T"] - 1)
    assert I.transitions(c["val"], c["res"][0], ring, mode="td") is None and len(ring) == c["T"] - 1 and not ring.done.any()
    ag = D.Agent(seed=5, bc=D.BC(alpha=0.025))
    ag.batch = 24
    ag.min_max_buffer(ring, len(ring), seed=5)
    qbars = []
    plain = ag.replay

    def recording(r):
        plain(r)
        qbars.append(ag.bc_q_abs_mean.clone())

    ag.replay = recording
    rows = I.offline(ag, ring, 200, record_every=1)
    del ag.replay
    torch.cuda.synchronize()
    assert len(rows) == 200 and [r[0] for r in rows] == list(range(200)) and ag.updates == 200
    assert np.isfinite(np.array(rows)).all()
    for k in AGENT_ARRAYS + ("bc_out",):
        assert torch.isfinite(getattr(ag, k)).all(), k
    print(f"offline: mse {rows[0][4]:.4g} -> {rows[-1][4]:.4g}, lambda {rows[0][3]:.4g} -> {rows[-1][3]:.4g}, actor loss {rows[0][2]:.4g} -> {rows[-1][2]:.4g}")
    first, last = float(np.mean([r[4] for r in rows[:10]])), float(np.mean([r[4] for r in rows[-10:]]))
    print(f"offline: mean mse of the first ten updates {first:.4g}, of the last ten {last:.4g}")
    assert last < first
    qb = torch.cat(qbars).cpu().numpy()
    lam = np.array([BR.lam(0.025, q, True) for q in qb], np.float32)
    np.testing.assert_allclose(np.array([r[3] for r in rows], np.float32), lam, rtol=4 * 2.0 ** -23, atol=0)
    assert rows[-1][1] == ag.losses[0].item() and rows[-1][2] == ag.losses[1].item()
    rows2 = I.offline(ag, ring, 25, record_every=10)
    assert [r[0] for r in rows2] == [0, 10, 20, 24]
    mc = D.ReplayRing(c["T"])
    I.transitions(c["val"], c["res"][0], mc, mode="mc")
    with pytest.raises(ValueError, match="'mc' ring"):
        I.offline(ag, mc, 5)
    assert ag.updates == 225


def test_entry_script_trains_with_the_term_and_offline_first(tmp_path):
    """SHEMS_BC appends its suffix behind the others and trains; SHEMS_FORESIGHT_OFFLINE writes its rows beside the imitation file."""
    import os
    pytest.importorskip("torch")
    M = importlib.import_module(U.PKG_NAME + ".main")
    base = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
            "SHEMS_SYNTHETIC_DATA": "1"}
    case0 = M.config_from_env(base).case
    cwd0 = os.getcwd()
    try:
        cfg, written = M.main(dict(base, SHEMS_ALGO="td3", SHEMS_BC="2.5:0.5", SHEMS_FORESIGHT="1", SHEMS_FORESIGHT_OFFLINE="20"), cwd=str(tmp_path),
                              log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    assert cfg.case == case0 + "_td3-d2-s0.2-c0.5_bc-a2.5-w0.5"
    off = [w for w in written if w.endswith("_offline.csv")]
    assert off == [M.offline_file_name(cfg.job_id, cfg.run, cfg.case)] and all(cfg.case in w for w in written)
    lines = open(tmp_path / off[0]).read().strip().split("\n")
    assert lines[0] == "update,critic_loss,actor_loss,lambda,mse" and len(lines) == 1 + 20
    assert np.isfinite(np.array([[float(x) for x in l.split(",")] for l in lines[1:]])).all()
    assert M.config_from_env(base).case == case0

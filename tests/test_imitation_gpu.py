"""Imitation of the foresight controller on the GPU: shems_foresight_demos_dev against the NumPy twin (tests/imitation_ref.py) bit for
bit, shems_ddpg_clone_update against the float64 evaluation of the same formulas (oracle/ddpg_oracle.py), and the host layer on top
(imitation.from_foresight / from_pass / dagger, ddpg.Agent.clone)."""
import importlib
import types

import numpy as np
import pytest

import ddpg_oracle as DO
import foresight_twin as FT
import imitation_ref as IR
import util as U

pytestmark = pytest.mark.gpu

SENT = 0xA5                                    # every byte of a ring before a demos call


def _mods():
    S = U.pkg()
    return S, FT.F(), importlib.import_module(U.PKG_NAME + ".imitation"), importlib.import_module(U.PKG_NAME + ".ddpg"), \
        importlib.import_module(U.PKG_NAME + ".harness")


_CACHE = {}


def _s1():
    """S1 on the device, once per process: the values, and the rows of three passes from reset!(rng = -1) -- the foresight pass (with
    the targets it chose), the rule-based pass, the pass of a freshly initialised actor -- with the audit's best action of each."""
    if not _CACHE:
        S, F, I, D, H = _mods()
        d, sh = FT.s1(), FT.S1
        assert d["idx0"] == 1                                               # the passes of harness.inference start on row 1
        T = sh["T"]
        cfgs = FT.configs(S, "s1")
        val = F.solve([d["tab"]], cfgs, d["idx0"], T, F.Grid(sh["nb"], sh["ne"], sh["nab"], sh["nae"]))
        env = S.ShemsBatch(1, T, [d["tab"]], cfgs).use_torch_stream()
        env.reset_(-1)
        _, fs_res, fs_tgt = F.track(env, val)
        _, rule = H.inference(env, None, track=-1, num_steps=T)
        ag = D.Agent(seed=3)
        _, fresh = H.inference(env, ag, track=1, num_steps=T)
        env.close()
        res = np.stack([fs_res[0], rule, fresh])
        best = F.audit(val, res).best_action
        _CACHE.update(val=val, res=res, fs_tgt=fs_tgt[0], best=best, tab=d["tab"], T=T, sh=sh, cfgs=cfgs)
    return _CACHE


def _sentinel_ring(I, cap, pos):
    import torch
    ring = I.Demos(cap)
    for t in (ring.s, ring.a, ring.r, ring.s2, ring.done):
        t.view(torch.uint8).fill_(SENT)
    ring.pushed = pos
    return ring


def _bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _sent_arrays(cap):
    v = np.frombuffer(bytes([SENT] * 4), np.float32)[0]
    return np.full((cap, 9), v, np.float32), np.full((cap, 2), v, np.float32)


@pytest.mark.parametrize("source", ["targets", "best_action"])
def test_s1_three_passes_wrap_the_ring_and_equal_the_twin(source):
    S, F, I, D, H = _mods()
    c = _s1()
    sh, T = c["sh"], c["T"]
    grid_tgt = FT.action_grid(sh["nab"], sh["nae"])
    if source == "targets":                     # the foresight pass with the targets it chose, the others with their best action's
        tg = np.stack([c["fs_tgt"], grid_tgt[c["best"][1]], grid_tgt[c["best"][2]]])
        kw = dict(targets=tg)
    else:
        kw = dict(best_action=c["best"])
    ring = _sentinel_ring(I, 128, 100)
    I._write(c["val"], c["res"], None, ring, **kw)
    assert ring.pushed == 190 and len(ring) == 128 and ring.pos == 62
    slot, ws, wa, st = IR.twin_demos(c["res"], c["tab"], 1, sh["nab"], sh["nae"], pos=100, capacity=128, **kw)
    assert (st == 0).all() and (slot >= 0).all()
    want_s, want_a = IR.fill(slot, ws, wa, 128, _sent_arrays(128))
    assert (U.bits32(ring.s.cpu().numpy()) == U.bits32(want_s)).all()
    assert (U.bits32(ring.a.cpu().numpy()) == U.bits32(want_a)).all()
    untouched = np.setdiff1d(np.arange(128), slot.ravel())
    assert len(untouched) == 38 and (_bytes(ring.s[untouched]) == SENT).all() and (_bytes(ring.a[untouched]) == SENT).all()
    for t in (ring.r, ring.s2, ring.done):
        assert (_bytes(t) == SENT).all()
    if source == "targets":                     # the foresight pass's own labels are the best actions of its own audit (regret 0)
        assert (U.bits32(wa[0]) == U.bits32(IR.label(grid_tgt[c["best"][0]]))).all()


def test_foresight_observations_are_what_the_env_shows_before_each_step():
    """30 single shems_step_dev calls with the recorded targets: shems_get_state before step t is s of slot t."""
    S, F, I, D, H = _mods()
    c = _s1()
    T = c["T"]
    env = S.ShemsBatch(1, T, [c["tab"]], c["cfgs"]).use_torch_stream()
    env.reset_(-1)
    ring = I.Demos(T)
    total, res, tgt = I.from_foresight(env, c["val"], ring)
    assert len(ring) == T and (U.bits64(res[0]) == U.bits64(c["res"][0])).all() and (tgt[0] == c["fs_tgt"]).all()
    s = ring.s.cpu().numpy()
    assert (U.bits32(ring.a.cpu().numpy()) == U.bits32(IR.label(c["fs_tgt"]))).all()
    assert not ring.r.any() and not ring.s2.any() and not ring.done.any()      # zero-allocated, never written
    env.reset_(-1)
    ret = 0.0
    for t in range(T):
        assert (U.bits32(np.array(env.state, np.float32)[0]) == U.bits32(s[t])).all(), t
        r, _, _ = env.step_(None, np.ascontiguousarray(c["fs_tgt"][t:t + 1]), track=1)
        ret += float(r[0])
    assert ret == pytest.approx(float(total[0]), abs=1e-9)
    env.close()


def test_a_corrupted_row_is_flagged_its_slot_untouched_and_the_rest_written():
    S, F, I, D, H = _mods()
    c = _s1()
    sh = c["sh"]
    bad = c["res"][1:2].copy()
    bad[0, 7, 0] += 1
    ring = _sentinel_ring(I, 40, 5)
    with pytest.raises(S._capi.BoundsError, match="pass 0"):
        I._write(c["val"], bad, None, ring, best_action=c["best"][1:2])
    assert ring.pushed == 5                     # a call that raised does not advance the length
    slot, ws, wa, st = IR.twin_demos(bad, c["tab"], 1, sh["nab"], sh["nae"], best_action=c["best"][1:2], pos=5, capacity=40)
    assert st[0] == S._capi.ERR_INDEX and slot[0, 7] == -1 and (slot >= 0).sum() == 29
    want_s, want_a = IR.fill(slot, ws, wa, 40, _sent_arrays(40))
    assert (U.bits32(ring.s.cpu().numpy()) == U.bits32(want_s)).all() and (U.bits32(ring.a.cpu().numpy()) == U.bits32(want_a)).all()
    assert (_bytes(ring.s[12]) == SENT).all() and (_bytes(ring.a[12]) == SENT).all()
    act = c["best"][1:2].copy()
    act[0, 4] = -1                              # an hour without a label
    with pytest.raises(S._capi.BoundsError):
        I._write(c["val"], c["res"][1:2], None, _sentinel_ring(I, 40, 0), best_action=act)
    with pytest.raises(S.ShemsError, match="90 pairs"):                       # more pairs than slots
        I._write(c["val"], c["res"], None, I.Demos(89), best_action=c["best"])
    with pytest.raises(ValueError, match="forecast"):
        I.from_pass(F.Values(c["val"].grid, c["T"], [None], None, None, None, forecast_off=[40], total_rows=80), c["res"], ring)


# ------------------------------------------------------------------ clone update --
# Per-block gradient bound, restated from tests/test_ddpg_gpu.py:57-62: every Flux.params block of the gradient within 2e-6 of ITS
# max-abs of the float64 evaluation (4 x the worst block measured there for float32 accumulation over K <= 500, B <= 128).
BLOCK_TOL = 2e-6
# A relu whose float64 pre-activation lies within fp32 accumulation error of zero is on in one evaluation order and off in another
# (tests/test_group_gpu.py:115-123): a failing block comparison is repeated with every such unit decided the other way.
TIE = 1e-7
# losses[1] against the float64 loss, as a fraction of max(1, |loss|): 4 x the worst distance of the FLOAT32 twin from float64 over
# IR.CLONE_CASES, the rule BLOCK_TOL was set by.  Measured (IR.twin_loss_distance()): worst 7.034e-8, case batch 1, ring length 90.
LOSS_TOL = 4 * 7.034e-8


def _assert_blocks(g, g64, what):
    errs = {n: float(np.abs(g[lo:hi] - g64[lo:hi]).max() / max(np.abs(g64[lo:hi]).max(), 1e-30)) for n, lo, hi in DO.blocks(9, 2)}
    for n, lo, hi in DO.blocks(9, 2):
        assert np.abs(g64[lo:hi]).max() > 0, (what, n, "reference block is all zero: the case does not exercise it")
    bad = {n: e for n, e in errs.items() if not e < BLOCK_TOL}
    assert not bad, (what, errs)
    return errs


def _tied_units(p, x):
    """[(index of the unit's bias in the flat parameter vector, sign of its closest-to-zero float64 pre-activation)]"""
    _, (_, z1, _, z2, _, _) = DO.mlp_forward(p, x, 9, 2, True, keep=True, dtype=np.float64)
    out = []
    for z, off in ((z1, 9 * 250), (z2, 9 * 250 + 250 + 250 * 500)):
        for u in np.unique(np.where(np.abs(z) < TIE)[1]):
            col = z[:, u]
            out.append((off + int(u), float(np.sign(col[np.argmin(np.abs(col))]) or 1.0)))
    return out


def _assert_blocks_or_the_other_relu_decision(g, actor, evaluate, x, what):
    """evaluate(actor parameters) -> float64 gradient.  Returns (per-block errors, tie used?)."""
    try:
        return _assert_blocks(g, evaluate(actor), what), False
    except AssertionError:
        tied = _tied_units(actor, x)
        if not tied or len(tied) > 3:
            raise
        flipped = actor.astype(np.float64)
        for i, sg in tied:
            flipped[i] -= sg * 4 * TIE
        return _assert_blocks(g, evaluate(flipped), what + " (tied relus decided the other way)"), True


def _clone_setup(length, batch, seed=IR.CLONE_SEED, hidden=(250, 500)):
    import torch
    S, F, I, D, H = _mods()
    d = IR.clone_data()
    ring = I.Demos(IR.CLONE_CAP)
    ring.s.copy_(torch.from_numpy(d["s"]))
    ring.a.copy_(torch.from_numpy(d["a"]))
    ring.r.fill_(float("nan"))                  # the update reads s and a only: anything it took from here would show
    ring.s2.fill_(float("nan"))
    ring.pushed = length
    ag = D.Agent(seed=seed, hidden=hidden)
    if hidden == (250, 500):
        ag.set_params(actor=d["pa"], critic=d["pc"])
    ag.set_norm(d["s_min"], d["s_max"])
    ag.batch = batch
    for k, v in (("m_critic", 0.25), ("v_critic", 0.5), ("grad_critic", -3.0)):      # what the update must leave alone, made visible
        getattr(ag, k).fill_(v)
    ag.losses[0] = 42.0
    return torch, D, ag, ring, d


@pytest.mark.parametrize("tau", [0.001, 1.0])
@pytest.mark.parametrize("batch,length", IR.CLONE_CASES)
def test_clone_update_matches_float64(batch, length, tau):
    torch, D, ag, ring, d = _clone_setup(length, batch)
    critic_side = {k: getattr(ag, k).clone() for k in ("critic", "critic_t", "m_critic", "v_critic", "grad_critic")}
    pub = torch.zeros_like(ag.actor)
    tick = IR.CLONE_TICK
    g64, l64, idx = IR.clone_reference(batch, length, np.float64)
    assert (ag.sample_indices(tick, length) == idx).all()
    ag.clone(ring, tick=tick, tau=tau, publish=pub)
    torch.cuda.synchronize()
    assert ag.clones == 1 and ag.updates == 0 and ag.bp_actor == [0.9 * 0.9, 0.999 * 0.999] and ag.bp_critic == [0.9, 0.999]
    g = ag.grad_actor.cpu().numpy()
    x = DO.normalize(d["s"][idx], d["s_min"], d["s_max"])
    ev = lambda p: IR.clone_grad(p, d["s"][idx], d["a"][idx], d["s_min"], d["s_max"], np.float64)[0]
    errs, tie = _assert_blocks_or_the_other_relu_decision(g, d["pa"], ev, x, f"clone gradient B={batch} len={length}")
    loss = float(ag.losses[1].item())
    print(f"B={batch} len={length} tau={tau}: block errors {errs}, tie {tie}; loss {loss!r} vs float64 {l64!r}: "
          f"{abs(loss - l64) / max(1.0, abs(l64)):.3e} (bound {LOSS_TOL:.3e})")
    assert np.isfinite(g).all() and abs(loss - l64) <= LOSS_TOL * max(1.0, abs(l64))
    # the minibatch the launches saw: normalised columns, stored labels, zero padding
    ws = ag.ws.cpu().numpy()
    XT, AT = ws[0:9 * 128].reshape(9, 128), ws[18 * 128:20 * 128].reshape(2, 128)
    np.testing.assert_allclose(XT[:, :batch].T, x, rtol=0, atol=1e-6)
    assert (AT[:, :batch].T == d["a"][idx]).all() and not XT[:, batch:].any() and not AT[:, batch:].any()
    # ADAM + soft update, element-wise, from the kernel's own gradient
    opt = DO.Adam(len(g), DO.ETA_ACT)
    pa1 = opt.step(d["pa"], g)
    act = ag.actor.cpu().numpy()
    np.testing.assert_allclose(act, pa1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.actor_t.cpu().numpy(), DO.soft_update(d["pa"], act, np.float32(tau)), rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.m_actor.cpu().numpy(), opt.m, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(ag.v_actor.cpu().numpy(), opt.v, rtol=1e-6, atol=1e-15)
    if tau == 1.0:
        assert torch.equal(ag.actor_t, ag.actor)                            # 1 p + 0 t
    else:
        assert not torch.equal(ag.actor_t, ag.actor)
    assert torch.equal(pub, ag.actor)
    for k, v in critic_side.items():
        assert torch.equal(getattr(ag, k), v), k
    assert float(ag.losses[0].item()) == 42.0


def test_second_clone_step_uses_advanced_beta_powers():
    torch, D, ag, ring, d = _clone_setup(90, 120)
    opt = DO.Adam(D.N_ACTOR, DO.ETA_ACT)
    p = d["pa"].copy()
    for t in range(3):
        ag.clone(ring, tick=t, tau=0.001)
        p = opt.step(p, ag.grad_actor.cpu().numpy())
        act = ag.actor.cpu().numpy()            # produced from the kernel's own previous actor: compare the step
        np.testing.assert_allclose(act, p, rtol=0, atol=2e-7)
        p = act
    assert ag.clones == 3 and ag.updates == 0 and abs(ag.bp_actor[0] - 0.9 ** 4) < 1e-15 and abs(ag.bp_actor[1] - 0.999 ** 4) < 1e-15
    before = ag.clones
    ag.clone(ring)                              # the default tick is the clone counter
    assert ag.clones == before + 1


def test_two_runs_leave_the_same_bytes():
    out = []
    for _ in range(2):
        torch, D, ag, ring, d = _clone_setup(128, 120)
        for t in range(3):
            ag.clone(ring, tick=t, tau=0.5)
        torch.cuda.synchronize()
        out.append({k: getattr(ag, k).clone() for k in ag._LEARNER_TENSORS})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    assert float(out[0]["grad_actor"][:2500].abs().max()) > 0


def test_a_padded_net_keeps_its_padding_at_zero():
    torch, D, ag, ring, d = _clone_setup(128, 120, hidden=(200, 400))
    own = D.net_size(9, 2, (200, 400))
    pad = D.pad_net(np.ones(own, np.float32), 9, 2, (200, 400)) == 0        # True where the (250, 500) layout holds padding
    pad[-2:] = False                                                        # (b3 of ones stays ones: not padding)
    assert pad.sum() == D.N_ACTOR - own
    first = ag.export_actor()
    for t in range(3):
        ag.clone(ring, tick=t, tau=0.5)
    torch.cuda.synchronize()
    for k in ("actor", "actor_t", "m_actor", "v_actor", "grad_actor"):
        v = getattr(ag, k).cpu().numpy()
        assert (U.bits32(v[pad]) == 0).all(), k
        assert np.isfinite(v).all() and np.abs(v[~pad]).max() > 0, k
    assert (ag.export_actor() != first).mean() > 0.3 and ag.export_actor().size == own


def test_what_clone_refuses():
    torch, D, ag, ring, d = _clone_setup(90, 129)
    with pytest.raises(NotImplementedError, match="129"):
        ag.clone(ring)
    ag.batch = 120
    ag.sync = types.SimpleNamespace(world=2)
    with pytest.raises(NotImplementedError, match="replicas"):
        ag.clone(ring)
    wide = D.Agent(seed=1, hidden=(300, 600))
    with pytest.raises(NotImplementedError, match="300"):
        wide.clone(ring)
    assert ag.clones == 0 and wide.clones == 0


# -------------------------------------------------------------------- end to end --
def test_cloning_the_foresight_pass_lowers_the_loss():
    import torch
    S, F, I, D, H = _mods()
    c = _s1()
    env = S.ShemsBatch(1, c["T"], [c["tab"]], c["cfgs"]).use_torch_stream()
    env.reset_(-1)
    demos = I.Demos(64)
    I.from_foresight(env, c["val"], demos)
    env.close()
    assert len(demos) == 30 and demos.pos == 30
    ag = D.Agent(seed=5)
    ag.min_max_buffer(demos)
    s = demos.s[:30].cpu().numpy()
    assert (ag.s_min.cpu().numpy() >= s.min(0)).all() and (ag.s_max.cpu().numpy() <= s.max(0)).all()
    ag.batch = 30
    losses = []
    for k in range(200):
        ag.clone(demos)
        if k in (0, 199):
            losses.append(float(ag.losses[1].item()))
    print("clone loss: first", losses[0], "last", losses[-1])
    assert ag.clones == 200 and losses[-1] < losses[0]
    for k in ("actor", "actor_t", "m_actor", "v_actor"):
        assert torch.isfinite(getattr(ag, k)).all(), k
    assert torch.equal(ag.actor, ag.actor_t)


def test_dagger_appends_a_pass_per_round_and_returns_finite_figures():
    S, F, I, D, H = _mods()
    c = _s1()
    env = S.ShemsBatch(1, c["T"], [c["tab"]], c["cfgs"]).use_torch_stream()
    demos = I.Demos(128)
    ag = D.Agent(seed=5)
    ag.batch = 30
    out = I.dagger(ag, env, c["val"], demos, 2, 20)
    env.close()
    assert [r["demos"] for r in out] == [30, 60] and len(demos) == 60 and ag.clones == 40 and ag.updates == 0
    assert all(np.isfinite(r["return"]) and np.isfinite(r["loss"]) for r in out)
    assert out[0]["return"] == pytest.approx(float(c["res"][0][:, 5].sum()), abs=1e-9)      # round 0 is the foresight pass
    # round 1's pairs are the states the cloned actor visited, labelled on the action grid
    a = demos.a[30:60].cpu().numpy()
    grid_lab = IR.label(FT.action_grid(c["sh"]["nab"], c["sh"]["nae"]))
    assert all((grid_lab == x).all(1).any() for x in a)


def test_entry_script_writes_the_imitation_file_beside_the_foresight_file(tmp_path):
    import csv
    import os
    S, F, I, D, H = _mods()
    M = importlib.import_module(U.PKG_NAME + ".main")
    env = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "1", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
           "SHEMS_SYNTHETIC_DATA": "1", "SHEMS_TRAIN": "0", "SHEMS_TRACK": "-1", "SHEMS_FORESIGHT": "1", "SHEMS_FORESIGHT_IMITATE": "2x3"}
    cwd0 = os.getcwd()
    try:
        cfg, written = M.main(env, cwd=str(tmp_path), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    names = [f"1179808_eval_results_{cfg.case}_rule_-1.csv", f"1179808_eval_results_{cfg.case}_foresight.csv",
             f"1179808_eval_results_{cfg.case}_imitation.csv"]
    assert [os.path.basename(w) for w in written] == names
    rows = list(csv.reader(open(tmp_path / written[2])))
    assert rows[0] == I.IMITATION_HEADER and len(rows) == 3
    assert [int(r[0]) for r in rows[1:]] == [0, 1] and [int(r[3]) for r in rows[1:]] == [1439, 2878]
    assert np.isfinite(np.array([[float(r[1]), float(r[2])] for r in rows[1:]])).all()
    fs = np.array(list(csv.reader(open(tmp_path / written[1])))[1:], np.float64)
    assert float(rows[1][1]) == pytest.approx(fs[:, 5].sum(), abs=1e-9)        # round 0 is the foresight pass the file beside it holds

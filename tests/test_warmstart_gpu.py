"""The DDPG warm start on the GPU: shems_foresight_transitions_dev against the NumPy twin (tests/warmstart_ref.py) bit for bit and
against the env itself, shems_ddpg_critic_update against the split calls (same bits) and against the float64 evaluation of the same
formulas (oracle/ddpg_oracle.py), and the host layer on top (imitation.transitions / warm_start, ddpg.Agent.evaluate, the entry
script's switch)."""
import importlib
import os

import numpy as np
import pytest

import ddpg_oracle as DO
import foresight_regret_ref as RR
import foresight_twin as FT
import imitation_ref as IR
import test_imitation_gpu as TI                # S1 on the device, once per process: the three passes exactly as its tests use them
import util as U
import warmstart_ref as WR

pytestmark = pytest.mark.gpu

SENT = TI.SENT
GAMMA = 0.99
CRITIC_SIDE = ("critic", "critic_t", "m_critic", "v_critic", "grad_critic")
ACTOR_SIDE = ("actor", "actor_t", "m_actor", "v_actor", "grad_actor")


def _sentinel_ring(D, cap, pos):
    import torch
    ring = D.ReplayRing(cap)
    for t in (ring.s, ring.a, ring.r, ring.s2, ring.done):
        t.view(torch.uint8).fill_(SENT)
    ring.pushed = pos
    return ring


def _ring_equals(ring, want):
    for k in ("s", "a", "r", "s2"):
        assert (U.bits32(getattr(ring, k).cpu().numpy()) == U.bits32(want[k])).all(), k
    assert (ring.done.cpu().numpy() == want["done"]).all()


# ------------------------------------------------------------------ transitions --
@pytest.mark.parametrize("mode,tail,count", [("td", 1, 87), ("mc", 5, 75)])
def test_s1_three_passes_wrap_the_ring_and_equal_the_twin(mode, tail, count):
    """The foresight pass, the rule-based pass (its rows used mechanically) and a fresh actor's pass into 128 sentinel slots from
    slot 100: all five arrays and the returns equal the twin bit for bit, the untouched slots keep the sentinel in all five."""
    S, F, I, D, H = TI._mods()
    c = TI._s1()
    ring = _sentinel_ring(D, 128, 100)
    ret = I.transitions(c["val"], c["res"], ring, mode=mode, gamma=GAMMA, tail=tail)
    assert ring.pushed == 100 + count and len(ring) == 128
    tw = WR.twin_transitions(c["res"], [c["tab"]] * 3, [1] * 3, WR.TRANSITION_MODE[mode], GAMMA, tail, pos=100, capacity=128)
    assert (tw["status"] == 0).all() and (tw["slot"] >= 0).all() and tw["slot"].size == count
    _ring_equals(ring, WR.fill(tw, 128, WR.sentinel_arrays(128, SENT)))
    untouched = np.setdiff1d(np.arange(128), tw["slot"].ravel())
    assert len(untouched) == 128 - count
    for t in (ring.s, ring.a, ring.r, ring.s2, ring.done):
        assert (TI._bytes(t[untouched]) == SENT).all()
    if mode == "mc":
        assert ret.shape == (3, 30) and (U.bits64(ret) == U.bits64(tw["G"])).all() and np.isfinite(ret).all()
        assert (ring.done.cpu().numpy()[tw["slot"].ravel()] == 1).all()
    else:
        assert ret is None and (ring.done.cpu().numpy()[tw["slot"].ravel()] == 0).all()


def test_transitions_are_what_the_env_does():
    """29 single shems_step_dev calls with the targets the foresight pass recorded: s is the state before step t, s2 the state after
    it, r the float32 of the reward, a the label of the targets, which columns 21 and 2 of the rows hold."""
    S, F, I, D, H = TI._mods()
    c = TI._s1()
    T = c["T"]
    res, tgt = c["res"][0], c["fs_tgt"]
    assert (res[:, 21] == tgt[:, 0].astype(np.float64)).all() and (res[:, 2] == tgt[:, 1].astype(np.float64)).all()
    ring = D.ReplayRing(T - 1)
    assert I.transitions(c["val"], res, ring) is None and len(ring) == T - 1            # [T][23], the defaults: td, tail 1
    s, a, r, s2 = (getattr(ring, k).cpu().numpy() for k in ("s", "a", "r", "s2"))
    assert (U.bits32(a) == U.bits32(IR.label(tgt[:T - 1]))).all() and not ring.done.any()
    env = S.ShemsBatch(1, T, [c["tab"]], c["cfgs"]).use_torch_stream()
    env.reset_(-1)
    for t in range(T - 1):
        assert (U.bits32(np.array(env.state, np.float32)[0]) == U.bits32(s[t])).all(), t
        rew, _, _ = env.step_(None, np.ascontiguousarray(tgt[t:t + 1]), track=1)
        assert (U.bits32(np.array(env.state, np.float32)[0]) == U.bits32(s2[t])).all(), t
        assert U.bits32(np.float32(rew[0])) == U.bits32(r[t]), t
    env.close()


def test_s2_problem_of_pass_and_a_pass_that_names_no_problem():
    S, F, I, D, H = TI._mods()
    d, sh = FT.s2(), FT.S2
    val = F.solve(d["tabs"], FT.configs(S, "s2"), d["idx0"], sh["T"], F.Grid(sh["nb"], sh["ne"], sh["nab"], sh["nae"]))
    res = RR.s2_passes()[:3]                                                # random-target passes on problems 3, 0, 2
    po = list(RR.S2_PASSES[:3])
    for mode, tail in (("td", 1), ("mc", 2)):
        keep = sh["T"] - tail
        ring = _sentinel_ring(D, 32, 30)
        ret = I.transitions(val, res[:2], ring, po[:2], mode=mode, gamma=GAMMA, tail=tail)
        tw = WR.twin_transitions(res[:2], [d["tabs"][p] for p in po[:2]], [d["idx0"][p] for p in po[:2]], WR.TRANSITION_MODE[mode], GAMMA,
                                 tail, pos=30, capacity=32)
        assert (tw["status"] == 0).all() and (tw["slot"] >= 0).all() and ring.pushed == 30 + 2 * keep
        _ring_equals(ring, WR.fill(tw, 32, WR.sentinel_arrays(32, SENT)))
        assert ret is None or (U.bits64(ret) == U.bits64(tw["G"])).all()
        # the same rows under the wrong problem do not sit on its table rows
        with pytest.raises(S._capi.BoundsError, match="pass 0"):
            I.transitions(val, res[:2], _sentinel_ring(D, 32, 0), [0, 0], mode=mode, gamma=GAMMA, tail=tail)
        # the middle pass names no problem: flagged, nothing of it written, the others are, and the length stays
        ring = _sentinel_ring(D, 32, 30)
        with pytest.raises(S._capi.BoundsError, match="pass 1"):
            I.transitions(val, res, ring, [po[0], 7, po[2]], mode=mode, gamma=GAMMA, tail=tail)
        assert ring.pushed == 30
        tw = WR.twin_transitions(res, [d["tabs"][po[0]], None, d["tabs"][po[2]]], [d["idx0"][po[0]], None, d["idx0"][po[2]]],
                                 WR.TRANSITION_MODE[mode], GAMMA, tail, pos=30, capacity=32)
        assert (tw["status"] == [0, S._capi.ERR_INDEX, 0]).all() and (tw["slot"][1] == -1).all() and (tw["slot"][[0, 2]] >= 0).all()
        _ring_equals(ring, WR.fill(tw, 32, WR.sentinel_arrays(32, SENT)))


# ---------------------------------------------------------------- critic update --
# Per-block gradient bound, restated from tests/test_ddpg_gpu.py:57-62: every Flux.params block of the gradient within 2e-6 of ITS
# max-abs of the float64 evaluation (4 x the worst block measured there for float32 accumulation over K <= 500, B <= 128).
BLOCK_TOL = 2e-6
# A relu whose float64 pre-activation lies within fp32 accumulation error of zero is on in one evaluation order and off in another
# (tests/test_group_gpu.py:115-123): a failing block comparison is repeated with every such unit decided the other way.
TIE = 1e-7


def _block_errs(g, g64):
    return {n: float(np.abs(g[lo:hi] - g64[lo:hi]).max() / max(np.abs(g64[lo:hi]).max(), 1e-30)) for n, lo, hi in DO.blocks(11, 1)}


def _assert_blocks(g, g64, what):
    errs = _block_errs(g, g64)
    for n, lo, hi in DO.blocks(11, 1):
        assert np.abs(g64[lo:hi]).max() > 0, (what, n, "reference block is all zero: the case does not exercise it")
    bad = {n: e for n, e in errs.items() if not e < BLOCK_TOL}
    assert not bad, (what, errs)
    return errs


def _tied_units(p, x):
    _, (_, z1, _, z2, _, _) = DO.mlp_forward(p, x, 11, 1, False, keep=True, dtype=np.float64)
    out = []
    for z, off in ((z1, 11 * 250), (z2, 11 * 250 + 250 + 250 * 500)):
        for u in np.unique(np.where(np.abs(z) < TIE)[1]):
            col = z[:, u]
            out.append((off + int(u), float(np.sign(col[np.argmin(np.abs(col))]) or 1.0)))
    return out


def _assert_blocks_or_the_other_relu_decision(g, critic, evaluate, x, what):
    try:
        return _assert_blocks(g, evaluate(critic), what), False
    except AssertionError:
        tied = _tied_units(critic, x)
        if not tied or len(tied) > 3:
            raise
        flipped = critic.astype(np.float64)
        for i, sg in tied:
            flipped[i] -= sg * 4 * TIE
        return _assert_blocks(g, evaluate(flipped), what + " (tied relus decided the other way)"), True


def _critic_setup(length, batch, reward="r", done=None):
    """critic_data in a ring of IR.CLONE_CAP slots of which `length` count, an agent on its networks with targets of their own, and
    what the update must leave alone made visible."""
    import torch
    S, F, I, D, H = TI._mods()
    d = WR.critic_data()
    ring = D.ReplayRing(IR.CLONE_CAP)
    dn = d["done"] if done is None else np.full(IR.CLONE_CAP, done, np.uint8)
    for t, v in ((ring.s, d["s"]), (ring.a, d["a"]), (ring.r, d[reward]), (ring.s2, d["s2"]), (ring.done, dn)):
        t.copy_(torch.from_numpy(v))
    ring.pushed = length
    ag = D.Agent(seed=WR.CRITIC_SEED)
    ag.set_params(actor=d["pa"], critic=d["pc"])
    ag.actor_t.copy_(torch.from_numpy(d["pa_t"]))
    ag.critic_t.copy_(torch.from_numpy(d["pc_t"]))
    ag.set_norm(d["s_min"], d["s_max"])
    ag.batch = batch
    for k, v in (("m_actor", 0.25), ("v_actor", 0.5), ("grad_actor", -3.0)):
        getattr(ag, k).fill_(v)
    ag.losses[1] = 42.0
    return torch, D, ag, ring, d


def _split_step(ag, ring, tick):
    d, st, rs = ag._ddpg_args(), ag._stream(), ring.struct()
    ag._critic_grad_ex(d, rs, len(ring), tick, 0, 0, st)
    ag._critic_apply(d, 1.0, st)
    ag.bp_critic = [ag.bp_critic[0] * 0.9, ag.bp_critic[1] * 0.999]


@pytest.mark.parametrize("done", [None, 1])
@pytest.mark.parametrize("batch,length", WR.CRITIC_CASES)
def test_evaluate_leaves_the_bits_of_the_split_form(batch, length, done):
    torch, D, ag, ring, d = _critic_setup(length, batch, done=done)
    if done is None:
        assert set(d["done"][:length].tolist()) == ({0, 1} if length > 1 else {0})
    snap = ag.snapshot()
    actor_side = {k: getattr(ag, k).clone() for k in ACTOR_SIDE}
    for step in range(2):                       # the second step runs on the advanced beta powers and the moved target
        ag.evaluate(ring, tick=WR.CRITIC_TICK + step)
    torch.cuda.synchronize()
    assert ag.evaluations == 2 and ag.updates == 0 and ag.clones == 0
    assert ag.bp_critic == [0.9 * 0.9 * 0.9, 0.999 * 0.999 * 0.999] and ag.bp_actor == [0.9, 0.999]
    for k, v in actor_side.items():
        assert torch.equal(getattr(ag, k), v), k
    assert float(ag.losses[1].item()) == 42.0
    got = {k: getattr(ag, k).clone() for k in CRITIC_SIDE + ("losses",)}
    ag.restore(snap)
    for step in range(2):
        _split_step(ag, ring, WR.CRITIC_TICK + step)
    torch.cuda.synchronize()
    for k in CRITIC_SIDE:
        assert torch.equal(got[k], getattr(ag, k)), k
    assert torch.equal(got["losses"][:1], ag.losses[:1])
    assert not torch.equal(got["critic"], snap[0]["critic"]) and not torch.equal(got["critic_t"], snap[0]["critic_t"])


def test_two_runs_leave_the_same_bytes_and_the_default_tick_is_the_counter():
    out = []
    for _ in range(2):
        torch, D, ag, ring, d = _critic_setup(128, 120)
        for _ in range(3):
            ag.evaluate(ring)                   # ticks 0, 1, 2
        torch.cuda.synchronize()
        out.append({k: getattr(ag, k).clone() for k in ag._LEARNER_TENSORS})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    assert ag.evaluations == 3
    torch, D, ag, ring, d = _critic_setup(128, 120)
    for t in range(3):
        ag.evaluate(ring, tick=t)
    torch.cuda.synchronize()
    for k in CRITIC_SIDE:
        assert torch.equal(out[0][k], getattr(ag, k)), k


@pytest.mark.parametrize("done", [None, 1])
@pytest.mark.parametrize("batch,length", WR.CRITIC_CASES)
def test_evaluate_matches_float64(batch, length, done):
    torch, D, ag, ring, d = _critic_setup(length, batch, done=done)
    tick = WR.CRITIC_TICK
    g64, l64, y, idx = WR.critic_reference(batch, length, done=done)
    assert (ag.sample_indices(tick, length) == idx).all()
    ag.evaluate(ring, tick=tick, tau=0.25)
    torch.cuda.synchronize()
    g = ag.grad_critic.cpu().numpy()
    x = np.concatenate([DO.normalize(d["s"][idx], d["s_min"], d["s_max"]), d["a"][idx]], 1)
    ev = lambda p: WR.critic_reference(batch, length, done=done, critic=p)[0]
    errs, tie = _assert_blocks_or_the_other_relu_decision(g, d["pc"], ev, x, f"critic gradient B={batch} len={length} done={done}")
    loss = float(ag.losses[0].item())
    print(f"B={batch} len={length} done={done}: block errors {errs}, tie {tie}; loss {loss!r} vs float64 {l64!r}")
    assert np.isfinite(g).all() and np.isfinite(loss)
    # ADAM + soft update, element-wise, from the kernel's own gradient
    opt = DO.Adam(len(g), DO.ETA_CRIT)
    pc1 = opt.step(d["pc"], g)
    crit = ag.critic.cpu().numpy()
    np.testing.assert_allclose(crit, pc1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.critic_t.cpu().numpy(), DO.soft_update(d["pc_t"], crit, np.float32(0.25)), rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.m_critic.cpu().numpy(), opt.m, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(ag.v_critic.cpu().numpy(), opt.v, rtol=1e-6, atol=1e-15)


@pytest.mark.parametrize("batch,length", [(120, 128), (7, 90)])
def test_on_an_mc_ring_the_target_is_the_stored_return(batch, length):
    """Rewards of the magnitude of real returns, done = 1 in every slot: y = r + gamma (1 - done) q' is the stored float32 G exactly,
    in the oracle and in the launch, and the gradient holds the same bound."""
    torch, D, ag, ring, d = _critic_setup(length, batch, reward="G", done=1)
    tick = WR.CRITIC_TICK
    g64, l64, y, idx = WR.critic_reference(batch, length, reward="G", done=1)
    assert (U.bits32(y) == U.bits32(d["G"][idx])).all() and np.abs(y).max() > 100
    ag.evaluate(ring, tick=tick)
    torch.cuda.synchronize()
    Y = ag.ws.cpu().numpy()[128 * 22:128 * 23][:batch]                      # WS_Y = (9 + 9 + 2 + 1 + 1) * 128
    assert (U.bits32(Y) == U.bits32(d["G"][idx])).all()
    g = ag.grad_critic.cpu().numpy()
    x = np.concatenate([DO.normalize(d["s"][idx], d["s_min"], d["s_max"]), d["a"][idx]], 1)
    ev = lambda p: WR.critic_reference(batch, length, reward="G", done=1, critic=p)[0]
    errs, tie = _assert_blocks_or_the_other_relu_decision(g, d["pc"], ev, x, f"critic gradient on returns B={batch} len={length}")
    print(f"MC ring B={batch} len={length}: block errors {errs}, tie {tie}; loss {float(ag.losses[0].item())!r} vs float64 {l64!r}")


def test_what_evaluate_refuses():
    import types
    torch, D, ag, ring, d = _critic_setup(90, 129)
    with pytest.raises(NotImplementedError, match="129"):
        ag.evaluate(ring)
    ag.batch = 120
    ag.sync = types.SimpleNamespace(world=2)
    with pytest.raises(NotImplementedError, match="replicas"):
        ag.evaluate(ring)
    wide = D.Agent(seed=1, hidden=(300, 600))
    with pytest.raises(NotImplementedError, match="300"):
        wide.evaluate(ring)
    assert ag.evaluations == 0 and wide.evaluations == 0


# -------------------------------------------------------------------- end to end --
@pytest.mark.parametrize("mode", ["td", "mc"])
def test_warm_start_fits_the_critic_on_a_pass_of_the_cloned_actor(mode):
    S, F, I, D, H = TI._mods()
    c = TI._s1()
    T = c["T"]
    env = S.ShemsBatch(1, T, [c["tab"]], c["cfgs"]).use_torch_stream()
    demos, ring = I.Demos(128), D.ReplayRing(64)
    ag = D.Agent(seed=5)
    ag.batch = 30
    out = I.warm_start(ag, env, c["val"], demos, ring, 2, 20, 50, mode=mode)
    env.close()
    *rounds, critic = out
    assert [r["demos"] for r in rounds] == [30, 60] and ag.clones == 40 and ag.evaluations == 50 and ag.updates == 0
    want = T - I.default_tail(mode, ag.gamma, T)
    assert critic["transitions"] == want == len(ring) and want == (29 if mode == "td" else 1)
    assert set(critic) == {"critic_loss_first", "critic_loss_last", "transitions"}
    assert np.isfinite(critic["critic_loss_first"]) and np.isfinite(critic["critic_loss_last"])
    print(f"warm start {mode}: critic loss first {critic['critic_loss_first']!r} last {critic['critic_loss_last']!r}")
    if mode == "mc":
        assert critic["critic_loss_last"] < critic["critic_loss_first"]    # regression on fixed targets with eta 1e-3
        assert ring.done[:want].all()
    else:
        assert not ring.done.any()
        ag.replay(ring)                         # the same ring goes straight on as the replay ring
        ag.replay(ring)
        assert ag.updates == 2


def test_entry_script_writes_the_warmstart_file_beside_the_imitation_file(tmp_path):
    import csv
    S, F, I, D, H = TI._mods()
    M = importlib.import_module(U.PKG_NAME + ".main")
    base = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "1", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
            "SHEMS_SYNTHETIC_DATA": "1", "SHEMS_TRAIN": "0", "SHEMS_TRACK": "-1", "SHEMS_FORESIGHT": "1"}
    cwd0 = os.getcwd()
    runs = {}
    for name, extra in (("with", {"SHEMS_FORESIGHT_IMITATE": "2x3", "SHEMS_FORESIGHT_WARMSTART": "4"}), ("without", {})):
        os.makedirs(tmp_path / name)
        try:
            runs[name] = M.main(dict(base, **extra), cwd=str(tmp_path / name), log=lambda *_: None)
        finally:
            os.chdir(cwd0)
    cfg, written = runs["with"]
    stem = f"1179808_eval_results_{cfg.case}"
    assert [os.path.basename(w) for w in written] == [stem + "_rule_-1.csv", stem + "_foresight.csv", stem + "_imitation.csv", stem + "_warmstart.csv"]
    assert os.path.dirname(written[3]) == os.path.dirname(written[2])
    rows = list(csv.reader(open(tmp_path / "with" / written[3])))
    assert rows[0] == I.WARMSTART_HEADER == ["critic_loss_first", "critic_loss_last"] and len(rows) == 2
    assert np.isfinite([float(x) for x in rows[1]]).all()
    imit = list(csv.reader(open(tmp_path / "with" / written[2])))
    assert imit[0] == I.IMITATION_HEADER and [int(r[3]) for r in imit[1:]] == [1439, 2878]
    cfg, written = runs["without"]
    assert [os.path.basename(w) for w in written] == [stem + "_rule_-1.csv", stem + "_foresight.csv"]
    left = {f for _, _, fs in os.walk(tmp_path / "without") for f in fs}
    assert not any("imitation" in f or "warmstart" in f for f in left)

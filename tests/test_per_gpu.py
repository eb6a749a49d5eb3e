"""GPU tests of prioritized replay (include/shems_hip.h: shems_per_sample_dev, shems_ddpg_update_given, shems_ddpg_update_per): the
sampler against the NumPy twin bit for bit, the GIVEN instantiations pinned to replay()'s bytes, every stage of the prioritized update
from the device's own previous stage, the write-back, and the refusals.

Tolerance-class outputs (powf): the importance weights and the new priorities are held to a float64 evaluation from the device's own
inputs.  Measured on MI355X: worst relative error of a weight 1.67e-7 (all sampler cases), of a new priority 8.4e-8 (batch 128);
bound = four times that (6.7e-7 and 3.4e-7), under the 1e-5 of the act path's class."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ddpg_oracle as DO
import per_cases as PC
import per_ref as PR
import test_ddpg_gpu as TD
import util as U

pytestmark = pytest.mark.gpu
f32 = np.float32

WEIGHT_ERR_MEASURED, PRIO_ERR_MEASURED = 1.67e-7, 8.4e-8
WEIGHT_TOL, PRIO_TOL = min(4 * WEIGHT_ERR_MEASURED, 1e-5), min(4 * PRIO_ERR_MEASURED, 1e-5)
LEARNER_ARRAYS = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic", "losses")
RING_ARRAYS = ("s", "a", "r", "s2", "done")
WS_Y, WS_Q, WS_D3C = 22 * 128, 23 * 128, 26 * 128
TIE = 1e-6


def _R():
    return importlib.import_module(U.PKG_NAME + ".replay")


def _per_ring(D, torch, ring, prio=None, **kw):
    """A PrioritizedRing with the transitions of `ring`, every priority set (no fresh range)."""
    pr = D.PrioritizedRing(ring.capacity, **kw)
    for k in RING_ARRAYS:
        getattr(pr, k).copy_(getattr(ring, k))
    pr.pushed = pr.covered = ring.pushed
    if prio is not None:
        pr.prio.copy_(torch.from_numpy(np.ascontiguousarray(prio, f32)))
    return pr


def _setup(batch=120, seed=11, cap=24000, boost=30.0, kind="decades", **kw):
    torch, S, D, ag, ring, h = TD._setup(seed=seed, cap=cap, boost=boost)
    ag.batch = batch
    prio = PC.update_priorities(kind, cap, seed)
    return torch, S, D, ag, ring, _per_ring(D, torch, ring, prio, **kw), h, prio


def _snap(ag):
    return {k: getattr(ag, k).clone() for k in LEARNER_ARRAYS}


def _given(torch, idx, batch):
    full = np.full(128, -1, np.int32)
    full[:batch] = idx[:batch]
    return torch.from_numpy(full).cuda(), torch.ones(128, dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------ the sampler --
def test_sampler_equals_the_twin_on_every_case():
    """Every case of tests/per_cases.py (ring_len 1 / 255 / 256 / 257 / 1 000 of 1 000 / 24 000; batch 1 / 17 / 120 / 128; random
    priorities, exact zeros, all mass in one slot, all mass in the last partial block; fresh ranges empty / one / wrapping / >= capacity
    with pmax != 1): slots, every S_b / C_b, T, u, t and the freshly filled prio equal the twin exactly; the weights are held to
    float64 from the device's own T and pi; pad columns hold -1 and 0; prio outside [0, ring_len) keeps its sentinel."""
    torch = pytest.importorskip("torch")
    S, R = U.pkg(), _R()
    L = R._declare_per()
    worst = 0.0
    for name, case in PC.sampler_cases():
        prio = PC.build(case)
        tw = PC.twin(case, prio)
        cap, n, b = case["capacity"], case["ring_len"], case["batch"]
        d_prio = torch.from_numpy(prio.copy()).cuda()
        d_pmax = torch.full((1,), case["pmax"], dtype=torch.float32, device="cuda")
        d_ws = torch.full((R.per_workspace_floats(cap) + 8,), -3.0, dtype=torch.float32, device="cuda")
        per = R.PerArgs(d_prio.data_ptr(), d_pmax.data_ptr(), d_ws.data_ptr(), 0.6, case["beta"], 1e-6, 0)
        S._capi.check(L.shems_per_sample_dev(C.byref(per), cap, n, case["fresh"][0], case["fresh"][1], case["seed"], case["tick"], b, None))
        torch.cuda.synchronize()
        ws, p = d_ws.cpu().numpy(), d_prio.cpu().numpy()
        nb = PR.n_blocks(n)
        assert U.bits32(ws[PR.PW_T:PR.PW_T + 1])[0] == U.bits32(np.array([tw["T"]], f32))[0], name
        assert ws[PR.PW_T + 2:PR.PW_T + 3].view(np.int32)[0] == nb, name
        assert np.array_equal(U.bits32(ws[PR.PW_S:PR.PW_S + nb]), U.bits32(tw["S"])), (name, "S")
        assert np.array_equal(U.bits32(ws[PR.PW_S + nb:PR.PW_S + 2 * nb]), U.bits32(tw["C"])), (name, "C")
        assert np.array_equal(U.bits32(ws[PR.PW_U:PR.PW_U + 128]), U.bits32(tw["u"])), (name, "u")
        assert np.array_equal(U.bits32(ws[PR.PW_TM:PR.PW_TM + 128]), U.bits32(tw["t"])), (name, "t")
        idx = ws[PR.PW_IDX:PR.PW_IDX + 128].view(np.int32)
        assert np.array_equal(idx, tw["idx"]), (name, "slots")
        assert np.array_equal(U.bits32(p), U.bits32(tw["prio"])), (name, "prio: fresh fill and sentinel")
        assert (ws[R.per_workspace_floats(cap):] == -3.0).all() and d_pmax.item() == f32(case["pmax"]), name
        w = ws[PR.PW_W:PR.PW_W + 128]
        w64 = PR.weights(n, p[tw["slots"]], ws[PR.PW_T], case["beta"], b, np.float64)
        err = float(np.abs(w[:b] / w64[:b] - 1).max())
        worst = max(worst, err)
        assert err < WEIGHT_TOL and not w[b:].any() and w[:b].max() == 1, (name, err)
        if case["beta"] == 0.0:
            assert (w[:b] == 1).all(), name
    print("importance weights, worst relative error against float64:", worst)


# ------------------------------------------------------------------ the pin --
@pytest.mark.parametrize("batch", [1, 17, 120, 128])
def test_given_slots_with_unit_weights_leave_replays_bytes(batch):
    """shems_ddpg_update_given with d_idx = shems_ddpg_sample_indices(seed, tick) and weights of 1.0: three updates leave
    Agent.replay's bytes in every learner array and in losses."""
    torch, S, D, ag, ring, _, h, _ = _setup(batch)
    _, _, _, ag2, _, _ = TD._setup()
    ag2.batch = batch
    for tick in range(3):
        ag.replay(ring, tick=tick)
        ag2.replay_given(ring, *_given(torch, ag2.sample_indices(tick, len(ring)).astype(np.int32), batch))
    torch.cuda.synchronize()
    for k in LEARNER_ARRAYS:
        assert torch.equal(getattr(ag, k).view(torch.int32), getattr(ag2, k).view(torch.int32)), (batch, k)
    assert ag2.updates == 3 and ag2.bp_critic == ag.bp_critic and ag2.bp_actor == ag.bp_actor


@pytest.mark.parametrize("batch", [1, 17, 120, 128])
def test_beta_zero_is_the_given_update_on_the_twins_slots(batch):
    """beta = 0: every weight is exactly 1, so Agent.replay on a PrioritizedRing leaves the bytes of shems_ddpg_update_given on the
    twin's slots (drawn from the device's priorities as they stand before each update) with weights 1."""
    torch, S, D, ag, ring, pr, h, _ = _setup(batch, beta=0.0)
    _, _, _, ag2, _, _ = TD._setup()
    ag2.batch = batch
    for tick in range(3):
        p, pmax = pr.prio.cpu().numpy(), pr.pmax.item()
        tw = PR.sample(p, pmax, pr.capacity, len(pr), 0, 0, ag.rng_seed, tick, batch, 0.0)
        ag.replay(pr, tick=tick)
        assert np.array_equal(pr.sampled.cpu().numpy(), tw["idx"]) and (pr.weights.cpu().numpy()[:batch] == 1).all()
        ag2.replay_given(ring, *_given(torch, tw["idx"], batch))
    torch.cuda.synchronize()
    for k in LEARNER_ARRAYS:
        assert torch.equal(getattr(ag, k).view(torch.int32), getattr(ag2, k).view(torch.int32)), (batch, k)


# ------------------------------------------------------------------ every stage --
def _tied_units(p, x):
    _, (_, z1, _, z2, _, _) = DO.mlp_forward(p, x, 11, 1, False, keep=True, dtype=np.float64)
    out = []
    for z, off in ((z1, 11 * 250), (z2, 11 * 250 + 250 + 250 * 500)):
        for u in np.unique(np.where(np.abs(z) < TIE)[1]):
            col = z[:, u]
            out.append((off + int(u), float(np.sign(col[np.argmin(np.abs(col))]) or 1.0)))
    return out


def _assert_critic_blocks(g, P, s, a, y, w, what, expect_ties=()):
    """tests/test_td3_gpu.py's handling of tied relus: a block that fails on one is compared again with that unit decided the other
    way, and the list of such units is asserted exactly."""
    g64 = P.critic_grad_w(s, a, y, w, dtype=np.float64)[0]
    try:
        errs = TD._assert_blocks(g, g64, 11, 1, what)
        tied = []
    except AssertionError:
        tied = _tied_units(P.critic, np.concatenate([DO.normalize(s, P.s_min, P.s_max), a], 1))
        if not tied or len(tied) > 3:
            raise
        keep = P.critic
        flipped = keep.astype(np.float64)
        for i, sg in tied:
            flipped[i] -= sg * 4 * TIE
        P.critic = flipped
        try:
            g64 = P.critic_grad_w(s, a, y, w, dtype=np.float64)[0]
        finally:
            P.critic = keep
        errs = TD._assert_blocks(g, g64, 11, 1, what + " (tied relus decided the other way)")
    assert [i for i, _ in tied] == list(expect_ties), (what, tied)
    return errs


@pytest.mark.parametrize("name,cap,batch,kind,want_dup", PC.update_cases(), ids=[c[0] for c in PC.update_cases()])
def test_every_stage_from_the_devices_previous_stage(name, cap, batch, kind, want_dup):
    """The rings of tests/per_cases.py:update_cases (tests/test_per_host.py asserts on the twin what each covers): priorities over four
    decades on the 24 000-slot ring at the four batches, where no column shares a slot, and five heavy slots on a 1 000-slot ring, where
    some columns share a slot and others do not -- the write-back's scan for the highest column works on a mixed batch.  beta = 0.4: y and q against the oracle (test_ddpg_gpu's bounds), dq = 2 w diff / batch from
    the device's w and diff exactly, every gradient block within BLOCK_TOL of float64, ADAM and the soft updates from the kernel's own
    gradient at 1e-7, losses[0] against the weighted mean, the write-back from the device's diff, pmax upwards only, every slot not
    drawn untouched, the ring's arrays untouched."""
    torch, S, D, ag, ring, pr, h, prio0 = _setup(batch, cap=cap, kind=kind)
    assert PC.UPDATE_SEED == 11
    ring_snap = {k: getattr(pr, k).clone() for k in RING_ARRAYS}
    tick = 3
    ag.replay(pr, tick=tick)
    torch.cuda.synchronize()
    idx, w = pr.sampled.cpu().numpy(), pr.weights.cpu().numpy()
    tw = PR.sample(prio0.copy(), 1.0, pr.capacity, len(pr), 0, 0, ag.rng_seed, tick, batch, 0.4)
    assert np.array_equal(idx, tw["idx"]) and w[:batch].max() == 1 and not w[batch:].any()
    assert batch == 1 or w[:batch].min() < 0.5              # (one live column: its weight is the maximum, 1)
    j, wl = idx[:batch].astype(np.int64), w[:batch]
    assert (len(np.unique(j)) < batch) == want_dup
    s, a, r, s2, done = (h[k][j] for k in ("s", "a", "r", "s2", "done"))
    P = PR.PerLearner(h["pa"], h["pc"], h["s_min"], h["s_max"])
    ws = ag.ws.cpu().numpy()
    y_dev, q_dev, dq_dev = ws[WS_Y:WS_Y + batch], ws[WS_Q:WS_Q + batch], ws[WS_D3C:WS_D3C + 128]
    np.testing.assert_allclose(y_dev, P.targets(r, s2, done.astype(bool)), rtol=2e-5, atol=2e-5)
    sn = DO.normalize(s, h["s_min"], h["s_max"])
    np.testing.assert_allclose(q_dev, DO.critic_forward(h["pc"], sn, a), rtol=2e-5, atol=2e-5)
    diff = (q_dev - y_dev).astype(f32)
    assert np.array_equal(U.bits32(dq_dev[:batch]), U.bits32(((f32(2) * wl).astype(f32) * diff).astype(f32) / f32(batch))) and not dq_dev[batch:].any()
    losses = ag.losses.cpu().numpy()
    lw = float(np.sum(wl.astype(np.float64) * diff.astype(np.float64) ** 2) / batch)
    assert abs(losses[0] - lw) < 1e-5 * max(1.0, abs(lw))
    gc = ag.grad_critic.cpu().numpy()
    errs = {"critic": _assert_critic_blocks(gc, P, s, a, y_dev, wl, f"critic gradient, {name}")}
    opt = DO.Adam(len(gc), DO.ETA_CRIT)
    pc1 = opt.step(h["pc"], gc)
    crit = ag.critic.cpu().numpy()
    np.testing.assert_allclose(crit, pc1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.critic_t.cpu().numpy(), DO.soft_update(h["pc"], crit), rtol=0, atol=1e-7)
    P.critic = crit
    ga = ag.grad_actor.cpu().numpy()
    ga64, la64 = P.actor_grad(s, dtype=np.float64)
    errs["actor"] = TD._assert_blocks(ga, ga64, 9, 2, f"actor gradient, {name}")
    assert abs(losses[1] - la64) < 1e-4 * max(1.0, abs(la64))
    act = ag.actor.cpu().numpy()
    np.testing.assert_allclose(act, DO.Adam(len(ga), DO.ETA_ACT).step(h["pa"], ga), rtol=0, atol=1e-7)
    np.testing.assert_allclose(ag.actor_t.cpu().numpy(), DO.soft_update(h["pa"], act), rtol=0, atol=1e-7)
    # write-back
    p1 = pr.prio.cpu().numpy()
    p64 = PR.new_priority(diff, pr.eps, pr.alpha, np.float64)
    last = {int(slot): m for m, slot in enumerate(j)}                  # the highest column of each drawn slot
    err = max(abs(float(p1[slot]) / p64[m] - 1) for slot, m in last.items())
    print(f"{name}: new priorities, worst relative error against float64: {err}; per-block gradient errors: {errs}")
    assert err < PRIO_TOL
    untouched = np.ones(pr.capacity, bool)
    untouched[j] = False
    assert np.array_equal(U.bits32(p1[untouched]), U.bits32(prio0[untouched]))
    pm = pr.pmax.item()
    assert pm == max(1.0, max(float(p1[slot]) for slot in last)) and pm >= 1.0
    for k in RING_ARRAYS:
        assert torch.equal(getattr(pr, k), ring_snap[k]), k


def test_one_slot_ring_takes_the_highest_columns_priority():
    """ring_len = capacity = 1: all 17 columns draw slot 0 and the write lands as ONE value, column 16's (tests/test_per_host.py holds the
    highest-column rule on the twin with distinct values: on the device, columns that drew one slot hold one transition and one diff)."""
    torch, S, D, ag, ring, pr, h, _ = _setup(17, cap=1, kind="random")
    ag.replay(pr, tick=0)
    torch.cuda.synchronize()
    assert (pr.sampled.cpu().numpy()[:17] == 0).all() and (pr.weights.cpu().numpy()[:17] == 1).all()
    ws = ag.ws.cpu().numpy()
    diff = (ws[WS_Q:WS_Q + 17] - ws[WS_Y:WS_Y + 17]).astype(f32)
    p64 = PR.new_priority(diff, pr.eps, pr.alpha, np.float64)
    assert abs(pr.prio.item() / p64[16] - 1) < PRIO_TOL            # (one transition in every column: the 17 candidates agree)
    assert pr.pmax.item() >= max(1.0, pr.prio.item())


def test_two_runs_leave_the_same_bytes():
    out = []
    for _ in range(2):
        torch, S, D, ag, ring, pr, h, _ = _setup(120)
        for tick in range(3):
            ag.replay(pr, tick=tick)
        torch.cuda.synchronize()
        out.append([getattr(ag, k).clone() for k in LEARNER_ARRAYS] + [pr.prio.clone(), pr.pmax.clone(), pr.ws.clone()])
    for x, y in zip(*out):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_training_on_a_fixed_ring_reduces_the_critic_loss():
    """The learnable reward of tests/test_ddpg_gpu.py, every transition fresh at the first update, beta = 0.4: the weighted loss of
    the last four updates is under half of the first four's, as the uniform and the TD3 tests assert it."""
    torch, S, D, ag, ring, pr, h, _ = _setup(120, seed=2, boost=1.0)
    r = (0.4 * (h["s"][:, 4] - h["s"][:, 3]) + h["a"][:, 1] - 0.5 * h["s"][:, 0]).astype(f32)
    pr.r.copy_(torch.from_numpy(r))
    pr.covered = 0
    first = last = 0.0
    n_up = 160
    pmax = 1.0
    for t in range(n_up):
        ag.replay(pr, tick=t)
        if t < 4:
            first += ag.losses[0].item() / 4
        if t >= n_up - 4:
            last += ag.losses[0].item() / 4
        if t % 40 == 0:
            assert pr.pmax.item() >= pmax
            pmax = pr.pmax.item()
    print("weighted critic loss, first four / last four updates:", first, last)
    assert np.isfinite(last) and last < 0.5 * first, (first, last)
    assert torch.isfinite(ag.actor).all() and torch.isfinite(ag.critic).all() and torch.isfinite(pr.prio).all() and (pr.prio >= 0).all()


def test_pushed_slots_receive_pmax():
    """Four updates with one push between them: exactly the pushed slot is filled with pmax (unless the same update drew it and wrote
    its new priority back)."""
    torch, S, D, ag, ring, pr, h, prio0 = _setup(17, cap=1000)
    for t in range(4):
        slot = pr.pos
        pr.pushed += 1                                                  # (the transition is already there)
        before, pmax = pr.prio.cpu().numpy(), f32(pr.pmax.item())
        assert pr.fresh_range() == (slot, 1)
        ag.replay(pr, tick=t)
        after, drawn = pr.prio.cpu().numpy(), set(pr.sampled.cpu().numpy()[:17].tolist())
        assert pr.covered == pr.pushed and pr.fresh_range()[1] == 0
        assert slot in drawn or after[slot] == pmax
        same = np.ones(1000, bool)
        same[list(drawn) + [slot]] = False
        assert np.array_equal(U.bits32(after[same]), U.bits32(before[same]))


def test_training_loop_runs_on_a_prioritized_ring():
    """episode_ and a short run_episodes are the Agent's own: a ring filled by populate_memory is all fresh at its first update."""
    torch = pytest.importorskip("torch")
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    tab = S.tables.synthetic_table("train", 98)
    mk = lambda n: S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    env, env_eval = mk(256), mk(100)
    ag = D.Agent(seed=1231)
    ring = D.PrioritizedRing(24000)
    ag.populate_memory(env, ring)
    ag.min_max_buffer(ring)
    assert ring.fresh_range() == (0, 24000)
    ret = ag.episode_(env, ring, train=True, rng_ep=7, episode=1)
    assert ret.shape == (256,) and torch.isfinite(ret).all() and ag.updates == 72 and ring.covered == ring.pushed
    assert (ring.prio > 0).all() and ring.pmax.item() >= 1.0
    total, score, best_run, best_actor = ag.run_episodes(env, env_eval, ring, 2, test_every=100, test_runs=100, anneal_beta_from=0.4)
    assert np.isfinite(total).all() and best_actor is not None and ag.updates == 216 and ring.beta == 1.0     # (the last episode runs at beta = 1)
    for k in LEARNER_ARRAYS:
        assert torch.isfinite(getattr(ag, k)).all(), k
    assert torch.isfinite(ring.prio).all()


def test_c_abi_refusals():
    """SHEMS_ERR_ARG / SHEMS_ERR_STATE with nothing launched: a canary over prio, the workspace and the learner's arrays."""
    torch, S, D, ag, ring, pr, h, _ = _setup(120, cap=1000)
    R = _R()
    L = R._declare_per()
    rs = pr.struct()
    pr.ws.fill_(-3.0)
    snap = _snap(ag)
    canary = [pr.prio.clone(), pr.pmax.clone(), pr.ws.clone(), ag.ws.clone()]
    ARG, STATE = S._capi.ERR_ARG, S._capi.ERR_STATE

    def call(d=None, per=None, ring_len=1000, fresh=(0, 0), bp=0.9):
        d = ag._ddpg_args() if d is None else d
        per = pr.per_struct() if per is None else per
        return L.shems_ddpg_update_per(C.byref(d), C.byref(rs), C.byref(per), ring_len, fresh[0], fresh[1], 11, 0, ag.eta_crit, bp, 0.999,
                                       ag.eta_act, 0.9, 0.999, ag._stream())

    def per(**kw):
        p = pr.per_struct()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    d = ag._ddpg_args()
    d.batch = 129
    assert call(d=d) == ARG and call(bp=1.0) == ARG                    # what shems_ddpg_update refuses
    d = ag._ddpg_args()
    d.critic = None
    assert call(d=d) == ARG
    for k in ("prio", "pmax", "ws"):
        assert call(per=per(**{k: None})) == ARG, k
    assert call(per=per(prio=pr.prio.data_ptr() + 4)) == ARG and call(per=per(ws=pr.ws.data_ptr() + 8)) == ARG
    assert call(per=per(pmax=pr.pmax.data_ptr() + 2)) == ARG
    assert call(per=per(ws=pr.prio.data_ptr())) == ARG and call(per=per(pmax=pr.prio.data_ptr() + 64)) == ARG
    assert call(per=per(pmax=pr.ws.data_ptr() + 16)) == ARG and call(per=per(prio=ag.ws.data_ptr())) == ARG
    for bad in (-0.1, float("nan"), float("inf")):
        for k in ("alpha", "beta", "eps_p"):
            assert call(per=per(**{k: bad})) == ARG, (k, bad)
    assert call(per=per(beta=1.5)) == ARG and "beta" in L.shems_last_error().decode()
    assert call(ring_len=0) == ARG and call(ring_len=1001) == ARG
    assert call(fresh=(-1, 1)) == ARG and call(fresh=(1000, 1)) == ARG and call(fresh=(0, -1)) == ARG
    assert call(ring_len=600, fresh=(590, 20)) == ARG                  # leaves the filled slots of a ring not yet full
    idx, w = _given(torch, np.zeros(120, np.int32), 120)
    given = lambda i, ww, n=1000: L.shems_ddpg_update_given(C.byref(ag._ddpg_args()), C.byref(rs), n, i, ww, ag.eta_crit, 0.9, 0.999,
                                                            ag.eta_act, 0.9, 0.999, ag._stream())
    assert given(None, w.data_ptr()) == ARG and given(idx.data_ptr(), None) == ARG and given(idx.data_ptr(), w.data_ptr(), 1001) == ARG
    sample = lambda p, cap=1000, n=1000, b=120: L.shems_per_sample_dev(C.byref(p), cap, n, 0, 0, 11, 0, b, None)
    assert sample(per(), b=0) == ARG and sample(per(), b=129) == ARG and sample(per(), cap=262145, n=1000) == ARG and sample(per(prio=None)) == ARG
    # a learner on the tiled working layout
    _, _, _, ag0, ring0, _ = TD._setup()
    ag0.use_tiled(True)
    ag0.replay(ring0, tick=0)
    assert ag0._tiled_current
    assert call(d=ag0._ddpg_args(raw=True)) == STATE
    ag0.use_tiled(False)
    torch.cuda.synchronize()
    for k in LEARNER_ARRAYS:
        assert torch.equal(getattr(ag, k), snap[k]), k
    for x, y in zip((pr.prio, pr.pmax, pr.ws, ag.ws), canary):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert call() == S._capi.OK                                        # and the unmodified record runs
    torch.cuda.synchronize()


def test_entry_script_trains_on_a_prioritized_ring_under_a_case_of_its_own(tmp_path):
    """SHEMS_REPLAY=per writes its files under the suffixed case; unset, the case is DDPG's.  beta reaches 1.0 in the last episode."""
    pytest.importorskip("torch")
    import os
    M = importlib.import_module(U.PKG_NAME + ".main")
    base = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_NUM_ENVS": "64",
            "SHEMS_SYNTHETIC_DATA": "1"}
    ddpg_case = M.config_from_env(base).case
    cwd0 = os.getcwd()
    with pytest.raises(ValueError, match="SHEMS_REPLAY"):              # refused by name before any device work or file
        M.main(dict(base, SHEMS_REPLAY="rank"), cwd=str(tmp_path / "nowhere"), log=lambda *_: None)
    with pytest.raises(NotImplementedError, match="SHEMS_REPLAY=per with SHEMS_ALGO=td3"):
        M.main(dict(base, SHEMS_REPLAY="per", SHEMS_ALGO="td3"), cwd=str(tmp_path / "nowhere"), log=lambda *_: None)
    assert os.getcwd() == cwd0 and not (tmp_path / "nowhere").exists()
    try:
        cfg, written = M.main(dict(base, SHEMS_REPLAY="per:0.6"), cwd=str(tmp_path), log=lambda *_: None)
    finally:
        os.chdir(cwd0)
    assert cfg.case == ddpg_case + "_per-a0.6-b0.4"
    stem = f"DDPG_Shems_Charger_v1_72_2_250_500_{cfg.case}_1231"
    for f in (f"out/bson/{stem}_actor_2.bson", f"out/bson/{stem}_scores_2.bson", f"out/bson/temp/{stem}_actor_1.bson"):
        assert (tmp_path / f).exists(), f
    assert len(written) == 2 and all(cfg.case in w for w in written)
    assert M.config_from_env(base).case == ddpg_case and "per" not in ddpg_case and M.replay_from_env(base) == ("uniform", None)

"""Prioritized replay for learner groups on the GPU: group.PrioritizedLearnerGroup / shems_ddpg_group_update_per_tp and
shems_per_group_sample_dev (csrc/shems_gupd.hip) against the NumPy twin (tests/per_ref.py with the key seed + l) and float64, per
learner, each stage from the device's own previous stage.

Cases, rings and ticks live in tests/group_per_cases.py (tests/test_group_per_host.py proves on the CPU that they hold what is asserted
here).  Bounds: the sampler's u, t, S_b, C_b, T, slots and fresh fill bit for bit; importance weights and new priorities against float64
under tests/test_per_gpu.py's bounds (6.7e-7 and 3.4e-7 relative); y and q rtol = atol = 2e-5 (tests/test_group_td3_gpu.py's); dq from the
device's w and diff exactly; every Flux.params block of a gradient BLOCK_TOL = 2e-6 of its float64 max-abs; losses 1e-5 / 1e-4 max(1,
|loss|); ADAM, targets and moments from the kernel's own gradient with tests/test_group_gpu.py's bounds (atol 1e-7; moments rtol 1e-6)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ddpg_oracle as DO
import group_per_cases as K
import per_cases as PC
import per_ref as PR
import util as U

pytestmark = pytest.mark.gpu
f32 = np.float32

BLOCK_TOL = 2e-6
WEIGHT_TOL, PRIO_TOL = min(4 * 1.67e-7, 1e-5), min(4 * 8.4e-8, 1e-5)        # tests/test_per_gpu.py's bounds
E, CAP = K.E, K.CAP
DDPG_SIDE = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic", "losses")
PER_BLOCKS = ("per_prio", "per_pmax", "per_ws")
RING_BLOCKS = ("ring_s", "ring_a", "ring_r", "ring_s2", "ring_done")
TP_D3C, TP_PER_PUB = 33160, 165000       # dq [2][128] of the throughput carve; y, q [2][128] (SHEMS_TP_PER_PUB)


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    return torch, S, mod("ddpg"), mod("group")


def _fill(torch, grp, l, reward=None):
    d = K.learner_data(l)
    ag, ring = grp.learners[l], grp.rings[l]
    up = lambda t, v: t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    ag.set_norm(d["s_min"], d["s_max"])
    for k in ("s", "a", "r", "s2", "done"):
        up(getattr(ring, k), d[k] if (k != "r" or reward is None) else reward(d))
    ring.pushed = CAP
    ag.set_params(actor=d["pa"], critic=d["pc"])
    up(ag.actor_t, d["pa_t"])
    up(ag.critic_t, d["pc_t"])
    return d, up


def _group(L, batch=120, tiled=None, hparams=None, reward=None, prio=True, **kw):
    """An L-learner prioritized group on tests/group_per_cases.py's data: full rings, every priority set (no fresh range)."""
    torch, S, D, G = _mods()
    grp = G.PrioritizedLearnerGroup(L, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=CAP, tiled=tiled, hparams=hparams, **kw)
    grp.store_grad = True
    for l, ag in enumerate(grp.learners):
        d, up = _fill(torch, grp, l, reward)
        if hparams is None:
            ag.batch = batch
        if prio:
            up(grp.prio_of(l), K.priorities(l))
    grp.covered = CAP if prio else 0
    if grp.tiled:
        grp.flux_changed()
    return torch, grp


def _ddpg_group(L, batch=120, tiled=None, hparams=None):
    torch, S, D, G = _mods()
    grp = G.LearnerGroup(L, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=CAP, form="throughput", tiled=tiled, hparams=hparams)
    grp.store_grad = True
    for l, ag in enumerate(grp.learners):
        _fill(torch, grp, l)
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


# ----------------------------------------------------------------------------------------------------- 1. the sampler --
def _assert_draw(name, ws, p, tw, n, b, beta):
    """One learner's published draw (ws: its sampler workspace, p: its priorities after the launch) against the twin `tw`."""
    nb = PR.n_blocks(n)
    assert U.bits32(ws[PR.PW_T:PR.PW_T + 1])[0] == U.bits32(np.array([tw["T"]], f32))[0], (name, "T")
    assert ws[PR.PW_T + 2:PR.PW_T + 3].view(np.int32)[0] == nb, name
    assert np.array_equal(U.bits32(ws[PR.PW_S:PR.PW_S + nb]), U.bits32(tw["S"])), (name, "S")
    assert np.array_equal(U.bits32(ws[PR.PW_S + nb:PR.PW_S + 2 * nb]), U.bits32(tw["C"])), (name, "C")
    assert np.array_equal(U.bits32(ws[PR.PW_U:PR.PW_U + 128]), U.bits32(tw["u"])), (name, "u")
    assert np.array_equal(U.bits32(ws[PR.PW_TM:PR.PW_TM + 128]), U.bits32(tw["t"])), (name, "t")
    idx = ws[PR.PW_IDX:PR.PW_IDX + 128].view(np.int32)
    assert np.array_equal(idx, tw["idx"]), (name, "slots")
    assert np.array_equal(U.bits32(p), U.bits32(tw["prio"])), (name, "prio: fresh fill and sentinel")
    w = ws[PR.PW_W:PR.PW_W + 128]
    w64 = PR.weights(n, p[tw["slots"]], ws[PR.PW_T], beta, b, np.float64)
    err = float(np.abs(w[:b] / w64[:b] - 1).max())
    assert err < WEIGHT_TOL and not w[b:].any() and w[:b].max() == 1, (name, err)
    if beta == 0.0:
        assert (w[:b] == 1).all(), name
    return err


def _sample_case(torch, S, grp, name, case, learners):
    """Runs shems_per_group_sample_dev on `case` with the case's priorities (a generator per learner) in `learners`' slabs."""
    cap, n, b = case["capacity"], case["ring_len"], case["batch"]
    prios = {}
    for l in learners:
        rng = np.random.default_rng(1000 * l + n + 13 * b)
        prios[l] = PC.priorities(case["kind"], cap, n, rng)
        full = np.full(grp.capacity, f32(-9.25), f32)
        full[:cap] = prios[l]
        grp.prio_of(l).copy_(torch.from_numpy(full))
        grp.pmax_of(l).fill_(case["pmax"])
        grp._view(l, "per_ws").fill_(-3.0)
    per = grp.per_struct()
    per.beta = case["beta"]
    g = grp.struct()
    S._capi.check(grp.LP.shems_per_group_sample_dev(C.byref(per), C.byref(g), None, cap, n, case["fresh"][0], case["fresh"][1], case["seed"],
                                                    case["tick"], b, grp._stream()))
    torch.cuda.synchronize()
    worst = 0.0
    for l in learners:
        p = prios[l].copy()
        tw = PR.sample(p, case["pmax"], cap, n, case["fresh"][0], case["fresh"][1], case["seed"] + l, case["tick"], b, case["beta"])
        tw["prio"] = p
        ws, pd = _np(grp, l, "per_ws"), _np(grp, l, "per_prio")
        worst = max(worst, _assert_draw(f"{name}, learner {l}", ws, pd[:cap], tw, n, b, case["beta"]))
        assert (pd[cap:] == f32(-9.25)).all() and grp.pmax_of(l).item() == f32(case["pmax"]), name
        used = PR.PW_S + 2 * PR.n_blocks(n)
        assert (ws[used:] == -3.0).all(), (name, "workspace behind the published block")
    return worst


@pytest.mark.parametrize("L", [2, 48])
def test_group_sampler_equals_the_twin_on_the_ring_and_batch_edges(L):
    """Every case of tests/per_cases.py that fits a 1 000-slot slab (ring_len 1 / 255 / 256 / 257 / 1 000 x batch 1 / 17 / 120 / 128;
    exact zeros, one slot, the last partial block, four decades; fresh ranges empty / one / wrapping / >= capacity with pmax != 1;
    beta = 0), for learners 0 and L - 1 with the keys seed and seed + L - 1: u, t, every S_b / C_b, T, the slots and the fresh fill equal
    the twin exactly, the weights are held to float64 from the device's own T and pi."""
    torch, S, D, G = _mods()
    grp = G.PrioritizedLearnerGroup(L, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=CAP)
    worst = 0.0
    for name, case in K.sampler_edge_cases():
        worst = max(worst, _sample_case(torch, S, grp, name, case, K.checked(L)))
    # every priority zero: the draw falls back to block 0 and its last slot, the weights to 1
    zero = dict(capacity=CAP, ring_len=CAP, batch=17, kind="one_slot", fresh=(0, 0), pmax=1.0, beta=0.4, seed=5, tick=9)
    for l in K.checked(L):
        grp.prio_of(l).zero_()
        grp.pmax_of(l).fill_(1.0)
    per, g = grp.per_struct(), grp.struct()
    S._capi.check(grp.LP.shems_per_group_sample_dev(C.byref(per), C.byref(g), None, CAP, CAP, 0, 0, zero["seed"], zero["tick"], 17, grp._stream()))
    torch.cuda.synchronize()
    for l in K.checked(L):
        tw = PR.sample(np.zeros(CAP, f32), 1.0, CAP, CAP, 0, 0, zero["seed"] + l, zero["tick"], 17, 0.4)
        assert np.array_equal(grp.sampled_of(l).cpu().numpy(), tw["idx"]) and (grp.weights_of(l).cpu().numpy()[:17] == 1).all()
        assert (tw["idx"][:17] == PR.BLOCK - 1).all() and not grp.prio_of(l).any()
    print(f"L={L}: importance weights, worst relative error against float64: {worst}")


def test_group_sampler_on_a_24000_slot_ring_and_with_records():
    """One 24 000-slot ring at L = 2 (94 blocks, three rounds of loads), and two learners with their own batch from the records: the
    first batch_l columns are live, t_m = (m + u_m) (T_l / batch_l), the weight maximum runs over learner l's live columns."""
    torch, S, D, G = _mods()
    big = G.PrioritizedLearnerGroup(2, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=K.BIG["capacity"])
    w = _sample_case(torch, S, big, "decades-24000", K.BIG, (0, 1))
    del big
    torch, grp = _group(2, hparams=K.RECORD_CASE)
    grp.per_sample(tick=K.TICKS[0], batch=99)                                       # (with records `batch` is ignored)
    torch.cuda.synchronize()
    for l, rec in enumerate(K.RECORD_CASE):
        tw, p = K.draw(l, K.TICKS[0], rec["batch"])
        tw["prio"] = p
        w = max(w, _assert_draw(f"records, learner {l}", _np(grp, l, "per_ws"), _np(grp, l, "per_prio"), tw, CAP, rec["batch"], K.BETA))
    assert grp.covered == CAP and grp.updates == 0
    print("worst relative weight error:", w)


# ------------------------------------------------------------------------------------------------------------ 2. the pin --
def _uniform_given(torch, grp, tick, batches):
    idx = np.full((grp.count, 128), -1, np.int32)
    for l, b in enumerate(batches):
        idx[l, :b] = DO.sample_indices(K.RNG_SEED + l, tick, b, CAP)
    return torch.from_numpy(idx).to(grp.device), torch.ones((grp.count, 128), dtype=torch.float32, device=grp.device)


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("L", [2, 48])
def test_given_uniform_slots_with_unit_weights_leave_replays_bytes(L, tiled, records):
    """SHEMS_TP_PER_GIVEN on the uniform sampler's indices (shems_ddpg_sample_indices(seed + l, tick)) with weights of 1.0, three
    updates: every learner array and losses hold LearnerGroup.replay()'s bytes from the same state, ring, seed and ticks -- every
    rounding of the new instantiations is an old one -- and prio / pmax are untouched."""
    hp = [{"batch": 120} for _ in range(L)] if records else None
    torch, ref = _ddpg_group(L, tiled=tiled, hparams=hp)
    torch, grp = _group(L, tiled=tiled, hparams=hp)
    assert grp.tiled == tiled and ref.tiled == tiled and grp.form == "throughput"
    assert grp.slab_floats > ref.slab_floats and all(grp.layout[k] == ref.layout[k] for k in ref.layout)
    before = {k: _bits(grp, k) for k in ("per_prio", "per_pmax")}
    for t in range(3):
        ref.replay(tick=t)
        grp.replay_given(*_uniform_given(torch, grp, t, [120] * L))
    torch.cuda.synchronize()
    a, b = _side(grp, DDPG_SIDE), _side(ref, DDPG_SIDE)
    for k in DDPG_SIDE:
        assert torch.equal(a[k], b[k]), k
    for k in before:
        assert torch.equal(before[k], _bits(grp, k)), k
    assert grp.updates == ref.updates == 3 and grp.covered == CAP
    for x, y in zip(grp.learners, ref.learners):
        assert x.bp_actor == y.bp_actor and x.bp_critic == y.bp_critic and x.updates == 3
    assert float(grp.learners[L - 1].grad_critic[:3000].abs().max()) > 0 and float(grp.learners[L - 1].grad_actor[:2500].abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------- 3. beta = 0 --
@pytest.mark.parametrize("L", [2, 48])
def test_beta_zero_is_the_given_update_on_the_twins_slots(L):
    """beta = 0: every weight is exactly 1, so replay() leaves the bytes of replay_given on the twin's slots (drawn from the device's
    priorities as they stand before each update) with weights 1 -- and the priorities are written."""
    torch, grp = _group(L, beta=0.0)
    torch, giv = _group(L)
    p0 = _bits(grp, "per_prio")
    for tick in K.TICKS:
        idx = np.full((L, 128), -1, np.int32)
        for l in range(L):
            tw = PR.sample(grp.prio_of(l).cpu().numpy(), grp.pmax_of(l).item(), CAP, CAP, 0, 0, K.RNG_SEED + l, tick, 120, 0.0)
            idx[l] = tw["idx"]
        grp.replay(tick=tick)
        torch.cuda.synchronize()
        for l in range(L):
            assert np.array_equal(grp.sampled_of(l).cpu().numpy(), idx[l]), (tick, l)
            assert (grp.weights_of(l).cpu().numpy()[:120] == 1).all()
        giv.replay_given(torch.from_numpy(idx).to(giv.device), torch.ones((L, 128), dtype=torch.float32, device=giv.device))
    torch.cuda.synchronize()
    a, b = _side(grp, DDPG_SIDE), _side(giv, DDPG_SIDE)
    for k in DDPG_SIDE:
        assert torch.equal(a[k], b[k]), k
    p1 = _bits(grp, "per_prio")
    assert all(not torch.equal(p0[l], p1[l]) for l in range(L))
    assert torch.equal(_bits(giv, "per_prio"), p0)


# ---------------------------------------------------------------------------------------------------- 4. every stage --
def _host_state(l, eta_crit=DO.ETA_CRIT, eta_act=DO.ETA_ACT):
    d = K.learner_data(l)
    return dict(pa=d["pa"].copy(), pa_t=d["pa_t"].copy(), pc=d["pc"].copy(), pc_t=d["pc_t"].copy(), opt_c=DO.Adam(len(d["pc"]), eta_crit),
                opt_a=DO.Adam(len(d["pa"]), eta_act), prio=np.array(K.priorities(l)), pmax=f32(1.0))


def _blocks_or_the_other_relu_decision(g, evaluate, nets, in_dim, out_dim, what):
    """tests/test_group_td3_gpu.py's: a failing block is evaluated again with every tied relu (|z| < K.TIE) decided the other way."""
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


def _check_update(grp, l, h, tick, B, beta, gamma=DO.GAMMA, worst=None):
    """Learner l's last update (already on the device, Flux order current) from the host copy `h` of the state it started from; `h`
    then takes the device's bytes.  Returns the ties set aside."""
    d = K.learner_data(l)
    ag = grp.learners[l]
    what = f"learner {l}, tick {tick}, B={B}"
    # steps 1-4 from the priorities the device held before the update
    p_before = h["prio"].copy()
    tw = PR.sample(p_before, h["pmax"], CAP, CAP, 0, 0, K.RNG_SEED + l, tick, B, beta)
    tw["prio"] = p_before
    ws = _np(grp, l, "per_ws")
    idx, w = grp.sampled_of(l).cpu().numpy(), grp.weights_of(l).cpu().numpy()
    assert np.array_equal(idx, tw["idx"]), what
    for k, o in (("u", PR.PW_U), ("t", PR.PW_TM)):
        assert np.array_equal(U.bits32(ws[o:o + 128]), U.bits32(tw[k])), (what, k)
    nb = PR.n_blocks(CAP)
    assert np.array_equal(U.bits32(ws[PR.PW_S:PR.PW_S + 2 * nb]), U.bits32(np.concatenate([tw["S"], tw["C"]]))), what
    w64 = PR.weights(CAP, p_before[tw["slots"]], ws[PR.PW_T], beta, B, np.float64)
    err_w = float(np.abs(w[:B] / w64[:B] - 1).max())
    assert err_w < WEIGHT_TOL and w[:B].max() == 1 and not w[B:].any(), (what, err_w)
    j, wl = idx[:B].astype(np.int64), w[:B]
    s, a, r, s2, done = K.minibatch(l, j)
    P = K.per_learner(l, h["pa"], h["pc"], h["pa_t"], h["pc_t"])
    # step 5: y, q against the oracle; dq and the loss from the device's own w and diff
    dws = _np(grp, l, "ws")
    y_dev, q_dev, dq_dev = dws[TP_PER_PUB:TP_PER_PUB + B], dws[TP_PER_PUB + 128:TP_PER_PUB + 128 + B], dws[TP_D3C:TP_D3C + 256]
    np.testing.assert_allclose(y_dev, K.target_y(P, r, s2, done, gamma), rtol=2e-5, atol=2e-5)
    sn = DO.normalize(s, d["s_min"], d["s_max"])
    np.testing.assert_allclose(q_dev, DO.critic_forward(h["pc"], sn, a), rtol=2e-5, atol=2e-5)
    diff = (q_dev - y_dev).astype(f32)
    assert np.array_equal(U.bits32(dq_dev[:B]), U.bits32(((f32(2) * wl).astype(f32) * diff).astype(f32) / f32(B))) and not dq_dev[B:].any(), what
    dq64 = 2.0 * wl.astype(np.float64) * (q_dev.astype(np.float64) - y_dev.astype(np.float64)) / B
    assert np.abs(dq_dev[:B] - dq64).max() <= 4 * np.finfo(f32).eps * max(1e-30, np.abs(dq64).max()), what
    loss = float(ag.losses[0])
    lw = float(np.sum(wl.astype(np.float64) * diff.astype(np.float64) ** 2) / B)
    assert abs(loss - lw) < 1e-5 * max(1.0, abs(lw)), (what, loss, lw)
    x = np.concatenate([sn, a], 1)
    ties = []
    gc = _np(grp, l, "grad_critic")

    def crit_eval(Pm):
        Q = K.per_learner(l, h["pa"], Pm["critic"], h["pa_t"], h["pc_t"])
        return Q.critic_grad_w(s, a, y_dev, wl, dtype=np.float64)[0]
    e, tie = _blocks_or_the_other_relu_decision(gc, crit_eval, {"critic": (h["pc"], x, 11, 1)}, 11, 1, f"critic gradient, {what}")
    if tie:
        ties.append(("critic", l, tick))
    errs = {"critic_" + k: v for k, v in e.items()}
    pc1 = h["opt_c"].step(h["pc"], gc)                                           # ADAM from the kernel's own gradient
    crit, crit_t = _np(grp, l, "critic"), _np(grp, l, "critic_t")
    np.testing.assert_allclose(crit, pc1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(_np(grp, l, "m_critic"), h["opt_c"].m, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(_np(grp, l, "v_critic"), h["opt_c"].v, rtol=1e-6, atol=1e-15)
    np.testing.assert_allclose(crit_t, DO.soft_update(h["pc_t"], crit), rtol=0, atol=1e-7)
    h["opt_c"].m, h["opt_c"].v = _np(grp, l, "m_critic").astype(h["opt_c"].m.dtype), _np(grp, l, "v_critic").astype(h["opt_c"].v.dtype)
    # the actor through the device's UPDATED critic
    ga = _np(grp, l, "grad_actor")
    a_pi = DO.actor_forward(h["pa"], sn, dtype=np.float64)

    def act_eval(Pm):
        return DO.Learner(Pm["actor"], Pm["critic"], d["s_min"], d["s_max"]).actor_grad(s, dtype=np.float64)[0]
    e, tie = _blocks_or_the_other_relu_decision(ga, act_eval, {"actor": (h["pa"], sn, 9, 2), "critic": (crit, np.concatenate([sn, a_pi], 1), 11, 1)},
                                                9, 2, f"actor gradient, {what}")
    if tie:
        ties.append(("actor", l, tick))
    errs.update({"actor_" + k: v for k, v in e.items()})
    _, la64 = DO.Learner(h["pa"], crit, d["s_min"], d["s_max"]).actor_grad(s, dtype=np.float64)
    assert abs(float(ag.losses[1]) - la64) < 1e-4 * max(1.0, abs(la64)), what
    pa1 = h["opt_a"].step(h["pa"], ga)
    act, act_t = _np(grp, l, "actor"), _np(grp, l, "actor_t")
    np.testing.assert_allclose(act, pa1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(act_t, DO.soft_update(h["pa_t"], act), rtol=0, atol=1e-7)
    h["opt_a"].m, h["opt_a"].v = _np(grp, l, "m_actor").astype(h["opt_a"].m.dtype), _np(grp, l, "v_actor").astype(h["opt_a"].v.dtype)
    # step 6: the write-back from the device's diff; the highest column of a shared slot is the writer
    p1 = _np(grp, l, "per_prio")
    p64 = PR.new_priority(diff, grp.eps, grp.alpha, np.float64)
    last = {int(slot): m for m, slot in enumerate(j)}
    err_p = max(abs(float(p1[slot]) / p64[m] - 1) for slot, m in last.items())
    assert err_p < PRIO_TOL, (what, err_p)
    shared, single = K.duplicates(j)
    for slot in shared:                                                          # a lower column's value is another one, and is not what landed
        cols = np.nonzero(j == slot)[0]
        lower = [m for m in cols[:-1] if abs(p64[m] / p64[cols[-1]] - 1) > 100 * PRIO_TOL]
        assert all(abs(float(p1[slot]) / p64[m] - 1) > PRIO_TOL for m in lower), (what, slot)
    untouched = np.ones(CAP, bool)
    untouched[j] = False
    assert np.array_equal(U.bits32(p1[untouched]), U.bits32(p_before[untouched])), what
    pm = f32(grp.pmax_of(l).item())
    assert pm == max(h["pmax"], max(f32(p1[slot]) for slot in last)) and pm >= h["pmax"], what
    print(f"{what}: weights {err_w:.2e}, new priorities {err_p:.2e} (relative, against float64); shared slots {len(shared)}, single {len(single)}; "
          f"loss {loss!r} vs float64 {lw!r}; per-block gradient errors {errs}")
    if worst is not None:
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    h.update(pa=act.copy(), pa_t=act_t.copy(), pc=crit.copy(), pc_t=crit_t.copy(), prio=p1.copy(), pmax=pm)
    return ties, (len(shared), len(single))


def _check_the_other_learners(grp, before, L):
    """Every learner's undrawn slots keep their bytes, its pmax only moves upwards, and nobody's ring moved."""
    torch = grp.torch
    p0, p1 = before["per_prio"].cpu().numpy(), _bits(grp, "per_prio").cpu().numpy()
    m0, m1 = before["per_pmax"].view(torch.float32).cpu().numpy()[:, 0], _bits(grp, "per_pmax").view(torch.float32).cpu().numpy()[:, 0]
    o = grp.layout["per_ws"][0]
    idx = grp.slab[:, o + PR.PW_IDX:o + PR.PW_IDX + 128].contiguous().view(torch.int32).cpu().numpy()
    for l in range(L):
        keep = np.ones(CAP, bool)
        keep[idx[l][idx[l] >= 0]] = False
        assert np.array_equal(p0[l][keep], p1[l][keep]), l
        assert not np.array_equal(p0[l], p1[l]) and m1[l] >= m0[l] >= 1.0, l
    for k in RING_BLOCKS:
        assert torch.equal(before[k], _bits(grp, k)), k


@pytest.mark.parametrize("L,batch", K.STAGE_CASES)
def test_every_stage_from_the_devices_previous_stage(L, batch):
    """Two updates in a row at beta = 0.4 (the second from the device's own priorities and on the advanced powers), learners 0 -- the
    ring with partial duplicates -- and L - 1."""
    ticks = K.ticks_of((L, batch))
    torch, grp = _group(L, batch)
    assert grp.tiled and grp.beta == K.BETA
    host = {l: _host_state(l) for l in K.checked(L)}
    ties, worst, dups = [], {}, {}
    for tick in ticks:
        before = {k: _bits(grp, k) for k in RING_BLOCKS + ("per_prio", "per_pmax")}
        grp.replay(tick=tick)
        grp.flux_()
        torch.cuda.synchronize()
        for l in K.checked(L):
            t, dups[(l, tick)] = _check_update(grp, l, host[l], tick, batch, K.BETA, worst=worst)
            ties += t
        _check_the_other_learners(grp, before, L)
    print(f"L={L} B={batch}: worst per-block errors {worst}; ties {ties}; (shared, single) slots {dups}")
    assert ties == K.EXPECTED_TIES[(L, batch)], ties
    if batch >= 120:                                                             # the duplicate ring's mixed batch (host test: on the twin)
        assert dups[(K.DUP_LEARNER, ticks[0])][0] >= 3 and dups[(K.DUP_LEARNER, ticks[0])][1] >= 20
    assert grp.updates == 2 and grp.covered == CAP
    for ag in grp.learners:
        assert abs(ag.bp_critic[0] - 0.9 ** 3) < 1e-15 and abs(ag.bp_actor[0] - 0.9 ** 3) < 1e-15


def test_two_learners_with_their_own_batch_eta_and_gamma_meet_their_own_float64():
    torch, grp = _group(2, hparams=K.RECORD_CASE)
    host = {l: _host_state(l, eta_crit=float(np.float32(K.RECORD_CASE[l]["eta_crit"]))) for l in range(2)}
    ties = []
    for tick in K.TICKS:
        grp.replay(tick=tick)
        grp.flux_()
        torch.cuda.synchronize()
        for l, rec in enumerate(K.RECORD_CASE):
            ties += _check_update(grp, l, host[l], tick, rec["batch"], K.BETA, gamma=np.float32(rec["gamma"]))[0]
    assert ties == []


@pytest.mark.parametrize("tiled", [True, False])
def test_layouts_and_uniform_records_leave_the_same_bits(tiled):
    """Two prioritized updates: the Flux-order layout leaves the tiled layout's bits, uniform records the shared scalars'."""
    def run(**kw):
        torch, grp = _group(2, 17, **kw)
        for t in K.TICKS:
            grp.replay(tick=t)
        torch.cuda.synchronize()
        return grp, _side(grp, DDPG_SIDE + PER_BLOCKS)
    g0, a = run(tiled=True)
    g1, b = run(tiled=tiled, hparams=[{"batch": 17}, {"batch": 17}])
    assert g0.tiled and g1.tiled == tiled and g1._hp_dev is not None
    for k in a:
        assert g0.torch.equal(a[k], b[k]), k


# -------------------------------------------------------------------------------------- 5. determinism and isolation --
def test_two_runs_leave_the_same_bytes_and_a_learner_does_not_depend_on_the_others():
    out = []
    for L in (2, 2, 3):
        torch, grp = _group(L, 120)
        for t in K.TICKS:
            grp.replay(tick=t)
        torch.cuda.synchronize()
        out.append(_side(grp, DDPG_SIDE + PER_BLOCKS))
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
        assert torch.equal(out[0][k], out[2][k][:2]), k


# ------------------------------------------------------------------------------------------------------ 6. learning --
def test_training_on_a_fixed_ring_reduces_the_weighted_critic_loss_of_every_learner():
    """The learnable reward of tests/test_per_gpu.py (a function of the stored state and action), every transition fresh at the first
    update, beta = 0.4, 160 updates: the mean weighted loss of the last four updates is below half that of the first four, per learner."""
    reward = lambda d: (0.4 * (d["s"][:, 4] - d["s"][:, 3]) + d["a"][:, 1] - 0.5 * d["s"][:, 0]).astype(np.float32)
    torch, grp = _group(2, 120, reward=reward, prio=False)
    assert grp.fresh_range() == (0, CAP)
    n_up = 160
    first, last = np.zeros(2), np.zeros(2)
    o = grp.layout["losses"][0]
    pmax = np.ones(2, f32)
    for t in range(n_up):
        grp.replay(tick=t)
        if t < 4 or t >= n_up - 4:
            v = grp.slab[:, o].cpu().numpy() / 4
            if t < 4:
                first += v
            else:
                last += v
        if t % 40 == 0:
            pm = np.array([grp.pmax_of(l).item() for l in range(2)], f32)
            assert (pm >= pmax).all()
            pmax = pm
    print("weighted critic losses [learner], first and last four updates:", first, last)
    assert np.isfinite(last).all() and (last < 0.5 * first).all(), (first, last)
    assert grp.updates == n_up and grp.fresh_range()[1] == 0
    grp.flux_()
    for k in DDPG_SIDE + ("per_prio", "per_pmax"):
        oo, n = grp.layout[k]
        assert bool(torch.isfinite(grp.slab[:, oo:oo + n]).all()), k
    assert bool((grp.slab[:, grp.layout["per_prio"][0]:grp.layout["per_prio"][0] + CAP] > 0).all())


# ---------------------------------------------------------------------------------- 7. fresh fill, 8. training runs --
def test_pushed_slots_receive_pmax_through_the_fused_steps_window():
    """Three fused steps that each remember four households per learner: exactly the pushed slots receive that learner's pmax before
    the draw (unless the same update drew one and wrote its new priority back), every other undrawn slot keeps its bytes."""
    torch, S, D, G = _mods()
    L = 2
    torch, grp = _group(L, 17)
    tab = S.tables.synthetic_table("train")
    env = S.ShemsBatch(L * E, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    env.reset_(3, episode=1)
    for l in range(L):
        grp.pmax_of(l).fill_(2.5 + l)
    for t in range(3):
        pos = grp.rings[0].pos
        grp.act_step(env, train=True, tick=t, window=(pos, 4, 4 * t))
        assert grp.fresh_range() == (pos, 4) and all(r.pushed == CAP + 4 * (t + 1) for r in grp.rings)
        before = _bits(grp, "per_prio").view(torch.float32).cpu().numpy()
        pmax = [f32(grp.pmax_of(l).item()) for l in range(L)]
        grp.replay(tick=t)
        torch.cuda.synchronize()
        after = _bits(grp, "per_prio").view(torch.float32).cpu().numpy()
        assert grp.covered == grp.rings[0].pushed and grp.fresh_range()[1] == 0
        for l in range(L):
            drawn = set(grp.sampled_of(l).cpu().numpy()[:17].tolist())
            pushed = [(pos + i) % CAP for i in range(4)]
            for slot in pushed:
                assert slot in drawn or after[l][slot] == pmax[l], (t, l, slot)
            same = np.ones(CAP, bool)
            same[list(drawn) + pushed] = False
            assert np.array_equal(U.bits32(after[l][same]), U.bits32(before[l][same])), (t, l)
    env.close()


def test_run_episodes_anneals_beta_and_the_inherited_calls_run():
    """16 x 32 prioritized group: populate_memory (every slot fresh at the first update), min_max_buffer, two episodes of run_episodes
    with one evaluation sweep and beta annealed from 0.4 -- exactly 1.0 in the last episode; eval_scores; clone leaves the critic's
    bytes and the priorities."""
    torch, S, D, G = _mods()
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    L = 16
    tab = S.tables.synthetic_table("train")
    env = S.ShemsBatch(L * E, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    grp = G.PrioritizedLearnerGroup(L, E, seed=K.SEED, rng_seed=K.RNG_SEED, capacity=2400)
    assert grp.form == "throughput" and grp.tiled and (grp.alpha, grp.beta, grp.eps) == (0.6, 0.4, 1e-6)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    assert grp.fresh_range() == (0, 2400)
    etab = S.tables.synthetic_table("eval")
    env_eval = G.eval_batch([etab], [0] * L, L, test_runs=32, maxsteps=72)
    betas = []
    res = grp.run_episodes(env, env_eval, 2, test_every=100, test_runs=32, anneal_beta_from=0.4, on_eval=lambda l, i, tot, sc: betas.append(grp.beta))
    torch.cuda.synchronize()
    assert res.sweeps == 1 and grp.updates == 2 * 72 and grp.beta == 1.0 and betas[0] == 0.4 and grp._anneal is None
    assert grp.covered == grp.rings[0].pushed
    for k in DDPG_SIDE + ("per_prio", "per_pmax"):
        o, n = grp.layout[k]
        assert bool(torch.isfinite(grp.slab[:, o:o + n]).all()), k
    assert all(bool((grp.prio_of(l) > 0).all()) and grp.pmax_of(l).item() >= 1.0 for l in range(L))
    scores = grp.eval_scores(env_eval, test_runs=32)
    assert scores.shape == (L,) and np.isfinite(scores).all()
    demos = I.GroupDemos(L, 64)
    for l, dm in enumerate(demos.rings):
        d = K.learner_data(l)
        dm.s.copy_(torch.from_numpy(np.ascontiguousarray(d["s"][:64]))); dm.a.copy_(torch.from_numpy(np.ascontiguousarray(d["a"][:64])))
        dm.pushed = 64
    keep = ("critic", "critic_t", "m_critic", "v_critic", "per_prio", "per_pmax")
    before = _side(grp, keep + ("actor",))
    grp.clone(demos, tick=0)
    after = _side(grp, keep + ("actor",))
    for k in keep:
        assert torch.equal(before[k], after[k]), k
    assert not torch.equal(before["actor"], after["actor"]) and grp.clones == 1
    env.close()
    env_eval.close()


# ------------------------------------------------------------------------------------------------------------ 9. refusals --
def test_c_abi_refusals_launch_nothing():
    """Each refusal under a canary over the whole slab."""
    torch, S, D, G = _mods()
    torch, grp = _group(2, 17, hparams=[{"batch": 17}, {"batch": 17}])
    grp._use_tiled()
    torch.cuda.synchronize()
    snap = grp.slab.clone()
    ERR = S._capi.ERR_ARG
    a0 = grp.learners[0]
    ptr = lambda name: grp.slab.data_ptr() + 4 * grp.layout[name][0]

    def call(d=None, ring=None, g=None, w="tiled", hp="own", per=None, flags=0, bp=0.9, length=CAP, fresh=(0, 0)):
        d = a0._ddpg_args() if d is None else d
        ring = grp._ring0() if ring is None else ring
        g = grp.struct() if g is None else g
        w = C.byref(grp.w2t_struct()) if w == "tiled" else w
        hp = grp._hp_ptr() if hp == "own" else hp
        per = grp.per_struct() if per is None else per
        return grp.LP.shems_ddpg_group_update_per_tp(C.byref(d), C.byref(ring), C.byref(g), w, hp, C.byref(per), length, fresh[0], fresh[1],
                                                     K.RNG_SEED, 3, a0.eta_crit, bp, 0.999, a0.eta_act, 0.9, 0.999, flags, grp._stream())

    def per(**kw):
        p = grp.per_struct()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    err = lambda: grp.LP.shems_last_error()
    # what shems_ddpg_group_update_tp refuses
    d = a0._ddpg_args(); d.critic_t = None
    assert call(d) == ERR and b"NULL buffer" in err()
    assert call(g=G.Group(0, 0, grp.slab_floats * 4, E)) == ERR and call(g=G.Group(2, 0, grp.slab_floats * 4 + 4, E)) == ERR
    assert call(length=0) == ERR and call(length=CAP + 1) == ERR and call(bp=1.0) == ERR
    assert call(flags=4) == ERR and b"unknown flag" in err() and call(flags=8 | 1) == ERR
    d = a0._ddpg_args(); d.actor = d.actor + 4
    assert call(d) == ERR
    d = a0._ddpg_args(); d.batch = 129
    assert call(d, hp=None) == ERR and b"batch" in err()
    d = a0._ddpg_args(); d.grad_critic = None
    assert call(d, flags=1) == ERR
    assert call(hp=C.c_void_p(grp._hp_dev.data_ptr() + 4)) == ERR
    t = grp.w2t_struct(); t.critic = None
    assert call(w=C.byref(t)) == ERR
    # what check_per refuses
    for k in ("prio", "pmax", "ws"):
        assert call(per=per(**{k: None})) == ERR, k
    assert call(per=per(prio=ptr("per_prio") + 4)) == ERR and call(per=per(ws=ptr("per_ws") + 8)) == ERR and call(per=per(pmax=ptr("per_pmax") + 2)) == ERR
    assert call(per=per(ws=ptr("per_prio"))) == ERR and call(per=per(pmax=ptr("per_prio") + 64)) == ERR and call(per=per(pmax=ptr("per_ws") + 16)) == ERR
    for bad in (-0.1, float("nan"), float("inf")):
        for k in ("alpha", "beta", "eps_p"):
            assert call(per=per(**{k: bad})) == ERR, (k, bad)
    assert call(per=per(beta=1.5)) == ERR and b"beta" in err()
    assert call(fresh=(-1, 1)) == ERR and call(fresh=(CAP, 1)) == ERR and call(fresh=(0, -1)) == ERR
    assert call(length=600, fresh=(590, 20)) == ERR
    ring = grp._ring0(); ring.capacity = 262145
    assert call(ring=ring) == ERR and b"262144" in err()
    # a per block inside the learner's DDPG blocks, workspace, tiles or ring, or past the slab stride
    for k in ("ws", "critic", "m_actor", "ring_s", "ring_done", "w2t_critic", "losses", "grad_actor"):
        assert call(per=per(prio=ptr(k))) == ERR and b"overlap" in err(), k
    assert call(per=per(pmax=ptr("s_min") + 4)) == ERR and b"overlap" in err()
    assert call(per=per(ws=ptr("ws") + 16 * 1000)) == ERR and b"overlap" in err()
    far = grp.slab.data_ptr() + 4 * grp.slab_floats
    assert call(per=per(ws=far - 64)) == ERR and b"slab stride" in err()
    assert call(g=G.Group(2, 0, grp.slab_floats * 4 - 64, E)) == ERR and b"slab stride" in err()      # the last block ends beyond a shorter stride
    assert call(per=per(prio=grp.slab.data_ptr() - 4 * CAP - 64), g=G.Group(2, 0, grp.slab_floats * 4 - 64, E)) == ERR
    # the sampler alone
    sample = lambda p, g=None, cap=CAP, n=CAP, b=17, hp=None, fresh=(0, 0): grp.LP.shems_per_group_sample_dev(
        C.byref(p), C.byref(grp.struct() if g is None else g), hp, cap, n, fresh[0], fresh[1], 11, 0, b, grp._stream())
    assert sample(per(), b=0) == ERR and sample(per(), b=129) == ERR and sample(per(), cap=262145) == ERR and sample(per(prio=None)) == ERR
    assert sample(per(), n=CAP + 1) == ERR and sample(per(), g=G.Group(0, 0, 16, E)) == ERR and sample(per(), fresh=(CAP, 1)) == ERR
    # (the sampler alone is not told where the slab begins: it holds the three blocks to one stride of the lowest of them)
    assert sample(per(), g=G.Group(2, 0, 1024, E)) == ERR and b"slab stride" in err()
    assert sample(per(), hp=C.c_void_p(grp._hp_dev.data_ptr() + 4)) == ERR
    assert grp.LP.shems_ddpg_group_update_per_tp(None, None, None, None, None, None, CAP, 0, 0, 1, 1, 1e-3, 0.9, 0.999, 1e-3, 0.9, 0.999, 0, None) == ERR
    # SHEMS_ERR_STATE: a single learner on its own tiled working layout
    import test_ddpg_gpu as TD
    _, _, _, ag0, ring0, _ = TD._setup()
    ag0.use_tiled(True)
    ag0.replay(ring0, tick=0)
    d = ag0._ddpg_args(raw=True)
    assert call(d, ring=ring0.struct(), g=G.Group(1, 0, 0, E), w=None, hp=None, length=len(ring0), per=per()) == S._capi.ERR_STATE
    ag0.use_tiled(False)
    torch.cuda.synchronize()
    assert torch.equal(grp.slab.view(torch.int32), snap.view(torch.int32))          # the canary: nothing was launched
    assert call() == 0 and call(flags=S._capi.TP_PER_GIVEN | S._capi.TP_STORE_GRAD) == 0       # and the unmodified records run
    torch.cuda.synchronize()
    assert not torch.equal(grp.slab.view(torch.int32), snap.view(torch.int32))


def test_python_refusals_name_their_reason():
    torch, S, D, G = _mods()
    torch, grp = _group(2, 17)
    with pytest.raises(NotImplementedError, match="evaluate"):
        grp.evaluate()
    grp.learners[0].batch = 129
    with pytest.raises(NotImplementedError, match="batch 129"):
        grp.replay()
    grp.learners[0].batch = 17
    ones = torch.ones((2, 128), dtype=torch.float32, device=grp.device)
    with pytest.raises(ValueError, match="replay_given"):
        grp.replay_given(torch.zeros((2, 120), dtype=torch.int32, device=grp.device), ones)
    with pytest.raises(ValueError, match="replay_given"):
        grp.replay_given(torch.zeros((2, 128), dtype=torch.int64, device=grp.device), ones)
    with pytest.raises(ValueError, match="anneal_beta"):
        grp.run_episodes(None, None, 2, anneal_beta_from=1.5)
    # warm_start_group needs evaluate(): refused before its DAgger stage trains anything
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    torch.cuda.synchronize()
    snap = grp.slab.clone()
    with pytest.raises(NotImplementedError, match="evaluate"):
        I.warm_start_group(grp, None, None, None, None, 2, 5, 5)
    assert torch.equal(grp.slab.view(torch.int32), snap.view(torch.int32)) and grp.clones == 0 and grp.updates == 0 and grp._anneal is None
    # a plain group keeps the parent's layout; the prioritized group's DDPG offsets are its own
    ref = G.LearnerGroup(2, E, seed=K.SEED, capacity=128, form="throughput", tiled=True)
    assert ref.slab_floats == 4243932 and list(ref.layout)[-1] == "ring_done"
    assert all(grp.layout[k][0] == G.slab_layout(D.N_ACTOR, D.N_CRITIC, 1902568, CAP, True)[0][k][0] for k in ref.layout)

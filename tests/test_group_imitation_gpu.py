"""Grouped imitation on the GPU: LearnerGroup.clone / evaluate (shems_ddpg_group_clone_update_tp / _critic_update_tp, csrc/shems_gupd.hip)
and the host layer on top (imitation.GroupDemos / GroupRings / dagger_group / warm_start_group).

The supervised update is held to the float64 evaluation of its definition (tests/imitation_ref.py: clone_grad), block by block, with
the bounds the grouped update is held to (tests/test_group_gpu.py); the critic-only update runs the update's own kernels on the
update's own inputs and is held to replay()'s BITS.  Shapes: 32 envs per learner, rings of 128 slots of synthetic data (a different
seed per learner, tests/warmstart_ref.py: critic_data, whose heads are lifted so that every gradient path carries signal), 2 learners
for the narrow launch shapes and 48 for the wide ones."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ddpg_oracle as DO
import imitation_ref as IR
import util as U
import warmstart_ref as WR

pytestmark = pytest.mark.gpu

E, CAP = 32, IR.CLONE_CAP
BLOCK_TOL = 2e-6                      # tests/test_ddpg_gpu.py:57-62, the bound of every gradient block in this suite
ACTOR_SIDE = ("actor", "actor_t", "m_actor", "v_actor", "grad_actor")
CRITIC_SIDE = ("critic", "critic_t", "m_critic", "v_critic", "grad_critic")
TICKS = (3, 4)
# csrc/shems_gupd.hip's workspace carve: two [12][128] input blocks, then r [128], done [128], the sampled slots [128] int32
TP_R, TP_DONE, TP_IDX = 2 * 12 * 128, 2 * 12 * 128 + 128, 2 * 12 * 128 + 256


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    return torch, S, mod("ddpg"), mod("group"), mod("imitation")


def _data(l):
    return WR.critic_data(100 + l, CAP)


def _group(L, length, batch=120, form="throughput", tiled=None, hparams=None, own_targets=False):
    """An L-learner group on learner-specific synthetic data: networks with lifted heads, the group's own rings holding full
    transitions (mixed done), and a GroupDemos whose r / s2 / done hold NaN / 0xFF (the supervised update must never read them)."""
    torch, S, D, G, I = _mods()
    grp = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=CAP, form=form, tiled=tiled, hparams=hparams)
    grp.store_grad = True
    demos = I.GroupDemos(L, CAP)
    data = []
    up = lambda t, v: t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    for l, ag in enumerate(grp.learners):
        d = _data(l)
        ag.set_params(actor=d["pa"], critic=d["pc"])
        if own_targets:                        # targets that differ from the live networks (Flux-order view is current after set_params)
            up(ag.actor_t, d["pa_t"]); up(ag.critic_t, d["pc_t"])
        ag.set_norm(d["s_min"], d["s_max"])
        if hparams is None:
            ag.batch = batch
        ring, dm = grp.rings[l], demos.rings[l]
        for k in ("s", "a", "r", "s2", "done"):
            up(getattr(ring, k), d[k])
        up(dm.s, d["s"]); up(dm.a, d["a"])
        dm.r.fill_(float("nan")); dm.s2.fill_(float("nan")); dm.done.fill_(0xFF)
        ring.pushed = dm.pushed = length
        data.append(d)
    if grp.tiled:
        grp.flux_changed()
    return torch, grp, demos, data


def _bits(grp, name):
    o, n = grp.layout[name]
    return grp.slab[:, o:o + n].contiguous().view(grp.torch.int32).clone()


def _side(grp, names):
    grp.flux_()
    return {k: _bits(grp, k) for k in names}


def _losses(grp):
    o = grp.layout["losses"][0]
    return grp.slab[:, o:o + 2].cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. clone against float64 --
# (learners, batch, ring length, tau) -> the comparisons that needed a tied relu decided the other way: [(learner, tick)]
CLONE_CASES = [(2, 1, 1, 1.0), (2, 1, 90, 1.0), (2, 17, 1, 1.0), (2, 17, 90, 0.001), (2, 128, 1, 0.001), (2, 128, 90, 1.0), (48, 120, CAP, 1.0)]
EXPECTED_TIES = {c: [] for c in CLONE_CASES}


def _clone_vs_float64(grp, demos, data, length, tau, batches, etas, check=None):
    """Two grp.clone steps; learner l (those in `check`) is held to IR.clone_grad in float64 on ITS minibatch of batches[l] draws,
    and ADAM / the soft update / the moments to DO.Adam(etas[l]) from the kernel's own gradient.  Returns the ties set aside."""
    import test_imitation_gpu as TI
    torch = grp.torch
    check = range(grp.count) if check is None else check
    host = {l: dict(pa=data[l]["pa"].copy(), pat=data[l]["pa"].copy(), opt=DO.Adam(len(data[l]["pa"]), etas[l])) for l in check}
    ties = []
    for step, tick in enumerate(TICKS):
        grp.clone(demos, tick=tick, tau=tau)
        grp.flux_()
        torch.cuda.synchronize()
        losses = _losses(grp)
        for l in check:
            ag, d, h, B = grp.learners[l], data[l], host[l], batches[l]
            idx = DO.sample_indices(grp.rng_seed + l, tick, B, length)
            s, a = d["s"][idx], d["a"][idx]
            g64, l64 = IR.clone_grad(h["pa"], s, a, d["s_min"], d["s_max"], np.float64)
            g = ag.grad_actor.cpu().numpy()
            ev = lambda p: IR.clone_grad(p, s, a, d["s_min"], d["s_max"], np.float64)[0]
            what = f"clone gradient of learner {l}, tick {tick}, B={B} len={length}"
            errs, tie = TI._assert_blocks_or_the_other_relu_decision(g, h["pa"], ev, DO.normalize(s, d["s_min"], d["s_max"]), what)
            if tie:
                ties.append((l, tick))
            loss = float(losses[l, 1])
            print(f"{what}: block errors {errs}, tie {tie}; loss {loss!r} vs float64 {l64!r}")
            assert np.isfinite(g).all() and abs(loss - l64) < 1e-4 * max(1.0, abs(l64)), what
            # the minibatch the launches saw
            got = ag.ws[TP_IDX:TP_IDX + 128].view(torch.int32).cpu().numpy()
            assert (got[:B] == idx).all() and (got[B:] == -1).all()
            # ADAM (the second step on the advanced beta powers), soft update and moments from the kernel's own gradient
            pa1 = h["opt"].step(h["pa"], g)
            act, act_t = ag.actor.cpu().numpy(), ag.actor_t.cpu().numpy()
            np.testing.assert_allclose(act, pa1, rtol=0, atol=1e-7)
            np.testing.assert_allclose(act_t, DO.soft_update(h["pat"], act, np.float32(tau)), rtol=0, atol=1e-7)
            np.testing.assert_allclose(ag.m_actor.cpu().numpy(), h["opt"].m, rtol=1e-6, atol=1e-12)
            np.testing.assert_allclose(ag.v_actor.cpu().numpy(), h["opt"].v, rtol=1e-6, atol=1e-15)
            if tau == 1.0:
                assert torch.equal(ag.actor_t, ag.actor), what                   # 1 p + 0 t
            else:
                assert not torch.equal(ag.actor_t, ag.actor), what
            h["pa"], h["pat"] = act, act_t                                       # the next step starts from the device's bytes
            h["opt"].m, h["opt"].v = ag.m_actor.cpu().numpy().astype(h["opt"].m.dtype), ag.v_actor.cpu().numpy().astype(h["opt"].v.dtype)
    assert grp.clones == 2 and grp.updates == 0 and grp.evaluations == 0
    for ag in grp.learners:
        assert ag.clones == 2 and ag.updates == 0 and ag.bp_critic == [0.9, 0.999]
        assert abs(ag.bp_actor[0] - 0.9 ** 3) < 1e-15 and abs(ag.bp_actor[1] - 0.999 ** 3) < 1e-15
    return ties


@pytest.mark.parametrize("L,batch,length,tau", CLONE_CASES)
def test_group_clone_matches_float64_per_block(L, batch, length, tau):
    torch, grp, demos, data = _group(L, length, batch)
    assert grp.tiled and grp.form == "throughput"
    ties = _clone_vs_float64(grp, demos, data, length, tau, [batch] * L, [DO.ETA_ACT] * L)
    assert ties == EXPECTED_TIES[(L, batch, length, tau)], ties
    end = grp.layout["grad_critic"][0]
    assert bool(torch.isfinite(grp.slab[:, :end]).all())


# ------------------------------------------------------------------------------------------ 2. what clone leaves alone --
def test_group_clone_leaves_the_critic_side_alone():
    torch, grp, demos, data = _group(2, 90, 17, own_targets=True)
    for ag in grp.learners:                    # not live in a clone step: made visible
        ag.m_critic.fill_(0.25); ag.v_critic.fill_(0.5); ag.grad_critic.fill_(-3.0)
        ag.losses[0] = 42.0
    grp.flux_changed()
    grp._use_tiled()                           # the critic's tiles as training would hold them
    before = _side(grp, CRITIC_SIDE)
    tiles0 = _bits(grp, "w2t_critic")
    for tick in TICKS:
        grp.clone(demos, tick=tick)
    torch.cuda.synchronize()
    after = _side(grp, CRITIC_SIDE)
    for k in CRITIC_SIDE:
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(tiles0, _bits(grp, "w2t_critic"))
    assert (_losses(grp)[:, 0] == 42.0).all()
    # r, s2 and done of the demonstration rings hold NaN / 0xFF: had they been read, something here would not be finite
    for k in ACTOR_SIDE:
        o, n = grp.layout[k]
        assert bool(torch.isfinite(grp.slab[:, o:o + n]).all()), k
    assert np.isfinite(_losses(grp)[:, 1]).all()
    for dm in demos.rings:
        assert bool(torch.isnan(dm.r).all()) and bool(torch.isnan(dm.s2).all()) and bool((dm.done == 0xFF).all())


# ------------------------------------------------------------------------------------------------ 3. layouts and records --
def _two_clone_steps(tau=0.5, **kw):
    torch, grp, demos, data = _group(2, 90, 17, **kw)
    for tick in TICKS:
        grp.clone(demos, tick=tick, tau=tau)
    torch.cuda.synchronize()
    return grp, dict(_side(grp, ACTOR_SIDE), losses=_bits(grp, "losses")[:, 1:])


def test_group_clone_tiled_and_flux_order_leave_the_same_bits():
    gt, tiled = _two_clone_steps(tiled=True)
    gf, flux = _two_clone_steps(tiled=False)
    assert gt.tiled and not gf.tiled
    for k in tiled:
        assert gt.torch.equal(tiled[k], flux[k]), k
    assert not gt.torch.equal(tiled["actor"], tiled["actor_t"])            # tau = 0.5: the target moved on its own


@pytest.mark.parametrize("tiled", [True, False])
def test_group_clone_uniform_records_leave_the_bits_of_the_shared_entry_point(tiled):
    gs, shared = _two_clone_steps(tiled=tiled)
    gr, rec = _two_clone_steps(tiled=tiled, hparams=[{"batch": 17}, {"batch": 17}])
    assert gs._hp_dev is None and gr._hp_dev is not None and len(gr._hp_variants) == 1
    for k in shared:
        assert gs.torch.equal(shared[k], rec[k]), k


def test_group_clone_per_learner_batch_and_eta_meet_their_own_float64():
    recs = [{"batch": 17, "eta_act": 3e-4}, {"batch": 120, "eta_act": 5e-5}]
    torch, grp, demos, data = _group(2, 90, hparams=recs)
    etas = [float(np.float32(r["eta_act"])) for r in recs]
    ties = _clone_vs_float64(grp, demos, data, 90, 1.0, [r["batch"] for r in recs], etas)
    assert ties == [], ties


# ------------------------------------------------------------------ 4. critic-only == the critic half of replay() --
@pytest.mark.parametrize("L,tiled", [(2, True), (2, False), (48, True), (48, False)])
def test_group_evaluate_leaves_the_bits_of_the_critic_half_of_replay(L, tiled):
    torch, ga, _, data = _group(L, 90, 120, tiled=tiled, own_targets=True)
    _, gb, _, _ = _group(L, 90, 120, tiled=tiled, own_targets=True)
    assert {0, 1} <= set(np.concatenate([d["done"][:90] for d in data]).tolist())          # mixed done
    both = ACTOR_SIDE + CRITIC_SIDE + ("losses",)
    sa, sb = _side(ga, both), _side(gb, both)
    for k in both:
        assert torch.equal(sa[k], sb[k]), k                                            # identical starts
    for step, tick in enumerate(TICKS):
        actor0 = dict(_side(ga, ACTOR_SIDE), loss1=_bits(ga, "losses")[:, 1:])
        ga.evaluate(tick=tick)
        gb.replay(tick=tick)
        torch.cuda.synchronize()
        sa, sb = _side(ga, both), _side(gb, both)
        for k in CRITIC_SIDE:
            assert torch.equal(sa[k], sb[k]), (k, tick)
        assert torch.equal(sa["losses"][:, :1], sb["losses"][:, :1]), tick
        for k in ACTOR_SIDE:                                                           # nothing of the actor side was written
            assert torch.equal(sa[k], actor0[k]), (k, tick)
        assert torch.equal(sa["losses"][:, 1:], actor0["loss1"])
        assert not torch.equal(sa["critic"], sa["critic_t"]) and not torch.equal(sb["actor"], actor0["actor"])
        # both start the next step alike: replay()'s actor side into the other group
        for k in ACTOR_SIDE + ("losses",):
            o, n = ga.layout[k]
            ga.slab[:, o:o + n].copy_(gb.slab[:, o:o + n])
        ga.flux_changed()
    assert ga.evaluations == 2 and ga.updates == 0 and gb.updates == 2
    for x, y in zip(ga.learners, gb.learners):
        assert x.bp_critic == y.bp_critic and x.bp_actor == [0.9, 0.999] and x.evaluations == 2


# ------------------------------------------------------------------------------------------- 5. a ring outside the slab --
def test_group_evaluate_on_an_mc_ring_outside_the_slabs():
    """Returns of magnitude 400 with done = 1 in a GroupRings.  The throughput form publishes the sampled r and done rows (not y): the
    head forms y = r + gamma (1 - done) q', which with done = 1 is the stored float32 return itself -- the rows must hold the stored
    bits and ones -- and the critic gradient meets the float64 evaluation with y = G."""
    import test_warmstart_gpu as TW
    torch, grp, _, data = _group(3, 90, 120, own_targets=True)
    _, S, D, G, I = _mods()
    rings = I.GroupRings(3, CAP)
    assert rings.stride_bytes != grp.slab_floats * 4
    up = lambda t, v: t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    for l, ring in enumerate(rings.rings):
        d = data[l]
        up(ring.s, d["s"]); up(ring.a, d["a"]); up(ring.r, d["G"]); up(ring.s2, d["s2"])
        ring.done.fill_(1)
        ring.pushed = 90
    own = [tuple(t.clone() for t in (r.s, r.a, r.r, r.s2, r.done)) for r in grp.rings]
    tick = TICKS[0]
    grp.evaluate(rings, tick=tick)
    grp.flux_()
    torch.cuda.synchronize()
    for l in (0, 2):
        ag, d = grp.learners[l], data[l]
        idx = DO.sample_indices(grp.rng_seed + l, tick, 120, 90)
        ws = ag.ws.cpu().numpy()
        assert (U.bits32(ws[TP_R:TP_R + 120]) == U.bits32(d["G"][idx])).all() and np.abs(d["G"][idx]).max() > 100
        assert (ws[TP_DONE:TP_DONE + 120] == 1.0).all() and not ws[TP_R + 120:TP_R + 128].any()
        Lr = WR.learner(d)
        y = Lr.targets(d["G"][idx], d["s2"][idx], np.ones(120, bool))
        assert (U.bits32(y) == U.bits32(d["G"][idx])).all()
        x = np.concatenate([DO.normalize(d["s"][idx], d["s_min"], d["s_max"]), d["a"][idx]], 1)

        def ev(p):
            Lq = WR.learner(d)
            Lq.critic = np.asarray(p)
            return Lq.critic_grad(d["s"][idx], d["a"][idx], y, dtype=np.float64)[0]
        g = ag.grad_critic.cpu().numpy()
        errs, tie = TW._assert_blocks_or_the_other_relu_decision(g, d["pc"], ev, x, f"critic gradient on returns, learner {l}")
        print(f"MC ring outside the slab, learner {l}: block errors {errs}, tie {tie}")
    for ring, keep in zip(grp.rings, own):                                             # the group's own rings were not involved
        assert all(torch.equal(a, b) for a, b in zip((ring.s, ring.a, ring.r, ring.s2, ring.done), keep))


# ------------------------------------------------------------------------------------------------------ 6. latency form --
def test_latency_form_leaves_the_bits_of_the_single_learner_calls():
    torch, grp, demos, data = _group(3, 90, 17, form="latency", own_targets=True)
    _, S, D, G, I = _mods()
    assert grp.form == "latency" and not grp.tiled
    grp.clone(demos, tick=3, tau=0.5)
    grp.evaluate(tick=4)
    grp.evaluate(tick=5, tau=0.25)
    torch.cuda.synchronize()
    assert grp.clones == 1 and grp.evaluations == 2 and grp.updates == 0
    up = lambda t, v: t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    for l, lg in enumerate(grp.learners):
        d = data[l]
        ag = D.Agent(seed=1, rng_seed=grp.rng_seed + l)
        ag.set_params(actor=d["pa"], critic=d["pc"])
        up(ag.actor_t, d["pa_t"]); up(ag.critic_t, d["pc_t"])
        ag.set_norm(d["s_min"], d["s_max"])
        ag.batch = 17
        dm, ring = I.Demos(CAP), D.ReplayRing(CAP)
        up(dm.s, d["s"]); up(dm.a, d["a"])
        for k in ("s", "a", "r", "s2", "done"):
            up(getattr(ring, k), d[k])
        dm.pushed = ring.pushed = 90
        ag.clone(dm, tick=3, tau=0.5)
        ag.evaluate(ring, tick=4)
        ag.evaluate(ring, tick=5, tau=0.25)
        torch.cuda.synchronize()
        for k in ag._LEARNER_TENSORS:
            assert torch.equal(getattr(ag, k).view(torch.int32), getattr(lg, k).view(torch.int32)), (l, k)
        assert ag.bp_actor == lg.bp_actor and ag.bp_critic == lg.bp_critic and lg.clones == 1 and lg.evaluations == 2


# ---------------------------------------------------------------------------------------------------------- 7. refusals --
def test_what_the_grouped_updates_refuse():
    torch, grp, demos, data = _group(2, 90, 17)
    _, S, D, G, I = _mods()
    grp._use_tiled()
    torch.cuda.synchronize()
    snap = grp.slab.clone()
    wide = G.LearnerGroup(2, E, capacity=CAP, form="wide")
    with pytest.raises(NotImplementedError, match="wide"):
        wide.clone(demos)
    with pytest.raises(NotImplementedError, match="wide"):
        wide.evaluate()
    demos.rings[1].pushed = 50
    with pytest.raises(ValueError, match="unequal lengths"):
        grp.clone(demos)
    demos.rings[1].pushed = 90
    good = demos.stride_bytes
    for bad in (good + 2, -good, 0):
        demos.stride_bytes = bad
        with pytest.raises(S._capi.ShemsError, match="ring stride"):
            grp.clone(demos)
        with pytest.raises(S._capi.ShemsError, match="ring stride"):
            grp.evaluate(demos)
    demos.stride_bytes = good

    def call(name, d=None, ring=None):
        a0 = grp.learners[0]
        d = a0._ddpg_args() if d is None else d
        r0 = demos.struct0() if ring is None else ring
        g, t = grp.struct(), grp.w2t_struct()
        return getattr(grp.L, name)(C.byref(d), C.byref(r0), good, C.byref(g), C.byref(t), None, 90, 7, 0, a0.eta_act, 0.9, 0.999, 1, grp._stream())

    ERR = S._capi.ERR_ARG
    r = demos.struct0(); r.a = None
    assert call("shems_ddpg_group_clone_update_tp", ring=r) == ERR and b"s and a" in grp.L.shems_last_error()
    r = demos.struct0(); r.done = None
    assert call("shems_ddpg_group_critic_update_tp", ring=r) == ERR and b"s, a, r, s2 and done" in grp.L.shems_last_error()
    r = demos.struct0(); r.r = r.s2 = r.done = None          # what the supervised update never reads may be absent
    d = grp.learners[0]._ddpg_args(); d.m_actor = None
    assert call("shems_ddpg_group_clone_update_tp", d=d, ring=r) == ERR and b"NULL buffer" in grp.L.shems_last_error()
    d = grp.learners[0]._ddpg_args(); d.critic_t = None
    assert call("shems_ddpg_group_critic_update_tp", d=d) == ERR and b"NULL buffer" in grp.L.shems_last_error()
    d = grp.learners[0]._ddpg_args(); d.batch = 129
    assert call("shems_ddpg_group_clone_update_tp", d=d) == ERR
    torch.cuda.synchronize()
    assert torch.equal(grp.slab.view(torch.int32), snap.view(torch.int32))
    assert grp.clones == 0 and grp.evaluations == 0 and all(ag.bp_actor == [0.9, 0.999] for ag in grp.learners)


# ---------------------------------------------------------------------- 8. dagger_group / warm_start_group, S1-sized --
GRID = dict(nb=9, ne=5, nab=5, nae=3)          # tests/foresight_twin.py: S1
T1 = 30


def _s1_group(S, G, F, H):
    """4 learners on two configs of the Charger98 eval table (env l on config l % 2), 30 hours from row 1."""
    tab = U.tables_mod().profile_table(98, "eval")
    cfgs = [S.make_config(98, 0, tab.shape[0]), S.make_config(98, 0, tab.shape[0], disc_weight=0.1, disc_pot=1.0)]
    co = np.array([0, 1, 0, 1], np.uint16)
    env = S.ShemsBatch(4, T1, [tab], cfgs, co).use_torch_stream()
    val = H.foresight_values(env, F.Grid(GRID["nb"], GRID["ne"], GRID["nab"], GRID["nae"]))
    assert val.n_problems == 2
    grp = G.LearnerGroup(4, E, seed=5, capacity=64, form="throughput")
    for ag in grp.learners:
        ag.batch = 30
    return tab, cfgs, env, val, grp


def test_dagger_group_and_warm_start_group_on_s1_sized_data():
    torch, S, D, G, I = _mods()
    F, H = importlib.import_module(U.PKG_NAME + ".foresight"), importlib.import_module(U.PKG_NAME + ".harness")
    STEPS = 100
    # group A stops after round 0: its actors are the ones group B's round 1 starts with (same seeds, same launches)
    tab, cfgs, env, val, ga = _s1_group(S, G, F, H)
    da = I.GroupDemos(4, 128)
    out_a = I.dagger_group(ga, env, val, da, 1, STEPS)
    _, _, _, _, gb = _s1_group(S, G, F, H)
    db, ring = I.GroupDemos(4, 128), I.GroupRings(4, 64)
    with pytest.raises(ValueError, match="training ring"):
        I.warm_start_group(gb, env, val, db, gb, 2, STEPS, 50, mode="mc")
    *rounds, critic = I.warm_start_group(gb, env, val, db, ring, 2, STEPS, 50, mode="mc")
    torch.cuda.synchronize()
    # every round appends one pass per learner; the figures are finite [count] arrays
    assert [r["demos"] for r in rounds] == [T1, 2 * T1] and all(len(r) == 2 * T1 for r in db.rings) and all(len(r) == T1 for r in da.rings)
    assert gb.clones == 2 * STEPS and gb.evaluations == 50 and gb.updates == 0
    for r in rounds + out_a:
        for k in ("return", "loss", "loss_first"):
            assert r[k].shape == (4,) and np.isfinite(r[k]).all(), k
        assert r["host_s"] > 0
    print("dagger_group: round 0 clone loss first", rounds[0]["loss_first"], "last", rounds[0]["loss"], "returns", [r["return"] for r in rounds])
    assert (rounds[0]["loss"] < rounds[0]["loss_first"]).all()                       # the clone loss of round 0 falls over its steps
    assert (rounds[0]["return"] == out_a[0]["return"]).all() and (rounds[0]["loss"] == out_a[0]["loss"]).all()
    assert rounds[0]["return"][0] == rounds[0]["return"][2] and rounds[0]["return"][1] == rounds[0]["return"][3]      # env l on config l % 2
    want = T1 - I.default_tail("mc", gb.learners[0].gamma, T1)
    assert critic["transitions"] == want and all(len(r) == want and bool(r.done[:want].all()) for r in ring.rings)
    print("warm_start_group mc: critic loss first", critic["critic_loss_first"], "last", critic["critic_loss_last"])
    assert critic["critic_loss_first"].shape == (4,) and np.isfinite(critic["critic_loss_first"]).all()
    assert (critic["critic_loss_last"] < critic["critic_loss_first"]).all()
    # learner l's ring against the single-agent functions on the same passes, bit for bit
    ga.flux_()
    for l in (1, 2):
        env1 = S.ShemsBatch(1, T1, [tab], [cfgs[l % 2]]).use_torch_stream()
        val1 = H.foresight_values(env1, F.Grid(GRID["nb"], GRID["ne"], GRID["nab"], GRID["nae"]))
        one = I.Demos(128)
        env1.reset_(-1)
        I.from_foresight(env1, val1, one)
        ag = D.Agent(seed=1)
        ag.set_params(actor=ga.learners[l].actor.cpu().numpy())
        ag.set_norm(ga.learners[l].s_min.cpu().numpy(), ga.learners[l].s_max.cpu().numpy())
        _, res = H.inference(env1, ag, track=1, num_steps=T1)
        I.from_pass(val1, res, one)
        env1.close()
        assert len(one) == 2 * T1
        for k in ("s", "a"):
            assert torch.equal(getattr(one, k)[:2 * T1].view(torch.int32), getattr(db.rings[l], k)[:2 * T1].view(torch.int32)), (l, k)
        assert torch.equal(getattr(one, "s")[:T1], da.rings[l].s[:T1])
        # the normalisation is the single learner's min_max_buffer on the foresight pass
        ref = D.Agent(seed=1, rng_seed=ga.learners[l].rng_seed)
        first = I.Demos(128)
        first.s[:T1].copy_(da.rings[l].s[:T1]); first.pushed = T1
        ref.min_max_buffer(first)
        assert torch.equal(ref.s_min, ga.learners[l].s_min) and torch.equal(ref.s_max, ga.learners[l].s_max)
    env.close()

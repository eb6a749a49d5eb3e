"""The layer-by-layer path (csrc/shems_wide.hip, wgemm*_body.h, k_track<true>) at the edges of the sizes, batches and rows its API takes,
each held to the float64 oracle at that size: act() at row counts on both sides of the small-M / tile boundaries, replay() at batches 1,
33 and 128, the fused step, the tracking pass, three wide learner groups (pass widths 160 and 256, 4096-wide networks) and the
sub-batches of a single Agent (uneven splits, three and eight parts).  Every network has non-zero biases in both hidden layers: with
b2 = 0 a padded column of the folded head adds relu(0) * W3 = 0 whether or not its guards work.

Bounds: the existing ones (act 1e-5, gradient blocks 2e-6 of the block's max-abs, ADAM / soft update 1e-7 element-wise, whole learner
3e-6) were set at (300, 600), where a pass chains one sum over each hidden layer, 900 terms in all.  A chained sum's rounding error
grows like the square root of its length, so each of them is multiplied by sqrt((l1 + l2) / 900) when that is above 1 (_scale); the
element-wise ADAM bound works on the kernel's own gradient and does not scale.  The whole-learner comparison leaves out the gradient
elements at ADAM's noise floor (_noisy) and holds them to ADAM's largest step instead.  Every test prints the largest error it saw next
to its bound."""
import ctypes as C
import importlib

import numpy as np
import pytest

import util as U
from util import oracle_c
import ddpg_oracle as DO
import test_group_wide_gpu as TG
import test_wide_gpu as TW

pytestmark = pytest.mark.gpu
f32 = np.float32

# hidden (l1, l2) -> the edge it exists for
SIZES = {
    (1, 1): "every product a partial tile; K = 1 in layers 2 and 3",
    (3, 5): "K = 3 and 5 in layers 2 and 3, below the input layer's 9 / 11; not V4",
    (16, 64): "exactly one K stage; l2 fills one head half, the other half's partial must be exact zero; V4",
    (17, 65): "one past each of those; not V4",
    (128, 128): "the exact 128 tile; V4",
    (129, 257): "one past the 128 tile in both; not V4",
    (260, 101): "l1 % 4 == 0, l2 % 4 != 0: only the l2 half of the V4 predicate keeps it off V4; l2 ends inside the second head half",
    (4096, 8): "lopsided: the shared launch's early return, workspace buffers of very different sizes",
    (8, 4096): "lopsided the other way: 64 head partials over an 8-deep layer 2",
    (4096, 4096): "64 head partials, 64 K stages of 64 in layer 2 (one tick, sampled rows)",
}
BIG = (4096, 4096)
DEPTH0 = 300 + 600                                # the chained summation depth the existing bounds were set at
EPS = 1e-8                                        # ADAM's epsilon (DO.Adam)
ACT_ROWS = (1, 33, 512, 513, 2085)                # k_wgemm_sk / k_wgemm at 512 / 513; 2085 % 128 = 37: a partial row tile


def _scale(hid):
    """sqrt(depth / 900), at least 1: a pass chains one sum over each hidden layer, l1 + l2 terms in all; the bounds were set at
    (300, 600), where that chain is 900 long (batches stay <= 256, shallower than either layer there)."""
    return max(1.0, float(np.sqrt((hid[0] + hid[1]) / DEPTH0)))


def _at(monkeypatch, hid):
    monkeypatch.setattr(DO, "L1", hid[0])
    monkeypatch.setattr(DO, "L2", hid[1])


def _lift_b2(pa, pc, hid, rng):
    """Both hidden layers' biases of both networks (in the flat Flux layout at `hid`) to positive values -- b1 0.05..0.3, b2 0.02..0.1 --
    so a network of one or a few units is not dead (the range checks also ask for a spread over the rows), and a padded column that
    took b2[0] and W3[0] instead of zeros would add relu(b2[0]) * W3[0] != 0."""
    h1, h2 = hid
    for p, i in ((pa, 9), (pc, 11)):
        o = i * h1
        p[o:o + h1] = rng.uniform(0.05, 0.3, h1)
        if h1 == 1:                               # one unit in layer 1: negative weights into or out of it would kill the network
            p[:o] = np.abs(p[:o])
            p[o + h1:o + h1 + h2] = np.abs(p[o + h1:o + h1 + h2])
        o += h1 + h1 * h2
        p[o:o + h2] = rng.uniform(0.02, 0.1, h2)
    pa[-2:] = [0.6, -0.5]                         # the actor's b3 (0.3, -0.2 from _boosted): |a| > 0.3 somewhere whatever the hidden layers add
    return pa, pc


def _nets(D, seed, hid):
    pa, pc = TW._boosted(D, seed, hid)
    return _lift_b2(pa, pc, hid, np.random.default_rng(seed + 1000))


def _rows(m, hid):
    """The rows held to float64: all of them, or at (4096, 4096) at most 512 around every tile boundary."""
    if hid != BIG:
        return np.arange(m)
    r = set(range(min(m, 40)))
    for b in (64, 128, 256, 384, 512, 640, 1024, 2048, m):
        r.update(range(max(0, b - 3), min(m, b + 3)))
    return np.array(sorted(r))


def _noisy(g64, in_dim, out_dim, eta, bound):
    """The gradient elements at ADAM's noise floor.  A first step moves a parameter by eta * g / (|g| + 1e-8), whose slope in g is
    eta * 1e-8 / (|g| + 1e-8)^2: for |g| near 1e-8 the fp32 rounding of g -- up to 2 x BLOCK_TOL x the block's max-abs between the
    kernel and the fp32 oracle, each within BLOCK_TOL of float64 -- moves the step by up to 2 * eta.  An element is at the floor when
    that rounding can move its step by more than a tenth of the learner bound."""
    out = np.zeros(len(g64), bool)
    for _, lo, hi in DO.blocks(in_dim, out_dim):
        g = np.abs(g64[lo:hi])
        out[lo:hi] = eta * EPS * 2 * TW.BLOCK_TOL * g.max() / (g + EPS) ** 2 > 0.1 * bound
    return out


def _learner_matches(ag, whole, noisy, grads, bound, ticks, what):
    """The whole learner against the fp32 oracle's learner: `bound` off the noisy elements (union over the ticks so far); on them,
    what two ADAM steps in opposite directions can differ by (a step is at most about eta: 2.5 * eta per tick).  Prints the worst element overall, with the kernel's and the float64 gradient there.
    Returns the worst error off the floor."""
    worst = 0.0
    for name, net, eta in (("critic", "critic", DO.ETA_CRIT), ("critic_t", "critic", DO.ETA_CRIT), ("actor", "actor", DO.ETA_ACT),
                           ("actor_t", "actor", DO.ETA_ACT)):
        d = np.abs(getattr(ag, name).cpu().numpy() - getattr(whole, name))
        m = noisy[net]
        err = float(d[~m].max()) if (~m).any() else 0.0
        assert err < bound, (what, name, err, bound)
        assert float(d.max()) < 2.5 * float(eta) * ticks, (what, name, float(d.max()))
        worst = max(worst, err)
        if name in ("critic", "actor"):
            j = int(d.argmax())
            g, g64 = grads[net]
            print(f"{what}: {name} worst element [{j}] off by {d[j]:.3g}, gradient {g[j]:.3g} (kernel) / {g64[j]:.3g} (float64), "
                  f"{'at the noise floor' if m[j] else 'held'}; {int(m.sum())} of {m.size} elements at the floor")
    return worst


def _host(ag):
    return {k: getattr(ag, k).cpu().numpy() for k in ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic")}


# ---- single wide Agents ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hid", list(SIZES), ids=lambda h: f"{h[0]}x{h[1]}")
def test_act_matches_float64_at_every_size_and_row_count(monkeypatch, hid):
    torch, S, D = TW._mods()
    _at(monkeypatch, hid)
    pa, _ = _nets(D, 101, hid)
    ag = D.Agent(seed=101, hidden=hid, wide=True)
    ag.set_params(actor=pa)
    assert (ag.export_actor() == pa).all()
    obs_all = TW._rand_obs(np.random.default_rng(7), max(ACT_ROWS))
    s_min, s_max = obs_all.min(0) - 0.01, obs_all.max(0) + 0.5
    ag.set_norm(s_min, s_max)
    bound, worst, top, spread = TW.ATOL * _scale(hid), 0.0, 0.0, 0.0
    for m in ACT_ROWS:
        obs = obs_all[:m]
        got = ag.act(torch.from_numpy(obs).cuda(), train=False).cpu().numpy()
        rows = _rows(m, hid)
        want = DO.act(pa, obs[rows], s_min.astype(f32), s_max.astype(f32), False, dtype=np.float64)
        err = float(np.abs(got[rows] - want).max())
        assert got.shape == (m, 2) and np.isfinite(got).all() and err < bound, (hid, m, err, bound)
        worst, top = max(worst, err), max(top, float(np.abs(want).max()))
        spread = max(spread, float(np.ptp(want, 0).min()) if len(rows) > 1 else 0.0)
    assert top > 0.3 and spread > 1e-3, (hid, top, spread)
    print(f"act {hid}: max |err| {worst:.3g} (bound {bound:.3g}), max |a| {top:.3f}, spread {spread:.3f}")


# (hidden, batch): every batch at >= 2 sizes, every size at >= 1 batch
REPLAY_CASES = [((1, 1), 1), ((1, 1), 33), ((3, 5), 128), ((16, 64), 33), ((17, 65), 1), ((17, 65), 128), ((128, 128), 128),
                ((129, 257), 33), ((260, 101), 1), ((4096, 8), 33), ((8, 4096), 128), (BIG, 128)]


@pytest.mark.parametrize("hid,B", REPLAY_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"b{v}")
def test_replay_matches_float64_per_block_adam_and_whole_learner(monkeypatch, hid, B):
    """Per tick: every gradient block against float64 (the critic's, then the actor's through the UPDATED critic), ADAM, its moments
    and the soft update element-wise from the kernel's own gradient; after every tick the whole learner against DO.Learner.replay
    (_learner_matches: off ADAM's noise floor)."""
    torch, S, D = TW._mods()
    _at(monkeypatch, hid)
    sc = _scale(hid)
    monkeypatch.setattr(TW, "BLOCK_TOL", TW.BLOCK_TOL * sc)
    seed = 17 + 3 * B + hid[0] + hid[1]
    ring, h = TW._ring(torch, S, D, np.random.default_rng(seed), cap=6000)
    pa, pc = _nets(D, seed, hid)
    ag = D.Agent(seed=seed, hidden=hid, wide=True)
    ag.batch = B
    ag.set_params(actor=pa, critic=pc)
    ag.set_norm(h["s_min"], h["s_max"])
    whole = DO.Learner(pa, pc, h["s_min"], h["s_max"])
    opt_c, opt_a = DO.Adam(len(pc), DO.ETA_CRIT), DO.Adam(len(pa), DO.ETA_ACT)
    errs = {"critic": 0.0, "actor": 0.0, "learner": 0.0}
    noisy = {"critic": np.zeros(len(pc), bool), "actor": np.zeros(len(pa), bool)}
    ticks = (3,) if hid == BIG else (3, 4)
    for n_tick, tick in enumerate(ticks, 1):
        idx = ag.sample_indices(tick, len(ring))
        assert (idx == DO.sample_indices(ag.rng_seed, tick, B, len(ring))).all()
        s, a, r, s2, done = (h[k][idx] for k in ("s", "a", "r", "s2", "done"))
        p0 = _host(ag)
        Lr = DO.Learner(p0["actor"], p0["critic"], h["s_min"], h["s_max"])
        Lr.actor_t, Lr.critic_t = p0["actor_t"], p0["critic_t"]
        y = Lr.targets(r, s2, done.astype(bool))
        gc64, lc64 = Lr.critic_grad(s, a, y, dtype=np.float64)
        ag.replay(ring, tick=tick)
        torch.cuda.synchronize()
        gc = ag.grad_critic.cpu().numpy()
        e = TW._assert_blocks(gc, gc64, 11, 1, f"critic gradient at {hid}, batch {B}, tick {tick}")
        errs["critic"] = max(errs["critic"], *e.values())
        losses = ag.losses.cpu().numpy()
        assert abs(losses[0] - lc64) < 1e-4 * max(1.0, abs(lc64)), (tick, losses[0], lc64)
        crit = ag.critic.cpu().numpy()
        np.testing.assert_allclose(crit, opt_c.step(p0["critic"], gc), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.critic_t.cpu().numpy(), DO.soft_update(p0["critic_t"], crit), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.m_critic.cpu().numpy(), opt_c.m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(ag.v_critic.cpu().numpy(), opt_c.v, rtol=1e-6, atol=1e-15)
        Lr.critic = crit
        ga64, la64 = Lr.actor_grad(s, dtype=np.float64)
        ga = ag.grad_actor.cpu().numpy()
        e = TW._assert_blocks(ga, ga64, 9, 2, f"actor gradient at {hid}, batch {B}, tick {tick}")
        errs["actor"] = max(errs["actor"], *e.values())
        assert abs(losses[1] - la64) < 1e-4 * max(1.0, abs(la64)), (tick, losses[1], la64)
        act = ag.actor.cpu().numpy()
        np.testing.assert_allclose(act, opt_a.step(p0["actor"], ga), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.actor_t.cpu().numpy(), DO.soft_update(p0["actor_t"], act), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.m_actor.cpu().numpy(), opt_a.m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(ag.v_actor.cpu().numpy(), opt_a.v, rtol=1e-6, atol=1e-15)
        opt_c.m, opt_c.v = ag.m_critic.cpu().numpy(), ag.v_critic.cpu().numpy()
        opt_a.m, opt_a.v = ag.m_actor.cpu().numpy(), ag.v_actor.cpu().numpy()
        whole.replay(s, a, r, s2, done.astype(bool))
        noisy["critic"] |= _noisy(gc64, 11, 1, DO.ETA_CRIT, 3e-6 * sc)
        noisy["actor"] |= _noisy(ga64, 9, 2, DO.ETA_ACT, 3e-6 * sc)
        err = _learner_matches(ag, whole, noisy, {"critic": (gc, gc64), "actor": (ga, ga64)}, 3e-6 * sc, n_tick,
                               f"replay {hid} batch {B} tick {tick}")
        errs["learner"] = max(errs["learner"], err)
    print(f"replay {hid} batch {B}: block errors {errs['critic']:.3g} / {errs['actor']:.3g} (bound {TW.BLOCK_TOL:.3g}), "
          f"whole learner {errs['learner']:.3g} (bound {3e-6 * sc:.3g})")


@pytest.mark.parametrize("hid", [(16, 64), (17, 65), (260, 101)], ids=lambda h: f"{h[0]}x{h[1]}")
def test_fused_step_equals_act_then_oracle_step_and_fills_ring(monkeypatch, hid):
    """(16, 64): l2 in one head half, V4; (17, 65) and (260, 101): not V4."""
    torch, S, D = TW._mods()
    _at(monkeypatch, hid)
    n, nsteps, wc = 2085, 2, 333
    tab = S.tables.synthetic_table("train", 98)
    env = S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    ref = oracle_c.Batch(n, 72, tab, oracle_c.profile(98))
    ag = D.Agent(seed=77, hidden=hid, wide=True)
    pa, _ = _nets(D, 77, hid)
    ag.set_params(actor=pa)
    env.reset_(5, episode=0)
    st0 = env.state
    ag.set_norm(st0.min(0), st0.max(0))
    ref.set_state(st0, env.idx)
    ring = D.ReplayRing(5000)
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    rew = torch.empty(n, dtype=torch.float64, device="cuda")
    rew32 = torch.empty(n, dtype=torch.float32, device="cuda")
    ret = torch.zeros(n, dtype=torch.float64, device="cuda")
    pos, tot, worst = 0, np.zeros(n), 0.0
    for t in range(nsteps):
        pre = env.state
        win = D.RingWindow(pos % ring.capacity, wc, (t * wc) % n)
        ag.act_step(env, train=True, tick=t, a_out=a_out, rewards=rew, rewards_f32=rew32, returns_acc=ret, ring=ring, window=win)
        env.check_error()
        a = a_out.cpu().numpy()
        want = DO.act(pa, pre, st0.min(0), st0.max(0), True, seed=77, tick=t, dtype=np.float64)
        err = float(np.abs(a - want).max())
        assert err < 5e-6 + TW.ATOL, (t, err)
        worst = max(worst, err)
        rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
        assert rc == 0
        r = rew.cpu().numpy()
        tot += r
        assert (U.bits64(r) == U.bits64(r_ref)).all() and (U.bits32(env.state) == U.bits32(o_ref)).all()
        assert (rew32.cpu().numpy() == r_ref.astype(np.float32)).all()
        rel = (np.arange(n) - (t * wc) % n) % n
        sel = np.where(rel < wc)[0]
        slots = (pos + rel[sel]) % ring.capacity
        assert (U.bits32(ring.s.cpu().numpy()[slots]) == U.bits32(pre[sel])).all()
        assert (U.bits32(ring.s2.cpu().numpy()[slots]) == U.bits32(o_ref[sel])).all()
        assert (U.bits32(ring.a.cpu().numpy()[slots]) == U.bits32(a[sel])).all()
        assert (ring.r.cpu().numpy()[slots] == r_ref[sel].astype(np.float32)).all()
        pos += wc
    assert (env.idx == ref.idx()).all() and (env.step == nsteps).all() and (ret.cpu().numpy() == tot).all()
    env.close()
    print(f"fused step {hid}: max |err| {worst:.3g} (bound {5e-6 + TW.ATOL:.3g})")


@pytest.mark.parametrize("hid", [(17, 65), (129, 257), (1031, 70)], ids=lambda h: f"{h[0]}x{h[1]}")
def test_tracking_pass_at_odd_and_long_l1(monkeypatch, hid):
    """k_track<true>: odd l1 (the scalar tail of layer 2's k loop), l1 = 1031 > 512 (three trips of layer 1's stride loop, 4 KB of
    dynamic LDS).  Every hour's targets against float64, every results row reproduced bit for bit by the C oracle from them."""
    torch, S, D = TW._mods()
    _at(monkeypatch, hid)
    H = importlib.import_module(U.PKG_NAME + ".harness")
    ev = S.tables.synthetic_table("eval", 98)
    env = S.ShemsBatch(1, 1439, [ev], [S.make_config(98, 0, ev.shape[0])])
    st = ev[:, [1, 1, 0, 2, 3, 4, 5, 6, 7]].copy()
    st[:, 0] = np.linspace(0, 6.75, len(st))
    lo, hi = st.min(0), st.max(0)
    ag = D.Agent(seed=4, hidden=hid, wide=True)
    pa, _ = _nets(D, 4, hid)
    ag.set_params(actor=pa)
    ag.set_norm(lo, hi)
    steps, bound, worst, top = 200, 1e-5 * _scale(hid), 0.0, 0.0
    total, res = H.inference(env, ag, track=1, num_steps=steps)
    env.close()
    assert res.shape == (steps, 23)
    ref = oracle_c.Batch(1, 1439, ev, oracle_c.profile(98)); ref.reset(True)
    for t in range(steps):
        a = DO.act(pa, ref.state(), lo, hi, False, dtype=np.float64)
        tgt = res[t, [21, 2]].astype(np.float32)[None]
        err = float(np.abs(oracle_c.scale_action(a) - tgt).max())
        assert err < bound, (t, err)
        worst, top = max(worst, err), max(top, float(np.abs(a).max()))
        rc, _, _, rr = ref.step(tgt, 1, want_results=True)
        assert rc == 0 and (U.bits64(rr[0]) == U.bits64(res[t])).all(), t
    assert top > 0.3
    if D.is_wide(hid):                                  # inference_many takes a wide actor's own layout
        many = S.ShemsBatch(2, 1439, [ev], [S.make_config(98, 0, ev.shape[0])])
        tot, resm = H.inference_many(many, np.stack([pa, _nets(D, 5, hid)[0]]), lo, hi, num_steps=steps, hidden=hid)
        many.close()
        assert resm.shape == (2, steps, 23) and (U.bits64(resm[0]) == U.bits64(res)).all() and tot[0] != tot[1]
    print(f"tracking {hid}: max |err| {worst:.3g} (bound {bound:.3g})")


# ---- sub-batches of a single Agent ---------------------------------------------------------------------------------------------

_capi = None


def _sub_slots(ag, sb, ring, torch):
    """The ring slots (wide) / the s rows (tuned) sub-batch `sb`'s last critic pass sampled."""
    global _capi
    _capi = _capi or importlib.import_module(U.PKG_NAME + "._capi")
    d = ag._ddpg_args(sb)
    if ag.wide:
        slots = np.empty(sb["batch"], np.int32)
        _capi.check(ag.L.shems_wide_batch_slots(C.byref(d), *ag.whidden, slots.ctypes.data_as(C.c_void_p), ag._stream()))
        return slots
    obs = torch.empty((sb["batch"], 9), dtype=torch.float32, device=ag.device)
    _capi.check(ag.L.shems_ddpg_batch_obs_dev(C.byref(d), C.byref(ring.struct()), C.c_void_p(obs.data_ptr()), ag._stream()))
    return obs.cpu().numpy()


@pytest.mark.parametrize("B,sizes", [(129, [65, 64]), (257, [86, 86, 85]), (1024, [128] * 8)], ids=["129", "257", "1024"])
@pytest.mark.parametrize("hid,wide", [((250, 500), False), ((129, 257), True)], ids=["tuned", "wide"])
def test_sub_batches_match_the_oracle_on_the_whole_batch(monkeypatch, hid, wide, B, sizes):
    """BATCH_SIZE above one pass: near-equal sub-batches, sub-batch i sampled with tick `tick * 8 + i`, gradients combined with weights
    b_i / B, one ADAM step.  Per tick, from the kernel's own pre-update state: the combined gradients per block against float64 over
    the same transitions as one minibatch, the losses, ADAM, its moments and the soft update from the combined gradient; and the whole
    learner against the oracle's replay of those minibatches (3e-6 off ADAM's noise floor).  The actor's head bias is (0.35, -0.25),
    where the whole-learner comparison without the floor once failed on the tuned path at batch 1024 (5.4e-5)."""
    torch, S, D = TW._mods()
    _at(monkeypatch, hid)
    ring, h = TW._ring(torch, S, D, np.random.default_rng(B))
    pa, pc = _nets(D, 31 + B, hid)
    pa[-2:] = [0.35, -0.25]
    ag = D.Agent(seed=31 + B, hidden=hid, wide=wide)
    assert ag.wide is wide
    ag.batch = B
    ag.set_params(actor=pa, critic=pc)
    ag.set_norm(h["s_min"], h["s_max"])
    subs = ag.sub_batches()
    assert [sb["batch"] for sb in subs] == sizes
    L = DO.Learner(pa, pc, h["s_min"], h["s_max"])
    worst = {"critic": 0.0, "actor": 0.0, "learner": 0.0}
    opt_c, opt_a = DO.Adam(len(pc), DO.ETA_CRIT), DO.Adam(len(pa), DO.ETA_ACT)
    noisy = {"critic": np.zeros(len(pc), bool), "actor": np.zeros(len(pa), bool)}
    for n_tick, tick in enumerate((5, 6), 1):
        parts = [ag.sample_indices(tick * 8 + i, len(ring), batch=b) for i, b in enumerate(sizes)]
        for i, (b, p) in enumerate(zip(sizes, parts)):
            assert (p == DO.sample_indices(ag.rng_seed, tick * 8 + i, b, len(ring))).all()
        idx = np.concatenate(parts)
        assert idx.shape == (B,)
        s, a, r, s2, done = (h[k][idx] for k in ("s", "a", "r", "s2", "done"))
        pre = _host(ag)
        Lk = DO.Learner(pre["actor"], pre["critic"], h["s_min"], h["s_max"])        # the kernel's own pre-update state
        Lk.actor_t, Lk.critic_t = pre["actor_t"], pre["critic_t"]
        gc64, lc64 = Lk.critic_grad(s, a, Lk.targets(r, s2, done.astype(bool)), dtype=np.float64)
        L.replay(s, a, r, s2, done.astype(bool))
        ag.replay(ring, tick=tick)
        torch.cuda.synchronize()
        for i, sb in enumerate(subs):                   # each sub-batch drew its own ticks' slots
            got = _sub_slots(ag, sb, ring, torch)
            assert (got == parts[i]).all() if wide else (U.bits32(got) == U.bits32(h["s"][parts[i]])).all(), (tick, i)
        gc = ag.grad_critic.cpu().numpy()
        e = TW._assert_blocks(gc, gc64, 11, 1, f"combined critic gradient, batch {B}, tick {tick}")
        worst["critic"] = max(worst["critic"], *e.values())
        crit = ag.critic.cpu().numpy()
        np.testing.assert_allclose(crit, opt_c.step(pre["critic"], gc), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.critic_t.cpu().numpy(), DO.soft_update(pre["critic_t"], crit), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.m_critic.cpu().numpy(), opt_c.m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(ag.v_critic.cpu().numpy(), opt_c.v, rtol=1e-6, atol=1e-15)
        Lk.critic = crit
        ga64, la64 = Lk.actor_grad(s, dtype=np.float64)
        ga = ag.grad_actor.cpu().numpy()
        e = TW._assert_blocks(ga, ga64, 9, 2, f"combined actor gradient, batch {B}, tick {tick}")
        worst["actor"] = max(worst["actor"], *e.values())
        act = ag.actor.cpu().numpy()
        np.testing.assert_allclose(act, opt_a.step(pre["actor"], ga), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.actor_t.cpu().numpy(), DO.soft_update(pre["actor_t"], act), rtol=0, atol=1e-7)
        np.testing.assert_allclose(ag.m_actor.cpu().numpy(), opt_a.m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(ag.v_actor.cpu().numpy(), opt_a.v, rtol=1e-6, atol=1e-15)
        opt_c.m, opt_c.v = ag.m_critic.cpu().numpy(), ag.v_critic.cpu().numpy()
        opt_a.m, opt_a.v = ag.m_actor.cpu().numpy(), ag.v_actor.cpu().numpy()
        losses = ag.losses.cpu().numpy()
        assert abs(losses[0] - lc64) < 1e-4 * max(1.0, abs(lc64)) and abs(losses[1] - la64) < 1e-4 * max(1.0, abs(la64)), (tick, losses)
        noisy["critic"] |= _noisy(gc64, 11, 1, DO.ETA_CRIT, 3e-6)
        noisy["actor"] |= _noisy(ga64, 9, 2, DO.ETA_ACT, 3e-6)
        err = _learner_matches(ag, L, noisy, {"critic": (gc, gc64), "actor": (ga, ga64)}, 3e-6, n_tick,
                               f"sub-batches {hid} batch {B} tick {tick}")
        worst["learner"] = max(worst["learner"], err)
    print(f"sub-batches {hid} batch {B}: blocks {worst['critic']:.3g} / {worst['actor']:.3g} (bound {TW.BLOCK_TOL:.3g}), whole learner "
          f"{worst['learner']:.3g} (bound 3e-06)")


# ---- wide learner groups -------------------------------------------------------------------------------------------------------

def _records(hids, batches):
    return [dict(hidden=h, batch=b, gamma=(0.95, 0.99, 0.999)[l % 3], tau=(1e-3, 5e-3)[l % 2], eta_act=(1e-4, 5e-4, 1e-5)[l % 3],
                 eta_crit=(1e-3, 5e-3, 1e-4)[l % 3], sigma=0.1 + 0.05 * (l % 3), mu=0.02 * (l % 2))
            for l, (h, b) in enumerate(zip(hids, batches))]


GROUPS = {
    # (129, 257), not V4; batches up to 129: pass width P = 160 (K = 160 in the weight-gradient products)
    "A": dict(H=(129, 257), ticks=(3, 4), recs=_records([(1, 1), (3, 5), (17, 65), (64, 4), (129, 257), (100, 3), (129, 1)],
                                                        [1, 33, 128, 129, 1, 33, 128])),
    # (64, 64), V4, l2 inside one head half; batches up to 256: P = 256
    "B": dict(H=(64, 64), ticks=(3, 4), recs=_records([(64, 64), (1, 1), (32, 16), (64, 3), (5, 64)], [256, 1, 100, 200, 64])),
    # (4096, 4096): the widest networks at the widest pass, one tick
    "C": dict(H=BIG, ticks=(3,), recs=_records([BIG, BIG], [128, 256])),
}


def _wide_group(name, E=32, perturb=None):
    """Group `name` with every learner's heads lifted (_boost), b2 set (_lift_b2) and ~5 % terminal transitions; perturb = k: learner
    k's actor and critic shifted (targets kept)."""
    torch = TG._mods()[0]
    g = GROUPS[name]
    env, grp = TG._group(len(g["recs"]), E, hparams=g["recs"], hidden=g["H"])
    assert grp.form == "wide" and grp.hidden == g["H"]
    rng = np.random.default_rng(5)
    for l, ag in enumerate(grp.learners):
        hid = g["recs"][l]["hidden"]
        TG._boost(ag, rng, hid)
        pa, pc = _lift_b2(ag.export_actor(), ag.export_critic(), hid, rng)
        ag.set_params(actor=pa, critic=pc)
        ring = grp.rings[l]
        ring.done.copy_(torch.from_numpy((rng.random(ring.capacity) < 0.05).astype(np.uint8)))
    if perturb is not None:
        ag = grp.learners[perturb]
        pa, pc = ag.export_actor(), ag.export_critic()
        pa[:50] += 0.01
        pc[:50] -= 0.01
        ag.set_params(actor=pa, critic=pc, sync_targets=False)
    return env, grp


@pytest.mark.parametrize("name", list(GROUPS))
def test_wide_group_matches_float64_per_learner_and_block(monkeypatch, name):
    torch, S, D, G = TG._mods()
    g = GROUPS[name]
    _at(monkeypatch, g["H"])
    sc = _scale(g["H"])
    monkeypatch.setattr(TG, "BLOCK_TOL", TG.BLOCK_TOL * sc)
    monkeypatch.setattr(TG, "HID", g["H"])                                # TG._pad_mask pads into the group's width
    env, grp = _wide_group(name)
    assert grp.max_batch == max(r["batch"] for r in g["recs"])
    host = {}
    for l, ag in enumerate(grp.learners):
        h = grp.hparams[l]
        ring = grp.rings[l]
        pa, pc = ag.actor.cpu().numpy(), ag.critic.cpu().numpy()
        host[l] = dict(pa=pa, pc=pc, pat=ag.actor_t.cpu().numpy(), pct=ag.critic_t.cpu().numpy(), s=ring.s.cpu().numpy(), a=ring.a.cpu().numpy(),
                       r=ring.r.cpu().numpy(), s2=ring.s2.cpu().numpy(), done=ring.done.cpu().numpy(), s_min=ag.s_min.cpu().numpy(),
                       s_max=ag.s_max.cpu().numpy(), opt_c=DO.Adam(len(pc), f32(h["eta_crit"])), opt_a=DO.Adam(len(pa), f32(h["eta_act"])),
                       batch=h["batch"], gamma=f32(h["gamma"]), tau=f32(h["tau"]))
    worst = 0.0
    for tick in g["ticks"]:
        grp.replay(tick=tick)
        torch.cuda.synchronize()
        for l, ag in enumerate(grp.learners):
            e = TG._learner_tick_matches_float64(grp, l, ag, host[l], tick)
            worst = max(worst, *e["critic"].values(), *e["actor"].values(), 0.0)
    for l, ag in enumerate(grp.learners):                                  # padded units stay exactly zero
        hid = g["recs"][l]["hidden"]
        for net, (i, o) in (("actor", (9, 2)), ("critic", (11, 1))):
            pad = TG._pad_mask(D, hid, i, o)
            assert pad.any() == (hid != g["H"]), l
            for k in (net, net + "_t", "m_" + net, "v_" + net, "grad_" + net):
                assert not getattr(ag, k).cpu().numpy()[pad].any(), (l, k)
    env.close()
    print(f"group {name} {g['H']}: worst block error {worst:.3g} (bound {TG.BLOCK_TOL:.3g})")


@pytest.mark.parametrize("epl", [32, 160])
@pytest.mark.parametrize("name", list(GROUPS))
def test_wide_group_fused_step_equals_act_then_oracle_step(monkeypatch, name, epl):
    """envs per learner 32 (with a ring window into every learner's ring) and 160 (> 128, not a multiple: a partial row tile in
    k_wgemm128_g, the learner offsets of k_act_tail_g off the 128 grid)."""
    torch, S, D, G = TG._mods()
    g = GROUPS[name]
    _at(monkeypatch, g["H"])
    env0, grp = _wide_group(name)
    L = len(g["recs"])
    env = env0 if epl == 32 else TG._env(S, L * epl)
    if epl != 32:
        env.reset_(9, episode=1)
    n = L * epl
    tab = S.tables.synthetic_table("train", 98)
    ref = oracle_c.Batch(n, 72, tab, oracle_c.profile(98))
    ref.set_state(env.state, env.idx)
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    ret = torch.zeros(n, dtype=torch.float64, device="cuda")
    wc, bound, worst = 16, 5e-6 * _scale(g["H"]), 0.0
    nets = [(ag.actor.cpu().numpy(), ag.s_min.cpu().numpy(), ag.s_max.cpu().numpy()) for ag in grp.learners]
    for t in range(2):
        pre = env.state
        pos = grp.rings[0].pos
        win = (pos, wc, (t * wc) % epl) if epl == 32 else None
        grp.act_step(env, train=True, tick=7 + t, a_out=a_out, returns_acc=ret, window=win, envs_per_learner=epl)
        env.check_error()
        a = a_out.cpu().numpy()
        zn = DO.gauss_noise(grp.rng_seed, 7 + t, n)
        for l, (pa, lo, hi) in enumerate(nets):
            sl = slice(l * epl, (l + 1) * epl)
            clean = DO.act(pa, pre[sl], lo, hi, False, dtype=np.float64)
            want = np.clip(clean + (f32(g["recs"][l]["mu"]) + f32(g["recs"][l]["sigma"]) * zn[sl]), -1, 1)
            err = float(np.abs(a[sl] - want).max())
            assert err < bound, (l, t, err)
            worst = max(worst, err)
        rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
        assert rc == 0 and (U.bits32(env.state) == U.bits32(o_ref)).all()
        if win is not None:
            for l in range(L):
                rel = (np.arange(epl) - win[2]) % epl
                sel = np.where(rel < wc)[0]
                slots = (pos + rel[sel]) % grp.capacity
                ring = grp.rings[l]
                gi = l * epl + sel
                assert (U.bits32(ring.s.cpu().numpy()[slots]) == U.bits32(pre[gi])).all(), (l, t)
                assert (U.bits32(ring.s2.cpu().numpy()[slots]) == U.bits32(o_ref[gi])).all(), (l, t)
                assert (U.bits32(ring.a.cpu().numpy()[slots]) == U.bits32(a[gi])).all(), (l, t)
                assert (ring.r.cpu().numpy()[slots] == r_ref[gi].astype(np.float32)).all(), (l, t)
    if env is not env0:
        env.close()
    env0.close()
    print(f"group {name} fused step, {epl} envs per learner: max |err| {worst:.3g} (bound {bound:.3g})")


@pytest.mark.parametrize("name", list(GROUPS))
def test_wide_group_learners_are_independent(name):
    """Learner k's networks perturbed: after the same updates every other learner's slab (networks, moments, gradients, workspace, ring)
    is bit-identical to the unperturbed run's, and learner k's is not."""
    torch = TG._mods()[0]
    g = GROUPS[name]
    k = len(g["recs"]) // 2
    slabs = []
    for perturb in (None, k):
        env, grp = _wide_group(name, perturb=perturb)
        for tick in g["ticks"]:
            grp.replay(tick=tick)
        torch.cuda.synchronize()
        slabs.append(grp.slab.cpu())
        env.close()
        del grp
    for l in range(len(g["recs"])):
        same = torch.equal(slabs[0][l].view(torch.int32), slabs[1][l].view(torch.int32))
        assert same == (l != k), l

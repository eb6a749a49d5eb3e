"""GPU tests of per-learner exploration and ring sizes in learner groups (shems_group_xparams, the *_x entry points): the fused step
with Ornstein-Uhlenbeck noise against the float64 restatement per learner, a "gn" group on the *_x path against today's path byte for
byte in every fused-step form, per-learner ring sizes against plain groups of that capacity, and the input template's 27 points
(RL-SHEMS/input.jl:58-100) training as one wide group."""
import importlib

import numpy as np
import pytest

import util as U
from util import oracle_c
import ddpg_oracle as DO

pytestmark = pytest.mark.gpu
f32 = np.float32
HID = (300, 600)
# (sigma, mu, theta) cycled over the learners
OU_CYCLE = ((0.1, 0.0, 0.15), (0.3, 0.0, 0.2), (0.2, -0.1, 0.0), (0.0, 0.2, 0.15))
DT = 1e-2


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    return torch, S, D, G


def _env(S, n):
    tab = S.tables.synthetic_table("train", 98)
    return S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()


def _group(L, E, cap=2400, **kw):
    torch, S, D, G = _mods()
    env = _env(S, L * E)
    grp = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=cap, **kw)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    env.reset_(9, episode=1)
    return env, grp


def _same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def _boost(ag, hid):
    """Lift the 3e-3 output layer of the learner's actor (its own units only: padding stays zero) so that tanh is exercised."""
    pa = ag.export_actor()
    pa[-(2 * hid[1] + 2):-2] *= 40.0
    pa[-2:] = [0.3, -0.2]
    ag.set_params(actor=pa)


# ---- the fused step with OU noise against the float64 restatement ------------------------------------------------------------------
def _ou_step_vs_oracle(monkeypatch, L, E, hidden_of, **kw):
    """Four training steps of an "ou" group cycling OU_CYCLE: per learner slice, oracle act(noise="ou") with the draws of the GLOBAL env
    index (the oracle draws by the index inside the array it is given: its draw function is pointed at the slice of the global draws
    for the call), the OU state, noise_acc and the C oracle's step on the produced actions; then an evaluation step."""
    torch, S, D, G = _mods()
    recs = [dict(sigma=OU_CYCLE[l % 4][0], mu=OU_CYCLE[l % 4][1], theta=OU_CYCLE[l % 4][2], **hidden_of(l)) for l in range(L)]
    env, grp = _group(L, E, noise_type="ou", dt=DT, hparams=recs, **kw)
    n = grp.n_envs
    assert grp.ou_state.shape == (n, 2) and not grp.ou_state.any().item()
    for l, ag in enumerate(grp.learners):
        _boost(ag, ag.hidden)
        assert (ag.noise_type, ag.dt) == ("ou", DT) and ag.theta == pytest.approx(recs[l]["theta"])
        assert ag.sigma == pytest.approx(recs[l]["sigma"]) and ag.mu == pytest.approx(recs[l]["mu"])
    tab = S.tables.synthetic_table("train", 98)
    ref = oracle_c.Batch(n, 72, tab, oracle_c.profile(98))
    ref.set_state(env.state, env.idx)
    X = np.zeros((n, 2), f32)                     # the oracle's OUNoise.X of every env
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    acc = torch.zeros(n, dtype=torch.float32, device="cuda")
    real_draws = DO.gauss_noise
    for t in range(4):
        pre = env.state
        acc.zero_()
        grp.act_step(env, train=True, tick=7 + t, a_out=a_out, noise_acc=acc, window=(grp.rings[0].pos, 16, (t * 16) % E))
        env.check_error()
        a = a_out.cpu().numpy()
        zn = real_draws(grp.rng_seed, 7 + t, n)
        for l, ag in enumerate(grp.learners):
            sl = slice(l * E, (l + 1) * E)
            sg, mu, th = OU_CYCLE[l % 4]
            Xl = X[sl].copy()
            with monkeypatch.context() as m:
                m.setattr(DO, "gauss_noise", lambda seed, tick, cnt, _z=zn[sl]: _z)
                want = DO.act(ag.actor.cpu().numpy(), pre[sl], ag.s_min.cpu().numpy(), ag.s_max.cpu().numpy(), True, seed=grp.rng_seed, tick=7 + t,
                              mu=mu, sigma=sg, noise="ou", ou_state=Xl, theta=th, dt=DT, dtype=np.float64)
            X[sl] = Xl
            assert np.abs(a[sl] - want).max() < 2e-5, (l, t)
        got_x = grp.ou_state.cpu().numpy()
        assert np.abs(got_x - X).max() < 1e-5, t
        assert np.abs(acc.cpu().numpy() - 0.5 * (got_x[:, 0] + got_x[:, 1])).max() < 1e-5, t
        rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
        assert rc == 0
        assert (U.bits32(env.state) == U.bits32(o_ref)).all(), t
    # the state accumulated.  After 4 steps X is N(~0, (2 sigma sqrt(dt))^2): a standard deviation of 0.02 at sigma = 0.1, so the spread
    # of a learner's 128 values is taken peak to peak (about 5 standard deviations); the sigma = 0.3 learners pooled are also held to
    # the figure of tests/test_policy_gpu.py::test_ou_and_epsilon_noise_branches, which runs at that sigma.
    for l in range(L):
        sl = slice(l * E, (l + 1) * E)
        if OU_CYCLE[l % 4][0] > 0:
            assert np.ptp(X[sl]) > 0.03 and np.ptp(got_x[sl]) > 0.03, l
        else:                                     # sigma = 0: every env of the learner drifts to mu together
            assert np.ptp(got_x[sl]) == 0 and 0 < got_x[sl][0, 0] < 0.2, l
    big = np.concatenate([got_x[l * E:(l + 1) * E] for l in range(L) if OU_CYCLE[l % 4][0] == 0.3])
    assert np.abs(big).std() > 0.03
    # evaluation: no noise, and the OU state is not touched
    before = grp.ou_state.clone()
    pre = env.state
    grp.act_step(env, train=False, tick=99, a_out=a_out)
    a = a_out.cpu().numpy()
    for l, ag in enumerate(grp.learners):
        sl = slice(l * E, (l + 1) * E)
        clean = DO.act(ag.actor.cpu().numpy(), pre[sl], ag.s_min.cpu().numpy(), ag.s_max.cpu().numpy(), False, dtype=np.float64)
        assert np.abs(a[sl] - clean).max() < 2e-5, l
    assert torch.equal(grp.ou_state.view(torch.int32), before.view(torch.int32))
    env.close()


@pytest.mark.parametrize("tiled", [True, False])
def test_ou_fused_step_matches_float64_per_learner_throughput_form(monkeypatch, tiled):
    _ou_step_vs_oracle(monkeypatch, 16, 64, lambda l: {}, tiled=tiled)


def test_ou_fused_step_matches_float64_per_learner_wide_form(monkeypatch):
    monkeypatch.setattr(DO, "L1", HID[0])
    monkeypatch.setattr(DO, "L2", HID[1])
    hid = [(300, 600), (200, 400), (250, 500), (150, 300)]
    _ou_step_vs_oracle(monkeypatch, 4, 64, lambda l: dict(hidden=hid[l]), form="wide")


# ---- a "gn" group on the *_x path leaves today's bytes, in every fused-step form ----------------------------------------------------
def _run(env, grp, steps=2, window=None):
    torch = grp.torch
    out = []
    for t in range(steps):
        a = torch.empty((grp.n_envs, 2), dtype=torch.float32, device="cuda")
        ret = torch.zeros(grp.n_envs, dtype=torch.float64, device="cuda")
        grp.act_step(env, train=True, tick=10 + t, a_out=a, returns_acc=ret, window=(grp.rings[0].pos, *grp.ring_window(72, window)))
        grp.tick += 1
        grp.replay(tick=20 + t)
        out.append((a.cpu().numpy(), ret.cpu().numpy()))
    grp.flux_()
    torch.cuda.synchronize()
    env.check_error()
    return out


# the shapes of the all-forms tests, and the remaining forms a group's dispatcher picks (k_actg<1, 4, 2, 2>, k_act<4, 4, 2>, k_act2)
X_FORMS = [(48, 32), (16, 128), (300, 96), (520, 64), (20, 1024), (160, 32), (256, 128), (1, 16384)]


@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("L,E", X_FORMS)
def test_gn_group_on_the_x_path_equals_todays_path_bitwise(L, E, tiled):
    torch, S, D, G = _mods()
    cap = 400 if L * E > 8192 else 2400
    env_a, ga = _group(L, E, cap=cap, tiled=tiled, hparams=[{}] * L)
    env_b, gb = _group(L, E, cap=cap, tiled=tiled, hparams=[{"mem_size": cap}] + [{}] * (L - 1))
    assert not ga._x and gb._x and gb.form == ga.form == "throughput" and gb.tiled == tiled and gb.ou_state is None
    ra, rb = _run(env_a, ga), _run(env_b, gb)
    for (aa, ret_a), (ab, ret_b) in zip(ra, rb):
        assert _same_bits(aa, ab) and _same_bits(ret_a, ret_b)
    assert _same_bits(env_a.state, env_b.state)
    for ring_a, ring_b in zip(ga.rings, gb.rings):
        assert ring_a.pushed == ring_b.pushed
        assert torch.equal(ring_a.s2.view(torch.int32), ring_b.s2.view(torch.int32)) and torch.equal(ring_a.a.view(torch.int32), ring_b.a.view(torch.int32))
    assert gb._pushed_dev.cpu().tolist() == [r.pushed for r in gb.rings]
    # networks, targets, moments, losses, workspace and rings of every learner
    assert torch.equal(ga.slab.view(torch.int32), gb.slab.view(torch.int32))


def test_gn_wide_group_on_the_x_path_equals_todays_path_bitwise():
    torch, S, D, G = _mods()
    hid = [(300, 600), (200, 400), (250, 500), (150, 300)]
    recs = [dict(hidden=hid[l % 4], batch=(50, 120, 200)[l % 3], sigma=0.1 + 0.05 * (l % 3)) for l in range(6)]
    env_a, ga = _group(6, 64, form="wide", hparams=recs)
    env_b, gb = _group(6, 64, form="wide", hparams=[dict(recs[0], mem_size=2400)] + recs[1:])
    assert not ga._x and gb._x
    ra, rb = _run(env_a, ga, window=16), _run(env_b, gb, window=16)
    for (aa, ret_a), (ab, ret_b) in zip(ra, rb):
        assert _same_bits(aa, ab) and _same_bits(ret_a, ret_b)
    assert _same_bits(env_a.state, env_b.state)
    assert torch.equal(ga.slab.view(torch.int32), gb.slab.view(torch.int32))


# ---- per-learner ring sizes against plain groups of that capacity ------------------------------------------------------------------
def _episodes(env, grp, episodes=2, steps=12, wc=16):
    """LearnerGroup.episode_ with the actions kept: `episodes` x `steps` fused steps + updates with a window of wc."""
    torch = grp.torch
    acts = []
    for ep in range(episodes):
        env.reset_(3, episode=ep + 1)
        for step in range(steps):
            a = torch.empty((grp.n_envs, 2), dtype=torch.float32, device="cuda")
            grp.act_step(env, train=True, tick=(ep + 1) * 4096 + step, a_out=a, window=(grp.rings[0].pos, *grp.ring_window(steps, wc)))
            grp.replay()
            grp.tick += 1
            acts.append(a.cpu().numpy())
    grp.flux_()
    torch.cuda.synchronize()
    env.check_error()
    return np.stack(acts)


@pytest.mark.parametrize("form", ["throughput", "wide"])
def test_per_learner_ring_sizes_equal_plain_groups_of_that_capacity(form):
    torch, S, D, G = _mods()
    L, E, CAP, sizes = 6, 64, 720, (96, 144, 720)
    base = [dict(batch=(50, 120, 200)[l % 3]) if form == "wide" else {} for l in range(L)]
    mem = [sizes[l % 3] for l in range(L)]

    def make(cap, recs):
        env = _env(S, L * E)
        grp = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=cap, form=form, hparams=recs)
        grp.populate_memory(env, seed=5)
        return env, grp

    env_a, ga = make(CAP, [dict(base[l], mem_size=mem[l]) for l in range(L)])
    assert ga._x and ga.form == form and [r.capacity for r in ga.rings] == mem and ga.ring_window(72)[0] == 1
    # populate_memory leaves every ring full, at its own push position
    assert [(r.pushed, r.pos, len(r)) for r in ga.rings[:3]] == [(144, 48, 96), (144, 0, 144), (720, 0, 720)]
    ga.min_max_buffer()
    acts_a = _episodes(env_a, ga)
    assert ga._pushed_dev.cpu().tolist() == [r.pushed for r in ga.rings]
    lay = ga.layout
    for c in sizes:
        env_b, gb = make(c, base if form == "wide" else None)
        assert not gb._x and gb.form == form
        gb.min_max_buffer()
        acts_b = _episodes(env_b, gb)
        for l in range(L):
            if mem[l] != c:
                continue
            sl = slice(l * E, (l + 1) * E)
            assert _same_bits(acts_a[:, sl], acts_b[:, sl]), (c, l)
            la, lb = ga.learners[l], gb.learners[l]
            for k in ("s_min", "s_max", "actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic"):
                assert torch.equal(getattr(la, k).view(torch.int32), getattr(lb, k).view(torch.int32)), (c, l, k)
            ra, rb = ga.rings[l], gb.rings[l]
            assert (ra.pushed, ra.pos, len(ra)) == (rb.pushed, rb.pos, len(rb)) and ra.capacity == c
            for k in ("s", "a", "r", "s2", "done"):
                x, y = getattr(ra, k), getattr(rb, k)
                assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (c, l, k)
            # the slots past the learner's ring size were never written
            for name, width in (("ring_s", 9), ("ring_a", 2), ("ring_r", 1), ("ring_s2", 9)):
                o, cnt = lay[name]
                assert not ga.slab[l, o + c * width:o + cnt].any().item(), (c, l, name)
            o, cnt = lay["ring_done"]
            assert not ga.slab[l, o:o + cnt].view(torch.uint8)[c:CAP].any().item(), (c, l)
        env_b.close()
    env_a.close()


def test_x_path_preconditions():
    torch, S, D, G = _mods()
    env = _env(S, 4 * 32)
    grp = G.LearnerGroup(4, 32, capacity=720, hparams=[{"mem_size": 96}, {}, {}, {}])
    with pytest.raises(S.ShemsError, match="learner 0 is empty"):            # nothing pushed yet: no length to sample from
        grp.replay()
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    env.reset_(9, episode=1)
    with pytest.raises(ValueError, match="smallest ring"):
        grp.act_step(env, train=True, tick=0, window=(0, 128, 0))
    env.close()


# ---- the grid itself ---------------------------------------------------------------------------------------------------------------
def test_the_whole_input_grid_trains_as_one_group():
    torch, S, D, G = _mods()
    recs, points = G.input_grid(range(27))
    L, E = 27, 32
    env = _env(S, L * E)
    grp = G.LearnerGroup(L, E, seed=21, rng_seed=77, capacity=G.INPUT_CAPACITY, form="wide", noise_type="ou", hparams=recs)
    assert grp.hidden == HID and grp.max_batch == 200 and grp._x
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    ret = grp.episode_(env, num_steps=72, rng_ep=3, episode=1, window_count=1)
    torch.cuda.synchronize()
    env.check_error()
    assert grp.updates == 72 and bool(torch.isfinite(ret).all())
    assert bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())     # parameters, targets, moments, gradients, normalisation, losses
    assert bool(grp.ou_state.any().item())
    for l, (ag, ring) in enumerate(zip(grp.learners, grp.rings)):
        r = recs[l]
        assert len(ring) == r["mem_size"] == ring.capacity
        assert ag.batch == r["batch"] and ag.hidden == r["hidden"] and ag.theta == pytest.approx(r["theta"]) and ag.noise_type == "ou"
        assert bool(torch.isfinite(ag.losses).all())
        if r["hidden"] == (150, 300):
            for net, (i, o) in (("actor", (9, 2)), ("critic", (11, 1))):
                pad = D.pad_net_to(np.ones(D.net_size(i, o, r["hidden"]), f32), i, o, r["hidden"], HID) == 0
                assert pad.any()
                for k in (net, net + "_t", "m_" + net, "v_" + net, "grad_" + net):
                    assert not getattr(ag, k).cpu().numpy()[pad].any(), (l, k)
    env.close()

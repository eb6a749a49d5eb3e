"""GPU tests of population-based training for learner groups (shems_pbt_select_dev, shems_pbt_copy_dev, LearnerGroup.pbt_round,
run_episodes(pbt=...)): everything bit for bit against the NumPy twin (tests/pbt_ref.py) and against groups into which the twin's round
is written by hand through torch copies."""
import ctypes as C
import importlib

import numpy as np
import pytest

import pbt_cases as PC
import pbt_ref as PR
import util as U

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
L8, E, CAP = 8, 32, 2400
POP8 = [0, 0, 0, 0, 1, 1, 1, 1]
COPIED = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "w2t_actor", "w2t_critic", "s_min", "s_max")
COPIED_TD3 = ("critic2", "critic2_t", "m_critic2", "v_critic2", "w2t_critic2")


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    G = importlib.import_module(U.PKG_NAME + ".group")
    T = importlib.import_module(U.PKG_NAME + ".td3")
    return torch, S, G, T


def _params_struct(S, p):
    return S._capi.PbtParams(p["seed"], p["round"], p["permille"], p["fields"], 0, p["down"], p["up"], (C.c_double * 4)(*p["lo"]),
                             (C.c_double * 4)(*p["hi"]))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_select_equals_the_twin_on_every_case():
    torch, S, G, T = _mods()
    L = S._capi.declare_pbt()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    seen = 0
    for name, c in PC.select_cases():
        n = len(c["pop"])
        d_pop, d_score = _dev(torch, c["pop"]), _dev(torch, c["score"])
        d_hp = _dev(torch, np.frombuffer(c["hp"].tobytes(), np.uint8).copy())
        d_parent, d_rank = torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
        p = _params_struct(S, c["params"])
        S._capi.check(L.shems_pbt_select_dev(C.byref(p), n, ptr(d_pop), ptr(d_score), ptr(d_hp), ptr(d_parent), ptr(d_rank), None))
        torch.cuda.synchronize()
        w_hp, w_parent, w_rank = PR.round_twin(c["params"], c["pop"], c["score"], c["hp"])
        assert np.array_equal(d_rank.cpu().numpy(), w_rank) and np.array_equal(d_parent.cpu().numpy(), w_parent), name
        got = d_hp.cpu().numpy().tobytes()
        assert got == w_hp.tobytes(), name                                   # every byte of every record, the untouched learners' included
        kept = w_parent == np.arange(n)
        assert np.frombuffer(got, PR.REC)[kept].tobytes() == c["hp"][kept].tobytes(), name
        seen += 1
    assert seen == 64


def test_copy_on_fake_slabs_moves_the_ranges_and_nothing_else():
    torch, S, G, T = _mods()
    L = S._capi.declare_pbt()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    for name, c in PC.copy_cases():
        slab = PC.sentinel_slab(c["count"], c["stride"])
        d_slab, d_parent = _dev(torch, slab), _dev(torch, c["parent"])
        arr = (S._capi.PbtRange * len(c["ranges"]))(*[S._capi.PbtRange(o, k) for o, k in c["ranges"]])
        g = G.Group(c["count"], 0, 4 * c["stride"], 32)
        S._capi.check(L.shems_pbt_copy_dev(ptr(d_slab), C.byref(g), arr, len(c["ranges"]), ptr(d_parent), None))
        torch.cuda.synchronize()
        want = PR.copy_twin(slab, c["ranges"], c["parent"])
        assert d_slab.cpu().numpy().tobytes() == want.tobytes(), name
        assert want.tobytes() != slab.tobytes()
    # bad arguments: SHEMS_ERR_ARG by name, the slab untouched
    c = dict(PC.copy_cases())["fake-slab"]
    slab = PC.sentinel_slab(c["count"], c["stride"])
    d_slab, d_parent = _dev(torch, slab), _dev(torch, c["parent"])
    g = G.Group(c["count"], 0, 4 * c["stride"], 32)
    for ranges, n, word in PC.bad_copy_args():
        arr = (S._capi.PbtRange * len(ranges))(*[S._capi.PbtRange(o, k) for o, k in ranges])
        rc = L.shems_pbt_copy_dev(ptr(d_slab), C.byref(g), arr, len(ranges) if n is None else n, ptr(d_parent), None)
        msg = L.shems_last_error().decode()
        assert rc == S._capi.ERR_ARG and "shems_pbt_copy_dev" in msg and word in msg, (ranges, msg)
    torch.cuda.synchronize()
    assert d_slab.cpu().numpy().tobytes() == slab.tobytes()
    # a parent entry outside the group, or one that names a child, leaves its learner untouched
    d_parent = _dev(torch, np.array([0, 9, -1, 4, 0, 5, 6], np.int32))
    arr = (S._capi.PbtRange * 1)(S._capi.PbtRange(0, 516))
    S._capi.check(L.shems_pbt_copy_dev(ptr(d_slab), C.byref(g), arr, 1, ptr(d_parent), None))
    torch.cuda.synchronize()
    want = PR.copy_twin(slab, [(0, 516)], np.array([0, 1, 2, 3, 0, 5, 6], np.int32))     # only 4 <- 0 is a well-formed pair (3 <- 4: 4 is a child)
    assert d_slab.cpu().numpy().tobytes() == want.tobytes()


# ---- groups ---------------------------------------------------------------------------------------------------------------------------
HP8 = [{"batch": 32, "eta_act": 1e-4 * (1 + l), "eta_crit": 1e-3 + 1e-4 * l, "tau": 0.001 * (1 + l % 3), "sigma": 0.1 + 0.02 * l, "mu": 0.01 * (l % 2)}
       for l in range(L8)]
GROUPS = {
    "tiled": lambda G, T: G.LearnerGroup(L8, E, seed=21, rng_seed=77, capacity=CAP, tiled=True, hparams=HP8),
    "flux": lambda G, T: G.LearnerGroup(L8, E, seed=21, rng_seed=77, capacity=CAP, tiled=False, hparams=HP8),
    "td3": lambda G, T: T.TD3LearnerGroup(L8, E, seed=21, rng_seed=77, capacity=CAP, hparams=HP8),
    "per": lambda G, T: G.PrioritizedLearnerGroup(L8, E, seed=21, rng_seed=77, capacity=CAP, hparams=HP8),
    "nstep": lambda G, T: G.LearnerGroup(L8, E, seed=21, rng_seed=77, capacity=CAP, n_step=3,
                                         hparams=[dict(h, gamma=0.99 - 0.01 * l) for l, h in enumerate(HP8)]),
}
SCORES8 = np.array([-300.0, -700.0, -200.0, -300.0, np.nan, -450.0, -100.0, -np.inf])        # ties in population 0, non-finite in 1


def _make(name):
    torch, S, G, T = _mods()
    tab = S.tables.synthetic_table("train", 98)
    env = S.ShemsBatch(L8 * E, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    grp = GROUPS[name](G, T)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    for _ in range(3):                                                       # non-trivial moments, targets and tiles
        grp.replay()
    return env, grp


def _blocks(grp, names):
    return [(grp.layout[n][0], grp.layout[n][1]) for n in names if n in grp.layout and grp.layout[n][1] > 0]


def _records_of(grp):
    return np.frombuffer(grp._hp_dev.cpu().numpy().tobytes(), PR.REC).copy()


def _twin_round(grp, pbt, scores, rnd):
    p = pbt.params(rnd, grp.rng_seed)
    pd = PR.params(seed=p.seed, round=p.round, permille=p.permille, fields=p.fields, down=p.down, up=p.up, lo=tuple(p.lo), hi=tuple(p.hi))
    return PR.round_twin(pd, pbt.populations, np.asarray(scores, f64), _records_of(grp))


def _mirror(grp, G, new, parent):
    """The host mirrors a round refreshes, written by hand from the twin's records."""
    old = [dict(h) for h in grp.hparams]
    for l in np.flatnonzero(parent != np.arange(grp.count)):
        l, r = int(l), new[int(l)]
        h = dict(grp.hparams[l], gamma=old[int(parent[l])]["gamma"], eta_act=float(r["eta_act"]), eta_crit=float(r["eta_crit"]),
                 tau=float(r["tau"]), sigma=float(r["noise_sigma"]), mu=float(r["noise_mu"]), batch=int(r["batch"]))
        grp.hparams[l] = h
        ag = grp.learners[l]
        ag.gamma, ag.tau, ag.batch, ag.eta_act, ag.eta_crit, ag.sigma, ag.mu = h["gamma"], h["tau"], h["batch"], h["eta_act"], h["eta_crit"], h["sigma"], h["mu"]
    grp._hp_host = (G.HParams * grp.count).from_buffer_copy(new.tobytes())
    if grp._gamma1_dev is not None:
        grp._gamma1_dev.copy_(grp.torch.tensor([h["gamma"] for h in grp.hparams], dtype=grp.torch.float32))
    grp._hp_variants = {}


def _round_by_hand(grp, G, pbt, scores, rnd, names):
    """The twin's round written into a group through torch copies, block by block, and its records and mirrors by hand."""
    torch = grp.torch
    new, parent, rank = _twin_round(grp, pbt, scores, rnd)
    before = grp.slab.clone()
    for l in np.flatnonzero(parent != np.arange(grp.count)):
        for o, n in _blocks(grp, names):
            grp.slab[int(l), o:o + n] = before[int(parent[l]), o:o + n]
    grp._hp_dev.copy_(torch.from_numpy(np.frombuffer(new.tobytes(), np.uint8).copy()))
    _mirror(grp, G, new, parent)
    return new, parent, rank


def _mirrors_of(grp):
    return ([dict(h) for h in grp.hparams], [(ag.eta_act, ag.eta_crit, ag.tau, ag.sigma, ag.mu, ag.batch, ag.gamma, ag.gamma_n) for ag in grp.learners],
            bytes(grp._hp_host), None if grp._gamma1_dev is None else grp._gamma1_dev.cpu().numpy().tobytes(), dict(grp._hp_variants))


@pytest.mark.parametrize("name", list(GROUPS))
def test_pbt_round_on_a_group(name):
    torch, S, G, T = _mods()
    names = COPIED + (COPIED_TD3 if name == "td3" else ())
    env_a, ga = _make(name)
    env_b, gb = _make(name)
    gb.slab.copy_(ga.slab)                                                   # the same state, byte for byte
    pbt = G.PBT(POP8, truncation=0.5, seed=99)
    snap = ga.slab.clone()
    hp0 = _records_of(ga)
    flags = (ga._flux_valid, ga._tiled_valid)
    if name == "td3":
        ga._hold_ptr(), gb._hold_ptr()                                       # a record variant exists: the round must drop it
        assert ga._hp_variants
    parent = ga.pbt_round(SCORES8, pbt, 4)
    new, w_parent, w_rank = _round_by_hand(gb, G, pbt, SCORES8, 4, names)
    torch.cuda.synchronize()
    # ---- the round itself: parent, rank, records ----
    assert parent.dtype == np.int32 and np.array_equal(parent, w_parent) and np.array_equal(ga.pbt_rank.cpu().numpy(), w_rank)
    children = [int(l) for l in np.flatnonzero(parent != np.arange(L8))]
    assert all(POP8[parent[l]] == POP8[l] and np.isfinite(SCORES8[parent[l]]) for l in children)
    assert children == [1, 3, 4, 7]                                          # the two worst of each population, the NaN and the -inf among them
    assert _records_of(ga).tobytes() == new.tobytes() and new.tobytes() != hp0.tobytes()
    # ---- the slab: copied blocks are the parent's pre-round bytes, everything else is the snapshot ----
    after = ga.slab
    copied = torch.zeros(ga.slab_floats, dtype=torch.bool, device=ga.device)
    for o, n in _blocks(ga, names):
        copied[o:o + n] = True
    assert int(copied.sum()) > 8 * 125000
    if ga.tiled:
        assert all(ga.layout[k][1] == G.W2T_FLOATS for k in ("w2t_actor", "w2t_critic")) and float(snap[:, ga.layout["w2t_actor"][0]:][:, :G.W2T_FLOATS].abs().max()) > 0
    as_int = lambda x: x.view(torch.int32)
    for l in range(L8):
        src = int(parent[l])
        assert torch.equal(as_int(after[l])[copied], as_int(snap[src])[copied]), (name, l)
        assert torch.equal(as_int(after[l])[~copied], as_int(snap[l])[~copied]), (name, l)
    for l in children:                                                       # (the copy changed something: parent and child differed)
        assert not torch.equal(as_int(snap[l])[copied], as_int(snap[int(parent[l])])[copied])
    for blk in ("ring_s", "ring_a", "ring_r", "ring_s2", "ring_done", "ws", "grad_actor", "grad_critic", "losses", "per_prio", "per_pmax", "per_ws",
                "ns_stage_s", "ns_hist_s", "ns_hist_a", "ns_hist_r", "grad_critic2", "ws2", "losses2"):
        if blk in ga.layout:
            o, n = ga.layout[blk]
            assert not bool(copied[o:o + n].any()), blk
    assert (ga._flux_valid, ga._tiled_valid) == flags
    # ---- the host mirrors ----
    ma, mb = _mirrors_of(ga), _mirrors_of(gb)
    assert ma == mb and ma[4] == {}
    for l in children:
        p = int(parent[l])
        assert ga.hparams[l]["gamma"] == ga.hparams[p]["gamma"] and ga.learners[l].gamma_n == ga.learners[p].gamma_n
        assert ga.hparams[l]["hidden"] == ga.hparams[p]["hidden"] and ga.hparams[l]["batch"] == new[l]["batch"] == hp0[p]["batch"]
        assert float(f32(ga.hparams[l]["tau"])) == ga.hparams[l]["tau"] and ga.hparams[l]["eta_act"] == float(new[l]["eta_act"])
        assert float(new[l]["gamma"]) == float(hp0[p]["gamma"])              # the record holds the parent's gamma^n
    # ---- flux_(): the child has the parent's actor ----
    ga.flux_(), gb.flux_()
    oa, na = ga.layout["actor"]
    for l in children:
        assert torch.equal(as_int(ga.slab[l, oa:oa + na]), as_int(ga.slab[int(parent[l]), oa:oa + na]))
        assert torch.equal(ga.learners[l].s_min, ga.learners[int(parent[l])].s_min)
    # ---- one further update: each on its own ring and stream, and the bits of the group written by hand ----
    ga.replay(), gb.replay()
    ga.flux_(), gb.flux_()
    torch.cuda.synchronize()
    assert torch.equal(as_int(ga.slab), as_int(gb.slab)), name
    for l in children:
        assert not torch.equal(as_int(ga.slab[l, oa:oa + na]), as_int(ga.slab[int(parent[l]), oa:oa + na]))


def test_run_episodes_with_pbt_equals_the_hand_driven_group():
    """5 episodes, test_every = 2, start = 3: sweeps after episodes 1, 3 and 5, ONE round, after episode 3 (episode 1 is before `start`,
    episode 5 is the last).  Against the same group driven by hand with the twin's round applied through torch copies."""
    torch, S, G, T = _mods()
    NUM_EP, TEST_EVERY, TEST_RUNS = 5, 2, 32
    env_a, ga = _make("tiled")
    env_b, gb = _make("tiled")
    tabs = [S.tables.synthetic_table("eval", c) for c in (1, 98)]
    mk_eval = lambda: G.eval_batch(tabs, [POP8[l] for l in range(L8)], L8, test_runs=TEST_RUNS, maxsteps=1439, charger_ids=(1, 98))
    pbt = G.PBT(POP8, truncation=0.5, seed=5, start=3)
    rounds = []
    orig = ga.pbt_round
    ga.pbt_round = lambda scores, p, r: (rounds.append(r), orig(scores, p, r))[1]
    res = ga.run_episodes(env_a, mk_eval(), NUM_EP, test_every=TEST_EVERY, test_runs=TEST_RUNS, pbt=pbt)
    assert rounds == [1] and res.pbt_episodes == [3] and res.sweeps == 3      # no round at episode 1 nor at the last sweep
    # ---- by hand ----
    env_eval = mk_eval()
    scores, log = [], []
    for i in range(1, NUM_EP + 1):
        gb.episode_(env_b, train=True, rng_ep=gb.seed, episode=i)
        if i % TEST_EVERY != 1:
            continue
        sc = gb.eval_scores(env_eval, TEST_RUNS)
        scores.append(sc)
        if 3 <= i < NUM_EP:
            new, parent, _ = _round_by_hand(gb, G, pbt, sc, -(-i // TEST_EVERY) - 1, COPIED)
            log.append((parent, [dict(h) for h in gb.hparams], new))
    gb.flux_()
    torch.cuda.synchronize()
    assert np.array_equal(res.score_mean.view(np.uint64), np.stack(scores, 1).view(np.uint64))
    assert res.pbt_parent.shape == (L8, 1) and res.pbt_parent.dtype == np.int32 and np.array_equal(res.pbt_parent[:, 0], log[0][0])
    assert (log[0][0] != np.arange(L8)).sum() >= 2
    assert res.pbt_hparams == [log[0][1]] and ga.hparams == gb.hparams
    assert _records_of(ga).tobytes() == log[0][2].tobytes() == _records_of(gb).tobytes()
    assert torch.equal(ga.slab.view(torch.int32), gb.slab.view(torch.int32))
    none = gb.run_episodes(env_b, env_eval, 1, test_every=TEST_EVERY, test_runs=TEST_RUNS)      # without pbt: empty logs
    assert none.pbt_parent.shape == (L8, 0) and none.pbt_episodes == [] and none.pbt_hparams == []

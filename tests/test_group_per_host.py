"""Prioritized replay for learner groups without a GPU: the ctypes mirror of the new entry points against the header, the slab layout,
the constructor's refusals, anneal_beta, and -- on the NumPy twins alone -- what the rings and ticks of tests/group_per_cases.py must
hold for the cases tests/test_group_per_gpu.py runs on the device.

The ctypes, layout, refusal and anneal tests exercise the library and the package.  The twin tests check TEST INFRASTRUCTURE and touch
the package only through _feature(): the constants the cases rest on are the package's."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import group_per_cases as K
import per_ref as PR
import util as U

f32 = np.float32


def _G():
    return importlib.import_module(U.PKG_NAME + ".group")


def _D():
    return importlib.import_module(U.PKG_NAME + ".ddpg")


def _feature():
    """The package side of what the case file assumes: fails where the prioritized group does not exist."""
    G, S = _G(), U.pkg()
    assert issubclass(G.PrioritizedLearnerGroup, G.LearnerGroup) and not G.PrioritizedLearnerGroup.has_evaluate
    assert (G.PW_IDX, G.PW_W, G.PER_COLS) == (PR.PW_IDX, PR.PW_W, PR.COLS) and G.MAX_GROUP_BATCH == PR.COLS
    assert (S._capi.TP_STORE_GRAD, S._capi.TP_PER_GIVEN) == (1, 2)
    return G


_C_TO_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}


def test_group_per_prototypes_match_the_header(built_lib):
    """Every prototype of _capi._group_per_sigs against its declaration in include/shems_hip.h, argument by argument: scalars by width,
    `shems_per *` / `shems_replay *` by their mirrors, every other pointer as a pointer; the flag and the published rows by value."""
    S = U.pkg()
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    sigs = S._capi._group_per_sigs()
    assert set(sigs) == {"shems_ddpg_group_update_per_tp", "shems_per_group_sample_dev"}
    for name, args in sigs.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        decl = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(decl) == len(args), (name, decl)
        for d, a in zip(decl, args):
            if "*" in d:
                base = d.replace("const", "").split("*")[0].strip()
                want = {"shems_per": (C.POINTER(S._capi.PerArgs),), "shems_replay": (C.POINTER(S._capi.Replay),)}.get(base, (C.c_void_p,))
                assert a in want, (name, d, a)
            else:
                assert a is _C_TO_CTYPES[d.split()[0]], (name, d, a)
    # the argument ORDER the issue states for the update
    m = re.search(r"\bint\s+shems_ddpg_group_update_per_tp\s*\(([^;]*?)\)\s*;", hdr, re.S)
    names = [re.sub(r"[\s*]+", " ", a).split()[-1] for a in m.group(1).split(",")]
    assert names == ["d0", "ring0", "g", "t", "d_hp", "per0", "ring_len", "fresh_pos", "fresh_count", "seed", "tick", "eta_crit", "bp1_crit",
                     "bp2_crit", "eta_act", "bp1_act", "bp2_act", "flags", "stream"]
    assert re.search(r"SHEMS_TP_PER_GIVEN\s*=\s*2\b", hdr) and re.search(r"SHEMS_TP_STORE_GRAD\s*=\s*1\b", hdr)
    assert re.search(r"#define\s+SHEMS_TP_PER_PUB\s+165000\b", hdr)
    L = S._capi.declare_group_per()
    for name in sigs:
        assert getattr(L, name).restype is C.c_int and list(getattr(L, name).argtypes) == sigs[name]
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib]).decode()
    assert set(sigs) <= set(re.findall(r" T (shems_[a-z0-9_]+)", out)) and set(sigs) <= set(S._capi.exported_symbols())


# slab_floats of a DDPG LearnerGroup(2, 32, capacity=128, form="throughput"): the figures tests/test_group_td3_gpu.py asserts
PARENT_SLAB_FLOATS = {True: 4243932, False: 3195356}


@pytest.mark.parametrize("tiled", [True, False])
def test_slab_layout_keeps_the_ddpg_offsets_and_appends_the_three_blocks(tiled):
    G, D = _feature(), _D()
    nws = 1902568
    base, n_base = G.slab_layout(D.N_ACTOR, D.N_CRITIC, nws, 128, tiled)
    assert n_base == PARENT_SLAB_FLOATS[tiled] and list(base)[-1] == "ring_done"          # a plain group: unchanged
    for cap in (128, K.CAP, 24000):
        base, n_base = G.slab_layout(D.N_ACTOR, D.N_CRITIC, nws, cap, tiled)
        extra = G.per_extra_blocks(cap)
        assert [e[0] for e in extra] == ["per_prio", "per_pmax", "per_ws"]
        assert extra[0][1] == cap and extra[2][1] == PR.ws_floats(cap)
        lay, n = G.slab_layout(D.N_ACTOR, D.N_CRITIC, nws, cap, tiled, extra)
        assert list(lay)[:len(base)] == list(base) and all(lay[k] == base[k] for k in base)     # every DDPG offset unchanged
        end_ring = base["ring_done"][0] + base["ring_done"][1]
        spans = [(lay[k][0], lay[k][0] + lay[k][1], k) for k in ("per_prio", "per_pmax", "per_ws")]
        assert spans[0][0] >= end_ring and spans[0][0] == n_base                               # behind ring_done
        for (lo, hi, k), nxt in zip(spans, spans[1:] + [(n, n, "end")]):
            assert lo % 4 == 0 and hi <= nxt[0], (k, lo, hi, nxt)                               # 16-byte aligned, in order, disjoint
        assert n % 4 == 0
    with pytest.raises(ValueError):
        G.slab_layout(D.N_ACTOR, D.N_CRITIC, nws, 128, tiled, (("ring_s", 4),))


def test_constructor_refusals_come_before_any_device_work():
    """Every refusal names its reason; none of them needs a device (this test runs without one)."""
    G = _feature()
    T = importlib.import_module(U.PKG_NAME + ".td3")
    mk = lambda **kw: G.PrioritizedLearnerGroup(2, 32, **kw)
    for kw, exc, word in ((dict(form="latency"), NotImplementedError, "latency"), (dict(form="wide"), NotImplementedError, "wide"),
                          (dict(noise_type="ou"), NotImplementedError, "Ornstein-Uhlenbeck"),
                          (dict(hparams=[{"mem_size": 64}, {}]), NotImplementedError, "mem_size"),
                          (dict(hparams=[{}, {"batch": 129}]), NotImplementedError, "batch 129"),
                          (dict(hparams=[{"hidden": (300, 600)}, {}]), NotImplementedError, "hidden"),
                          (dict(hidden=(300, 600)), NotImplementedError, "hidden="),
                          (dict(capacity=262145), NotImplementedError, "capacity 262145"),
                          (dict(alpha=-0.1), ValueError, "alpha"), (dict(beta=1.5), ValueError, "beta"), (dict(eps=float("nan")), ValueError, "eps"),
                          (dict(beta=float("inf")), ValueError, "beta"), (dict(form="fast"), ValueError, "form")):
        with pytest.raises(exc) as ei:
            mk(**kw)
        assert word in str(ei.value), (kw, str(ei.value))

    class Both(G.PrioritizedLearnerGroup, T.TD3LearnerGroup):
        pass

    class Other(T.TD3LearnerGroup, G.PrioritizedLearnerGroup):
        pass

    for cls in (Both, Other):
        with pytest.raises(NotImplementedError, match="TD3LearnerGroup"):
            cls(2, 32)
    G.per_group_refusals(hparams=K.RECORD_CASE)              # the records of the GPU case are ones a prioritized group takes


def test_anneal_beta_reaches_one_in_the_last_episode():
    """run_episodes' rule: beta of episode i is anneal_beta(beta0, i - 1, num_ep - 1)."""
    D = _D()
    for beta0 in (0.0, 0.4, 1.0):
        for num_ep in (1, 2, 3, 400):
            b = [D.anneal_beta(beta0, i - 1, max(1, num_ep - 1)) for i in range(1, num_ep + 1)]
            assert b[0] == beta0 and (num_ep == 1 or b[-1] == 1.0) and all(x <= y for x, y in zip(b, b[1:])) and max(b) <= 1.0
    assert D.anneal_beta(0.4, 399, 399) == 1.0 and D.anneal_beta(0.4, 1000, 399) == 1.0
    with pytest.raises(ValueError):
        D.anneal_beta(1.5, 0, 1)
    import inspect
    G = _feature()
    sig = inspect.signature(G.PrioritizedLearnerGroup.run_episodes)
    assert sig.parameters["anneal_beta_from"].default is None
    assert list(inspect.signature(G.PrioritizedLearnerGroup.__init__).parameters)[3:6] == ["alpha", "beta", "eps"]


# ------------------------------------------------------------------------------------------ the twin on the GPU cases' rings --
def test_the_rings_hold_what_the_gpu_cases_are_there_for():
    _feature()
    assert PR.n_blocks(K.CAP) == 4 and K.CAP % PR.BLOCK != 0                                 # four blocks, the last one partial
    for l in (1, 2, 47):
        p = K.priorities(l)
        assert p.min() > 0 and p.max() / p.min() >= 1e4, l                                   # four decades
    p0 = K.priorities(K.DUP_LEARNER)
    assert (p0 == f32(60.0)).sum() == 5 and not np.array_equal(p0, K.priorities(1))
    # different learners draw different columns from the same tick (key seed + l)
    u = [PR.uniforms(K.RNG_SEED + l, K.TICKS[0]) for l in range(3)]
    assert not (u[0] == u[1]).any() and not (u[1] == u[2]).any()
    assert np.array_equal(u[1], PR.uniforms(K.RNG_SEED + 1, K.TICKS[0]))


@pytest.mark.parametrize("L,batch", K.STAGE_CASES)
def test_the_gpu_cases_meet_their_duplicate_and_tie_conditions_on_the_twin(L, batch):
    _feature()
    assert K.DUP_LEARNER in K.checked(L)
    for l in K.checked(L):
        for tick in K.ticks_of((L, batch))[:1]:              # the first update starts from the initial state: it can be looked at here
            tu = K.twin_update(l, tick, batch)
            live = tu["idx"][:batch]
            assert (live >= 0).all() and (live < K.CAP).all() and (tu["idx"][batch:] == -1).all()
            assert tu["w"][:batch].max() == 1 and (tu["w"][:batch] > 0).all() and not tu["w"][batch:].any()
            assert batch == 1 or tu["w"][:batch].min() < 0.9
            shared, single = K.duplicates(live)
            if l == K.DUP_LEARNER and batch >= 120:
                assert len(shared) >= 3 and len(single) >= 20, (len(shared), len(single))
                # the writer of a shared slot is the HIGHEST column that drew it, and its value differs from a lower column's
                pn = PR.new_priority(tu["diff"], K.EPS_P, K.ALPHA)
                for slot in shared:
                    cols = np.nonzero(live == slot)[0]
                    assert tu["writer"][int(slot)] == cols.max() and tu["prio"][slot] == pn[cols.max()]
            # undrawn slots keep their priorities, pmax is only raised
            keep = np.ones(K.CAP, bool)
            keep[live] = False
            assert np.array_equal(tu["prio"][keep], K.priorities(l)[keep]) and tu["pmax"] >= 1.0
            assert K.initial_ties(l, tick, batch) == [], (l, tick, batch)
    assert K.EXPECTED_TIES[(L, batch)] == []


def test_the_record_case_draws_each_learners_own_batch():
    _feature()
    for l, rec in enumerate(K.RECORD_CASE):
        b = rec["batch"]
        tu = K.twin_update(l, K.TICKS[0], b)
        assert (tu["idx"][:b] >= 0).all() and (tu["idx"][b:] == -1).all() and tu["w"][:b].max() == 1
        # t_m = (m + u_m) (T / batch_l): another batch, other targets from the same uniforms
        other, _ = K.draw(l, K.TICKS[0], 128 - b)
        mine, _ = K.draw(l, K.TICKS[0], b)
        assert np.array_equal(other["u"], mine["u"]) and not np.array_equal(other["t"], mine["t"])
        assert K.initial_ties(l, K.TICKS[0], b) == []


def test_the_twin_is_per_ref_with_the_groups_key():
    """The twin of a prioritized group, composed on the CPU: learner l's draw is per_ref.sample with key RNG_SEED + l, its update
    per_ref.PerLearner.replay_w on the drawn columns; with unit weights that is the oracle's replay() on those columns."""
    import ddpg_oracle as DO
    _feature()
    l, tick, b = 1, K.TICKS[0], 17
    tw, p = K.draw(l, tick, b)
    ref = PR.sample(np.array(K.priorities(l)), 1.0, K.CAP, K.CAP, 0, 0, K.RNG_SEED + l, tick, b, K.BETA)
    for k in ("S", "C", "u", "t", "idx", "w"):
        assert np.array_equal(tw[k], ref[k]), k
    s, a, r, s2, done = K.minibatch(l, tw["slots"][:b])
    P, Q = K.per_learner(l), K.per_learner(l)
    ones = np.ones(b, f32)
    lc, la, diff = P.replay_w(s, a, r, s2, done, ones)
    lc0, la0 = DO.Learner.replay(Q, s, a, r, s2, done)
    assert np.array_equal(P.critic, Q.critic) and np.array_equal(P.actor, Q.actor) and abs(lc - lc0) < 1e-6 * max(1, abs(lc0))
    assert np.array_equal(K.target_y(K.per_learner(l), r, s2, done), K.per_learner(l).targets(r, s2, done))
    # the sampler edge cases of per_cases that fit the group's slabs are all there
    names = [n for n, _ in K.sampler_edge_cases()]
    assert len(names) == 31 and "beta0" in names and "fresh-wrap" in names and "zeros-1000" in names and all("24000" not in n for n in names)


def test_group_refusals_word_for_word_and_in_order():
    """The walk a prioritized group shares with a TD3 group (tests/util.py holds the rows), then its own numbers."""
    G = _feature()
    rows = U.group_variant_refusal_rows("prioritized learner group", "prioritized update", "weighted head", "shems_ddpg_group_update_per_tp",
                         " (the rings advance in lockstep)", "the sampler draws at most 128 columns")
    cap = "prioritized learner group: capacity 262145 > 262144: a learner's sampler workgroup keeps every block sum in LDS"
    own = [(dict(capacity=262145), NotImplementedError, cap), (dict(alpha=-0.1), ValueError, "prioritized learner group: alpha = -0.1 must be finite and >= 0"),
           (dict(beta=1.5), ValueError, "prioritized learner group: beta = 1.5 must be in [0, 1]"),
           (dict(hparams=[{"hidden": (300, 600)}], capacity=262145), NotImplementedError, rows[7][2]),           # the walk before the own numbers
           (dict(capacity=262145, alpha=-0.1), NotImplementedError, cap),
           (dict(alpha=-0.1, beta=1.5), ValueError, "prioritized learner group: alpha = -0.1 must be finite and >= 0")]
    for kw, exc, message in rows + own:
        with pytest.raises(exc) as ei:
            G.per_group_refusals(**kw)
        assert str(ei.value) == message, kw
    assert G.per_group_refusals() is None and G.per_group_refusals(form="throughput", hparams=[{"batch": 128, "hidden": (250, 500)}]) is None

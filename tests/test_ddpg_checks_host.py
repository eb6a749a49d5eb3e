"""The argument checks of the single-learner update and of the latency form of learner groups (csrc/shems_ddpg.hip), without a GPU: one
table of faults, applied to every entry point that takes the faulty argument.  Each call carries exactly one fault and is refused with
SHEMS_ERR_ARG and the exact message before the first HIP call -- host memory stands in for the device buffers, which are never
dereferenced on these paths, and on a machine without a device any HIP call in front of a check would turn the refusal into
SHEMS_ERR_NODEVICE ("hipGetDevice: no ROCm-capable device is detected").  The messages are written out here, as callers match on them: the critic side names shems_ddpg_critic_grad (its exclusion
window shems_ddpg_critic_grad_ex), the actor side shems_ddpg_actor_grad, the sweeps' beta powers `adam`, whichever entry point was called.
SHEMS_ERR_STATE (a learner on the tiled layout) needs a learner that has entered, i.e. a launch: tests/test_agent_tiled_gpu.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import util as U

(UPDATE, CRITIC_UPDATE, CLONE, GIVEN, PER, TD3, CGRAD, CGRAD_EX, GCGRAD, GUPDATE, AGRAD, GAGRAD, PREPARE, CAPPLY, AAPPLY, AAPPLY_PUB, GCAPPLY,
 GAAPPLY, BATCH_OBS, TILED_ENTER) = ENTRY = (
    "shems_ddpg_update", "shems_ddpg_critic_update", "shems_ddpg_clone_update", "shems_ddpg_update_given", "shems_ddpg_update_per",
    "shems_td3_update", "shems_ddpg_critic_grad", "shems_ddpg_critic_grad_ex", "shems_ddpg_group_critic_grad", "shems_ddpg_group_update",
    "shems_ddpg_actor_grad", "shems_ddpg_group_actor_grad", "shems_ddpg_actor_prepare", "shems_ddpg_critic_apply", "shems_ddpg_actor_apply",
    "shems_ddpg_actor_apply_pub", "shems_ddpg_group_critic_apply", "shems_ddpg_group_actor_apply", "shems_ddpg_batch_obs_dev",
    "shems_ddpg_tiled_enter")
CRITIC_SIDE = (UPDATE, CRITIC_UPDATE, CGRAD, CGRAD_EX, GCGRAD, GUPDATE)           # K1..K3 through the shared check: it names critic_grad
RING = CRITIC_SIDE + (CLONE, GIVEN, PER, TD3)                                      # take a ring and a ring length
CRITIC_BP = (UPDATE, CRITIC_UPDATE, GIVEN, PER, TD3, GUPDATE, CAPPLY, GCAPPLY)     # take the critic's beta powers
ACTOR_BP = (UPDATE, CLONE, GIVEN, PER, TD3, GUPDATE, AAPPLY, AAPPLY_PUB, GAAPPLY)  # ... the actor's
GROUP = (GCGRAD, GUPDATE, GAGRAD, GCAPPLY, GAAPPLY)
APPLY = (CAPPLY, AAPPLY, AAPPLY_PUB, GCAPPLY, GAAPPLY)
CG, AG = "shems_ddpg_critic_grad", "shems_ddpg_actor_grad"
D_NAME = {**dict.fromkeys(CRITIC_SIDE, CG), AGRAD: AG, GAGRAD: AG, AAPPLY_PUB: AAPPLY}   # who the shems_ddpg refusals name; else the entry point
BLK, WS, W2T, CAP, NCRIT = 131072, 1902568, 524288, 16, 129001   # floats: a parameter block, the workspace, a tiled region; ring slots; a critic
NAN, INF = float("nan"), float("inf")
D_BUFFERS = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic", "s_min", "s_max",
             "ws", "losses")
C2_BUFFERS = ("critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2", "ws2", "losses2")


class Blocks:
    """128-byte aligned host blocks of the sizes the entry points assume, carved from one array (the TD3 entry point compares addresses:
    its blocks must not overlap).  pair: room for two critic-sized buffers that touch."""
    def __init__(self):
        sizes = dict.fromkeys(D_BUFFERS[:10] + C2_BUFFERS[:5], BLK)
        sizes.update(dict.fromkeys(("s_min", "s_max", "losses", "losses2", "prio", "pmax", "idx", "w", "obs"), 1152))
        sizes.update(ws=WS, ws2=WS, ta=W2T, tc=W2T, per_ws=544, pair=2 * BLK, s=CAP * 9, a=CAP * 2, r=CAP, s2=CAP * 9, done=CAP)
        self.raw = np.zeros(sum(-(-n // 32) * 32 for n in sizes.values()) + 32, np.float32)
        at = self.raw.ctypes.data + (-self.raw.ctypes.data) % 128
        for name, n in sizes.items():
            assert at % 128 == 0
            setattr(self, name, at)
            at += 4 * (-(-n // 32) * 32)


@pytest.fixture(scope="module")
def env(built_lib):
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    D, G, T = mod("ddpg"), mod("group"), mod("td3")
    L = T._declare()
    assert G._declare_group() is L and S._capi.declare_per() is L
    return S, D, G, T, L, Blocks()


def _table(S, D, G, B):
    """(what, arguments that differ from a valid call, the refusal with {d} / {fn} for the names, entry points the row is for)."""
    def ddpg(batch=120, **other):
        d = D.DdpgArgs(*(getattr(B, n) for n in D_BUFFERS), 0.99, 1.0, batch, 0)
        for k, v in other.items():
            setattr(d, k, v)
        return d

    def ring(capacity=CAP, without=()):
        return S._capi.Replay(capacity, *(getattr(B, k) if k not in without else None for k in ("s", "a", "r", "s2", "done")))

    grp = lambda count, stride: G.Group(count, 0, stride, 32)
    null, batch, align = "{d}: shems_ddpg has a NULL buffer", "{d}: batch must be in 1..128 (got %d)", "{d}: parameter blocks must be 16-byte aligned"
    bad_ring, window = "{r}: bad replay ring / length", "shems_ddpg_critic_grad_ex: an exclusion window needs a full ring and 0 <= count < capacity"
    beta, group = "{b}: beta powers must be in (0,1)", "{fn}: shems_group needs 1 <= count <= 65535 and a 16-byte-multiple stride"
    given = "{fn}: d_idx and d_w must be device arrays of 128 elements"
    c2_null, c2_16, c2_4 = ("{fn}: shems_td3 has a NULL critic-2 buffer", "{fn}: critic-2 parameter blocks and ws2 must be 16-byte aligned",
                            "{fn}: critic-2 buffers must be float aligned")
    trg, enter = "{fn}: sigma_trg and clip_trg must be finite and >= 0", "{fn}: shems_group_w2t needs two 128-byte aligned device regions"
    every = tuple(e for e in ENTRY if e != TD3)                     # (the TD3 entry point takes a shems_td3, which holds the shems_ddpg)
    rows = [("shems_ddpg NULL", dict(d=None), null, every), ("shems_td3 NULL", dict(d=None), "{fn}: NULL", (TD3,))]
    rows += [(n + " NULL", dict(d=ddpg(**{n: None})), null, ENTRY) for n in D_BUFFERS]
    rows += [("batch %d" % b, dict(d=ddpg(batch=b)), batch % b, ENTRY) for b in (0, 129)]
    rows += [(n + " + %d" % o, dict(d=ddpg(**{n: getattr(B, n) + o})), align, ENTRY) for n, o in (("actor", 8), ("critic", 4), ("actor_t", 12), ("critic_t", 8))]
    rows += [("ring NULL", dict(ring=None), bad_ring, RING)]
    rows += [("ring without " + k, dict(ring=ring(without=(k,))), bad_ring, RING) for k in ("s", "a", "r", "s2", "done")]
    rows += [("ring_len 0", dict(ring_len=0), bad_ring, RING), ("ring_len capacity + 1", dict(ring_len=CAP + 1), bad_ring, RING)]
    rows += [("ring NULL", dict(ring=None), "{fn}: bad arguments", (BATCH_OBS,)), ("ring without s", dict(ring=ring(without=("s",))), "{fn}: bad arguments", (BATCH_OBS,)),
             ("d_obs NULL", dict(obs=None), "{fn}: bad arguments", (BATCH_OBS,))]
    rows += [("window count -1", dict(excl=(0, -1)), window, (UPDATE, CGRAD_EX)), ("window pos -1", dict(excl=(-1, 0)), window, (UPDATE, CGRAD_EX)),
             ("window on a ring not full", dict(excl=(0, 4), ring_len=CAP - 1), window, (UPDATE, CGRAD_EX)),
             ("window of the whole ring", dict(excl=(0, CAP)), window, (UPDATE, CGRAD_EX))]
    rows += [(f"critic beta power {i + 1} = {v}", dict(bp={i: v}), beta, CRITIC_BP) for i in (0, 1) for v in (0.0, 1.0, NAN)]
    rows += [(f"actor beta power {i - 1} = {v}", dict(bp={i: v}), beta, ACTOR_BP) for i in (2, 3) for v in (0.0, 1.0, NAN)]
    rows += [("group NULL", dict(g=None), group, GROUP), ("count 0", dict(g=grp(0, 4096)), group, GROUP), ("count 65536", dict(g=grp(65536, 4096)), group, GROUP),
             ("stride 4100", dict(g=grp(2, 4100)), group, GROUP), ("stride -4096", dict(g=grp(2, -4096)), group, GROUP),
             ("stride 0, count 2", dict(g=grp(2, 0)), group, GROUP)]
    rows += [("d_idx NULL", dict(idx=None), given, (GIVEN,)), ("d_w NULL", dict(w=None), given, (GIVEN,)),
             ("d_idx + 2", dict(idx=B.idx + 2), given, (GIVEN,)), ("d_w + 2", dict(w=B.w + 2), given, (GIVEN,))]
    rows += [("update_policy 2", dict(policy=2), "{fn}: update_policy must be 0 or 1 (got 2)", (TD3,))]
    rows += [(f"{k} = {v}", dict(td3={k: v}), trg, (TD3,)) for k in ("sigma_trg", "clip_trg") for v in (-0.5, NAN, INF)]
    rows += [(n + " NULL", dict(td3={n: None}), c2_null, (TD3,)) for n in C2_BUFFERS]
    rows += [(n + " + %d" % o, dict(td3={n: getattr(B, n) + o}), c2_16, (TD3,)) for n, o in (("critic2", 8), ("critic2_t", 4), ("ws2", 4))]
    rows += [(n + " + 2", dict(td3={n: getattr(B, n) + 2}), c2_4, (TD3,)) for n in ("m_critic2", "v_critic2", "grad_critic2", "losses2")]
    # the overlap test, one row per pair class and both ends of a range; a pair that touches is not refused by it: the call goes on to the
    # next check, here the batch
    one, two = "{fn}: a critic-2 buffer overlaps one of critic 1's", "{fn}: two critic-2 buffers overlap"
    rows += [("critic2 inside critic", dict(td3=dict(critic2=B.critic + 4000)), one, (TD3,)),
             ("m_critic2 ends inside grad_critic", dict(td3=dict(m_critic2=B.grad_critic - 4 * NCRIT + 4)), one, (TD3,)),
             ("v_critic2 begins on the last float of critic_t", dict(td3=dict(v_critic2=B.critic_t + 4 * NCRIT - 4)), one, (TD3,)),
             ("critic2_t inside critic2", dict(td3=dict(critic2_t=B.critic2 + 4096)), two, (TD3,)),
             ("grad_critic2 = v_critic2", dict(td3=dict(grad_critic2=B.v_critic2)), two, (TD3,)),
             ("ws2 inside ws", dict(td3=dict(ws2=B.ws + 64)), "{fn}: ws2 overlaps ws", (TD3,)),
             ("ws2 ends inside ws", dict(td3=dict(ws2=B.ws - 64)), "{fn}: ws2 overlaps ws", (TD3,)),
             ("losses2 = losses + 1", dict(td3=dict(losses2=B.losses + 4)), "{fn}: losses2 overlaps losses", (TD3,)),
             ("m_critic2 touches m_critic, batch 0", dict(d=ddpg(batch=0, m_critic=B.pair), td3=dict(m_critic2=B.pair + 4 * NCRIT)), batch % 0, (TD3,)),
             ("m_critic touches m_critic2, batch 0", dict(d=ddpg(batch=0, m_critic=B.pair + 4 * NCRIT), td3=dict(m_critic2=B.pair)), batch % 0, (TD3,)),
             ("losses2 = losses + 2, batch 0", dict(d=ddpg(batch=0), td3=dict(losses2=B.losses + 8)), batch % 0, (TD3,))]
    rows += [("w2t NULL", dict(t=None), enter, (TILED_ENTER,)), ("w2t without actor", dict(t=D.W2T(None, B.tc)), enter, (TILED_ENTER,)),
             ("w2t without critic", dict(t=D.W2T(B.ta, None)), enter, (TILED_ENTER,)), ("w2t actor + 64", dict(t=D.W2T(B.ta + 64, B.tc)), enter, (TILED_ENTER,)),
             ("w2t critic + 64", dict(t=D.W2T(B.ta, B.tc + 64)), enter, (TILED_ENTER,))]
    valid = dict(d=ddpg(), ring=ring(), ring_len=CAP, excl=(0, 0), bp={}, g=grp(2, 4096), idx=B.idx, w=B.w, policy=1, td3={}, t=D.W2T(B.ta, B.tc),
                 obs=B.obs)
    return rows, valid


def _call(env, name, a):
    S, D, G, T, L, B = env
    by = lambda x: C.byref(x) if x is not None else None
    bp = [a["bp"].get(i, v) for i, v in enumerate((0.9, 0.999, 0.9, 0.999))]
    d, r, g, n, fn = by(a["d"]), by(a["ring"]), by(a["g"]), a["ring_len"], getattr(L, name)
    crit, act, sample = (1e-4, bp[0], bp[1]), (1e-4, bp[2], bp[3]), (7, 0)
    if name == UPDATE:
        rc = fn(d, r, n, *sample, *a["excl"], *crit, *act, None, None)
    elif name == CRITIC_UPDATE:
        rc = fn(d, r, n, *sample, *crit, None)
    elif name == CLONE:
        rc = fn(d, r, n, *sample, *act, None, None)
    elif name == GIVEN:
        rc = fn(d, r, n, a["idx"], a["w"], *crit, *act, None)
    elif name == PER:
        rc = fn(d, r, by(S._capi.PerArgs(B.prio, B.pmax, B.per_ws, 0.6, 0.4, 1e-3, 0)), n, 0, 0, *sample, *crit, *act, None)
    elif name == TD3:
        c2 = {**{k: getattr(B, k) for k in C2_BUFFERS}, "sigma_trg": 0.2, "clip_trg": 0.5, **a["td3"]}
        t3 = None if a["d"] is None else T.Td3Args(a["d"], *(c2[k] for k in C2_BUFFERS), c2["sigma_trg"], c2["clip_trg"])
        rc = fn(by(t3), r, n, *sample, *crit, *act, a["policy"], None)
    elif name == CGRAD:
        rc = fn(d, r, n, *sample, None)
    elif name == CGRAD_EX:
        rc = fn(d, r, n, *sample, *a["excl"], None)
    elif name == GCGRAD:
        rc = fn(d, r, g, n, *sample, None)
    elif name == GUPDATE:
        rc = fn(d, r, g, n, *sample, *crit, *act, None)
    elif name in (AGRAD, PREPARE):
        rc = fn(d, None)
    elif name == GAGRAD:
        rc = fn(d, g, None)
    elif name in (CAPPLY, AAPPLY):
        rc = fn(d, *(crit if name == CAPPLY else act), 1.0, None)
    elif name == AAPPLY_PUB:
        rc = fn(d, *act, 1.0, None, None)
    elif name in (GCAPPLY, GAAPPLY):
        rc = fn(d, g, *(crit if name == GCAPPLY else act), None)
    elif name == BATCH_OBS:
        rc = fn(d, r, a["obs"], None)
    else:
        rc = fn(d, by(a["t"]), None)
    return rc, L.shems_last_error().decode()


def _expected(name, text):
    return text.format(fn=name, d=D_NAME.get(name, name), r=CG if name in CRITIC_SIDE else name, b="adam" if name in APPLY else name)


@pytest.mark.parametrize("name", ENTRY)
def test_every_entry_point_refuses_each_fault_with_its_message_before_any_hip_call(env, name):
    S, D, G, T, L, B = env
    rows, valid = _table(S, D, G, B)
    mine = [row for row in rows if name in row[3]]
    assert mine
    for what, kw, text, _ in mine:
        rc, msg = _call(env, name, {**valid, **kw})
        assert (rc, msg) == (S._capi.ERR_ARG, _expected(name, text)), (name, what, rc, msg)
    assert not B.raw.any()


def test_the_td3_overlap_test_is_ranges_overlap():
    """The truth table of the buffer checks of shems_td3_update, on element addresses as the entry point once wrote it (two < one + n and
    one < two + n) and on byte ranges as ranges_overlap of csrc/shems_internal.h has it: equal for every placement of a second buffer
    around a first one, for equal sizes (the critic blocks) and for unequal ones (ws2 against ws, losses2 against losses)."""
    def by_elements(two, n2, one, n1):
        return two < one + n1 and one < two + n2

    def ranges_overlap(a, na, b, nb):
        return a < b + nb and b < a + na

    for n1, n2 in ((5, 5), (2, 1), (7, 3), (3, 7)):
        for one in (16, 17):
            for two in range(one - n2 - 2, one + n1 + 3):
                want = any(two <= e < two + n2 for e in range(one, one + n1))
                assert by_elements(two, n2, one, n1) == ranges_overlap(4 * two, 4 * n2, 4 * one, 4 * n1) == want, (n1, n2, one, two)

"""The argument checks that the six throughput entry points of the grouped update share, without a GPU: one table of faults, applied to
every entry point.  Each call carries exactly one fault and is refused with SHEMS_ERR_ARG before the first HIP call -- host memory stands
in for the device buffers, which are never dereferenced on these paths.  The faults of one entry point alone (update_policy, sigma_trg,
d_hp_hold, critic-2 overlaps, d_xp, the fresh range, the slab) are held by test_c_abi_refusals_launch_nothing of the TD3 and
prioritized GPU tests, and the ring stride of the half updates by tests/test_group_imitation_host.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import util as U

TP, TP_X, CLONE, CRITIC, TD3, PER = ("shems_ddpg_group_update_tp", "shems_ddpg_group_update_tp_x", "shems_ddpg_group_clone_update_tp",
                                     "shems_ddpg_group_critic_update_tp", "shems_td3_group_update_tp", "shems_ddpg_group_update_per_tp")
ENTRY = (TP, TP_X, CLONE, CRITIC, TD3, PER)
BLK, WS, W2T, CAP = 131072, 1902568, 524288, 16      # floats: a parameter block (>= 129 002), the workspace, a tiled region; ring slots
NAN = float("nan")


class Blocks:
    """16-byte aligned host blocks of the sizes the entry points assume, carved from one array (the TD3 entry point compares addresses:
    its blocks must not overlap)."""
    def __init__(self):
        sizes = dict.fromkeys(("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic",
                               "critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2"), BLK)
        sizes.update(dict.fromkeys(("s_min", "s_max", "losses", "losses2", "hp", "xp", "pushed", "prio", "pmax"), 32))
        sizes.update(ws=WS, ws2=WS, ta=W2T, tc=W2T, tc2=W2T, per_ws=528, s=CAP * 9, a=CAP * 2, r=CAP, s2=CAP * 9, done=CAP)
        self.raw = np.zeros(sum(sizes.values()) + 4, np.float32)
        at = self.raw.ctypes.data + (-self.raw.ctypes.data) % 16
        for name, n in sizes.items():
            assert n % 4 == 0 and at % 16 == 0
            setattr(self, name, at)
            at += 4 * n


@pytest.fixture(scope="module")
def env(built_lib):
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    D, G, T = mod("ddpg"), mod("group"), mod("td3")
    L = T._declare_group()
    assert S._capi.declare_group_per() is L
    return S, D, G, T, L, Blocks()


def _table(D, G, B):
    """(what, arguments that differ from a valid call, word of the refusal, entry points the row is not for)."""
    def ddpg(batch=120, **other):
        d = D.DdpgArgs(*(getattr(B, n) for n, _ in D.DdpgArgs._fields_[:14]), 0.99, 1.0, batch, 0)
        for k, v in other.items():
            setattr(d, k, v)
        return d

    def ring(capacity=CAP, without=()):
        return U.pkg()._capi.Replay(capacity, *(getattr(B, k) if k not in without else None for k in ("s", "a", "r", "s2", "done")))

    grp = lambda count, stride: G.Group(count, 0, stride, 32)
    rows = [("group NULL", dict(g=None), "shems_group", ()), ("count 0", dict(g=grp(0, 4096)), "shems_group", ()),
            ("count 65536", dict(g=grp(65536, 4096)), "shems_group", ()), ("stride 4100", dict(g=grp(2, 4100)), "shems_group", ()),
            ("stride 0, count 2", dict(g=grp(2, 0)), "shems_group", ()),
            ("shems_ddpg NULL", dict(d=None), "NULL", ())]          # (the TD3 entry point takes a shems_td3, which holds the shems_ddpg)
    rows += [(n + " NULL", dict(d=ddpg(**{n: None})), "NULL buffer", ()) for n in ("actor", "actor_t", "s_min", "s_max", "ws", "losses")]
    rows += [(n + " NULL", dict(d=ddpg(**{n: None})), "NULL buffer", (CRITIC,)) for n in ("m_actor", "v_actor")]      # no actor step
    rows += [(n + " NULL", dict(d=ddpg(**{n: None})), "NULL buffer", (CLONE,)) for n in ("critic", "critic_t", "m_critic", "v_critic")]   # no critic
    rows += [("STORE_GRAD, no grad_actor", dict(d=ddpg(grad_actor=None), flags=1), "STORE_GRAD", (CRITIC,)),
             ("STORE_GRAD, no grad_critic", dict(d=ddpg(grad_critic=None), flags=1), "STORE_GRAD", (CLONE,)),
             ("flag bit 8", dict(flags=8), "unknown flag", ()),
             ("batch 0", dict(d=ddpg(batch=0)), "batch", (TP_X,)), ("batch 129", dict(d=ddpg(batch=129)), "batch", (TP_X,)),    # _x: always records
             ("d_hp + 4", dict(hp=C.c_void_p(B.hp + 4)), "d_hp", ()),
             ("actor + 8", dict(d=ddpg(actor=B.actor + 8)), "16-byte aligned", ()), ("actor_t + 4", dict(d=ddpg(actor_t=B.actor_t + 4)), "16-byte aligned", ()),
             ("ws + 4", dict(d=ddpg(ws=B.ws + 4)), "16-byte aligned", ()),
             ("critic + 8", dict(d=ddpg(critic=B.critic + 8)), "16-byte aligned", (CLONE,)),
             ("critic_t + 4", dict(d=ddpg(critic_t=B.critic_t + 4)), "16-byte aligned", (CLONE,)),
             ("ring NULL", dict(ring=None), "ring", ())]
    rows += [("ring without " + k, dict(ring=ring(without=(k,))), "ring", ()) for k in ("s", "a")]
    rows += [("ring without " + k, dict(ring=ring(without=(k,))), "ring", (CLONE,)) for k in ("r", "s2", "done")]      # demonstrations: s and a
    rows += [("ring_len 0", dict(ring_len=0), "length", (TP_X,)), ("ring_len capacity + 1", dict(ring_len=CAP + 1), "length", (TP_X,))]   # _x: device lengths
    rows += [(f"critic beta power {i + 1} = {v}", dict(bp={i: v}), "beta powers", (CLONE,)) for i, v in ((0, 0.0), (1, 1.0), (0, NAN))]
    rows += [(f"actor beta power {i - 1} = {v}", dict(bp={i: v}), "beta powers", (CRITIC,)) for i, v in ((2, 0.0), (3, 1.0), (3, NAN))]
    rows += [("w2t without critic", dict(t=G.GroupW2T(B.ta, None)), "both regions", ()), ("w2t without actor", dict(t=G.GroupW2T(None, B.tc)), "both regions", ()),
             ("w2t actor + 4", dict(t=G.GroupW2T(B.ta + 4, B.tc)), "16-byte aligned", ()), ("w2t critic + 8", dict(t=G.GroupW2T(B.ta, B.tc + 8)), "16-byte aligned", ())]
    return rows, dict(d=ddpg(), ring=ring(), g=grp(2, 4096), t=None, hp=None, ring_len=CAP, flags=0, bp={})


def _call(env, name, a):
    S, D, G, T, L, B = env
    by = lambda x: C.byref(x) if x is not None else None
    bp = [a["bp"].get(i, v) for i, v in enumerate((0.9, 0.999, 0.9, 0.999))]
    d, r, g, t, hp = by(a["d"]), by(a["ring"]), by(a["g"]), by(a["t"]), a["hp"]
    fn = getattr(L, name)
    if name == TP:
        rc = fn(d, r, g, t, hp, a["ring_len"], 7, 0, 1e-4, bp[0], bp[1], 1e-4, bp[2], bp[3], a["flags"], None)
    elif name == TP_X:
        rc = fn(d, r, g, t, hp or C.c_void_p(B.hp), B.xp, B.pushed, 7, 0, 1e-4, bp[0], bp[1], 1e-4, bp[2], bp[3], a["flags"], None)
    elif name in (CLONE, CRITIC):
        rc = fn(d, r, 64, g, t, hp, a["ring_len"], 7, 0, 1e-4, *(bp[2:] if name == CLONE else bp[:2]), a["flags"], None)
    elif name == TD3:
        t3 = None if a["d"] is None else T.Td3Args(a["d"], B.critic2, B.critic2_t, B.m_critic2, B.v_critic2, B.grad_critic2, B.ws2, B.losses2, 0.2, 0.5)
        rc = fn(by(t3), r, g, t, B.tc2 if a["t"] is not None else None, hp, None, a["ring_len"], 7, 0, 1e-4, bp[0], bp[1], 1e-4, bp[2], bp[3],
                1, a["flags"], None)
    else:
        per = S._capi.PerArgs(B.prio, B.pmax, B.per_ws, 0.6, 0.4, 1e-3, 0)
        rc = fn(d, r, g, t, hp, by(per), a["ring_len"], 0, 0, 7, 0, 1e-4, bp[0], bp[1], 1e-4, bp[2], bp[3], a["flags"], None)
    return rc, L.shems_last_error().decode()


@pytest.mark.parametrize("name", ENTRY)
def test_every_entry_point_refuses_the_common_faults_before_any_launch(env, name):
    S, D, G, T, L, B = env
    rows, valid = _table(D, G, B)
    for what, kw, word, not_for in rows:
        if name in not_for:                        # the entry point does not take or need it: such a call would go on to launch
            continue
        rc, msg = _call(env, name, {**valid, **kw})
        assert rc == S._capi.ERR_ARG and name in msg and word in msg, (name, what, rc, msg)
    assert not B.raw.any()

"""Grouped imitation without a GPU: the two entry points in the header, the library and the ctypes table, the stride arithmetic of
imitation.GroupDemos / GroupRings, every SHEMS_ERR_ARG refusal of the entry points (they return before the first HIP call: host memory
stands in for the device pointers, which are never dereferenced on these paths) and the refusals of the Python layer."""
import ctypes as C
import importlib
import os
import re
import types

import numpy as np
import pytest

import util as U

ENTRY = ("shems_ddpg_group_clone_update_tp", "shems_ddpg_group_critic_update_tp")


def _mods():
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    return S, mod("ddpg"), mod("group"), mod("imitation")


def test_header_library_and_ctypes_table_agree_on_the_two_entry_points(built_lib):
    S, D, G, I = _mods()
    L = G._declare_group()
    assert set(ENTRY) <= set(S._capi.exported_symbols())
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    for name in ENTRY:
        assert hasattr(L, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert n_args == 14 == len(getattr(L, name).argtypes), (name, n_args)
        assert getattr(L, name).restype is C.c_int
        assert "int64_t ring_stride_bytes" in m.group(1)


def test_ring_slab_stride_arithmetic():
    S, D, G, I = _mods()
    torch = pytest.importorskip("torch")
    for cap in (1, 3, 30, 127, 128, 24000):
        offs, floats = I.ring_slab_floats(cap)
        assert floats % 4 == 0 and [offs[k][1] for k in ("s", "a", "r", "s2")] == [9 * cap, 2 * cap, cap, 9 * cap]
        assert 4 * offs["done"][1] >= cap                                # the done bytes fit their floats
        end = 0
        for k in ("s", "a", "r", "s2", "done"):                         # in order, on 16-byte boundaries, without overlap
            assert offs[k][0] % 4 == 0 and offs[k][0] >= end
            end = offs[k][0] + offs[k][1]
        assert end <= floats < end + 4
    with pytest.raises(ValueError, match="capacity"):
        I.ring_slab_floats(0)
    for cls, ring_cls in ((I.GroupDemos, I.Demos), (I.GroupRings, D.ReplayRing)):
        gr = cls(3, 30, device="cpu")
        assert gr.stride_bytes == 4 * I.ring_slab_floats(30)[1] and gr.stride_bytes % 16 == 0 and len(gr) == 3 and len(gr.rings) == 3
        r0 = gr.struct0()
        assert r0.capacity == 30
        for l, ring in enumerate(gr.rings):
            assert type(ring) is ring_cls and ring.capacity == 30 and len(ring) == 0
            for k in ("s", "a", "r", "s2", "done"):                     # ring l = ring 0 + l * stride, every array
                assert getattr(ring, k).data_ptr() == getattr(r0, k) + l * gr.stride_bytes, (l, k)
            assert ring.done.dtype == torch.uint8 and ring.done.shape == (30,) and ring.s.shape == (30, 9)
        gr.rings[1].s.fill_(1.0); gr.rings[1].done.fill_(255)           # a ring's arrays are its own
        assert not gr.rings[0].s.any() and not gr.rings[2].s.any() and not gr.rings[0].done.any() and not gr.rings[2].a.any()
    with pytest.raises(ValueError, match="count"):
        I.GroupRings(0, 30, device="cpu")


def test_entry_points_refuse_bad_arguments_before_any_launch(built_lib):
    S, D, G, I = _mods()
    L = G._declare_group()
    # 16-byte aligned host blocks stand in for the device buffers
    raw = np.zeros(64 + 8, np.float32)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16
    names = [n for n, _ in D.DdpgArgs._fields_[:14]]
    cap = 16
    arr = dict(s=np.zeros((cap, 9), np.float32), a=np.zeros((cap, 2), np.float32), r=np.zeros(cap, np.float32),
               s2=np.zeros((cap, 9), np.float32), done=np.zeros(cap, np.uint8))

    def ddpg(batch=120, **without):
        d = D.DdpgArgs(*([base] * 14), 0.99, 1.0, batch, 0)
        for k, v in without.items():
            setattr(d, k, v)
        return d

    def ring(capacity=cap, without=()):
        return S._capi.Replay(capacity, *(arr[k].ctypes.data if k not in without else None for k in ("s", "a", "r", "s2", "done")))

    def call(name, **kw):
        a = dict(d=ddpg(), ring=ring(), stride=64, g=G.Group(2, 0, 4096, 32), t=None, hp=None, ring_len=cap, eta=1e-4, bp1=0.9, bp2=0.999, flags=0)
        a.update(kw)
        by = lambda x: C.byref(x) if x is not None else None
        rc = getattr(L, name)(by(a["d"]), by(a["ring"]), a["stride"], by(a["g"]), by(a["t"]), a["hp"], a["ring_len"], 7, 0, a["eta"], a["bp1"],
                              a["bp2"], a["flags"], None)
        return rc, L.shems_last_error().decode()

    both = [(dict(g=None), "shems_group"), (dict(g=G.Group(0, 0, 4096, 32)), "shems_group"), (dict(g=G.Group(2, 0, 4100, 32)), "shems_group"),
            (dict(g=G.Group(2, 0, 0, 32)), "shems_group"), (dict(g=G.Group(65536, 0, 4096, 32)), "shems_group"),
            (dict(stride=-64), "ring stride -64"), (dict(stride=66), "ring stride 66"), (dict(stride=0), "ring stride 0"),
            (dict(d=None), "NULL buffer"), (dict(d=ddpg(actor=None)), "NULL buffer"), (dict(d=ddpg(actor_t=None)), "NULL buffer"),
            (dict(d=ddpg(s_min=None)), "NULL buffer"), (dict(d=ddpg(s_max=None)), "NULL buffer"), (dict(d=ddpg(ws=None)), "NULL buffer"),
            (dict(d=ddpg(losses=None)), "NULL buffer"), (dict(flags=2), "unknown flag"), (dict(d=ddpg(batch=0)), "batch"),
            (dict(d=ddpg(batch=129)), "batch"), (dict(hp=C.c_void_p(base + 4)), "d_hp"), (dict(d=ddpg(ws=base + 4)), "16-byte aligned"),
            (dict(d=ddpg(actor=base + 8)), "16-byte aligned"), (dict(ring=None), "ring"), (dict(ring=ring(without=("s",))), "ring"),
            (dict(ring=ring(without=("a",))), "ring"), (dict(ring_len=0), "ring length"), (dict(ring_len=cap + 1), "ring length"),
            (dict(bp1=0.0), "beta powers"), (dict(bp2=1.0), "beta powers"), (dict(bp1=float("nan")), "beta powers"),
            (dict(t=G.GroupW2T(base, None)), "both regions"), (dict(t=G.GroupW2T(base + 4, base)), "16-byte aligned")]
    clone_only = [(dict(d=ddpg(m_actor=None)), "NULL buffer"), (dict(d=ddpg(v_actor=None)), "NULL buffer"),
                  (dict(d=ddpg(grad_actor=None), flags=1), "STORE_GRAD")]
    critic_only = [(dict(d=ddpg(critic=None)), "NULL buffer"), (dict(d=ddpg(critic_t=None)), "NULL buffer"), (dict(d=ddpg(m_critic=None)), "NULL buffer"),
                   (dict(d=ddpg(v_critic=None)), "NULL buffer"), (dict(d=ddpg(grad_critic=None), flags=1), "STORE_GRAD"),
                   (dict(d=ddpg(critic=base + 8)), "16-byte aligned")] + \
                  [(dict(ring=ring(without=(k,))), "s, a, r, s2 and done") for k in ("r", "s2", "done")]
    for name, cases in ((ENTRY[0], both + clone_only), (ENTRY[1], both + critic_only)):
        for kw, word in cases:
            rc, msg = call(name, **kw)
            assert rc == S._capi.ERR_ARG and name in msg and word in msg, (name, kw, msg)
    assert not raw.any() and not any(v.any() for v in arr.values())


def test_python_layer_refuses_before_the_library_is_asked(monkeypatch):
    S, D, G, I = _mods()
    class R:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    grp = types.SimpleNamespace(form="wide", count=2)
    for what in ("clone", "evaluate"):
        with pytest.raises(NotImplementedError, match=what + ".*wide"):
            G.LearnerGroup._group_rings(grp, None, what)
    grp = types.SimpleNamespace(form="throughput", count=2, device="cpu", slab_floats=100, rings=[R(5), R(5)], _ring0=lambda: "r0")
    assert G.LearnerGroup._group_rings(grp, None, "evaluate") == (grp.rings, "r0", 400, 5)
    dev = types.SimpleNamespace(device="cpu")
    with pytest.raises(ValueError, match="3 rings for a group of 2"):
        G.LearnerGroup._group_rings(grp, types.SimpleNamespace(rings=[1, 2, 3]), "clone")

    class RS(R):
        s = dev
    with pytest.raises(ValueError, match=r"clone: the rings hold unequal lengths \(7 \.\. 9\)"):
        G.LearnerGroup._group_rings(grp, types.SimpleNamespace(rings=[RS(7), RS(9)], stride_bytes=64, struct0=lambda: "r0"), "clone")
    other = types.SimpleNamespace(device="cuda:1")

    class RO(R):
        s = other
    with pytest.raises(ValueError, match="the rings live on"):
        G.LearnerGroup._group_rings(grp, types.SimpleNamespace(rings=[RO(7), RO(7)], stride_bytes=64, struct0=lambda: "r0"), "clone")
    ok = types.SimpleNamespace(rings=[RS(7), RS(7)], stride_bytes=64, struct0=lambda: "r0")
    assert G.LearnerGroup._group_rings(grp, ok, "clone") == (ok.rings, "r0", 64, 7)
    grp._group_rings = lambda rings, what: G.LearnerGroup._group_rings(grp, rings, what)
    for tau in (0.0, -1.0, 1.5):
        with pytest.raises(ValueError, match="tau"):
            G.LearnerGroup._half_update(grp, "clone", ok, None, tau, False)

    def no_lib():
        raise AssertionError("refused before the library is loaded")

    monkeypatch.setattr(S._capi, "lib", no_lib)
    F = importlib.import_module(U.PKG_NAME + ".foresight")
    val = F.Values(F.Grid(9, 5, 5, 3), 5, [None], None, None, None, total_rows=40)
    with pytest.raises(ValueError, match="at least one of each"):
        I.dagger_group(None, None, val, None, 0, 3)
    with pytest.raises(ValueError, match="at least one of each"):
        I.dagger_group(None, None, val, None, 2, 0)
    with pytest.raises(ValueError, match="forecast ensemble"):
        I.dagger_group(None, None, F.EnsembleValues(val, 2, np.ones((1, 2)) / 2), None, 1, 1)
    g2, env3 = types.SimpleNamespace(count=2, rings=[1, 2]), types.SimpleNamespace(n=3)
    with pytest.raises(ValueError, match="3 envs for a group of 2"):
        I.dagger_group(g2, env3, val, ok, 1, 1)
    with pytest.raises(ValueError, match="1 rings for a group of 2"):
        I.dagger_group(g2, types.SimpleNamespace(n=2), val, types.SimpleNamespace(rings=[1]), 1, 1)
    with pytest.raises(ValueError, match="at least one"):
        I.warm_start_group(g2, env3, val, ok, ok, 1, 1, 0)
    with pytest.raises(ValueError, match="neither 'td' nor 'mc'"):
        I.warm_start_group(g2, env3, val, ok, ok, 1, 1, 5, mode="x")
    own = types.SimpleNamespace(rings=g2.rings)
    with pytest.raises(ValueError, match="training ring"):
        I.warm_start_group(g2, types.SimpleNamespace(n=2), val, ok, own, 1, 1, 5, mode="mc")

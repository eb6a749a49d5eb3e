"""Host-side tests of the learner group's evaluation sweep (LearnerGroup.run_episodes, shems_group_eval_best_dev): the C declaration
against the ctypes one, the exported symbol, and every argument error -- all raised before any device work."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import util as U

FN = "shems_group_eval_best_dev"


def _g():
    U.pkg()
    return importlib.import_module(U.PKG_NAME + ".group")


def _header_params():
    txt = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    m = re.search(r"int\s+" + FN + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, "the header declares " + FN
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_and_ctypes_declarations_agree(built_lib):
    G = _g()
    from importlib import import_module
    D = import_module(U.PKG_NAME + ".ddpg")
    L = G._declare_group()
    params = _header_params()
    want = []
    for p in params:
        star = "*" in p
        base = re.sub(r"[*]", " ", p).replace("const ", "").split()[0]
        if star and base == "shems_ddpg":
            want.append(C.POINTER(D.DdpgArgs))
        elif star and base == "shems_group":
            want.append(C.POINTER(G.Group))
        elif star and base == "shems_group_w2t":
            want.append(C.POINTER(G.GroupW2T))
        elif star:
            want.append(C.c_void_p)
        else:
            want.append({"int32_t": C.c_int32, "int64_t": C.c_int64}[base])
    assert len(params) == 15
    assert list(L.shems_group_eval_best_dev.argtypes) == want
    assert L.shems_group_eval_best_dev.restype is C.c_int


def test_symbol_is_exported_and_listed(built_lib):
    S = U.pkg()
    assert FN in S._capi.exported_symbols()
    assert hasattr(S._capi.lib(), FN)


# ---- argument errors of the C entry point (fake, aligned addresses: no check dereferences them, no call reaches the device) --------
A16 = 0x7f0000000000


def _call(**over):
    G = _g()
    from importlib import import_module
    D = import_module(U.PKG_NAME + ".ddpg")
    L = G._declare_group()
    row = 4 * (((129002 + 3) & ~3) + 32)
    a = dict(actor=A16, s_min=A16 + 0x100000, s_max=A16 + 0x100040, count=4, stride=1 << 20, epl=128, t=None, l1=0, l2=0,
             returns=A16 + 0x200000, runs=100, episode=1, score=A16 + 0x300000, best_score=A16 + 0x300100, best_run=A16 + 0x300200,
             improved=A16 + 0x300300, best0=A16 + 0x400000, best_stride=row)
    a.update(over)
    d = D.DdpgArgs()
    d.actor, d.s_min, d.s_max = a["actor"], a["s_min"], a["s_max"]
    g = G.Group(a["count"], 0, a["stride"], a["epl"])
    t = a["t"]
    rc = L.shems_group_eval_best_dev(C.byref(d), C.byref(g), C.byref(t) if t is not None else None, a["l1"], a["l2"], a["returns"],
                                     a["runs"], a["episode"], a["score"], a["best_score"], a["best_run"], a["improved"], a["best0"],
                                     a["best_stride"], None)
    return rc, (L.shems_last_error().decode() if rc else "")


ROW = 4 * (((129002 + 3) & ~3) + 32)


@pytest.mark.parametrize("over,word", [
    (dict(count=0), "count >= 1"),
    (dict(stride=8), "16-byte-multiple stride"),
    (dict(count=2, stride=0), "16-byte-multiple stride"),
    (dict(epl=100), "multiple of 32"),
    (dict(epl=0), "multiple of 32"),
    (dict(runs=0), "runs must be in 1..envs_per_learner"),
    (dict(runs=129), "runs must be in 1..envs_per_learner"),
    (dict(actor=0), "actor, s_min and s_max"),
    (dict(s_max=0), "actor, s_min and s_max"),
    (dict(actor=A16 + 8), "actor block must be 16-byte aligned"),
    (dict(returns=0), "required"),
    (dict(best0=0), "required"),
    (dict(improved=0), "required"),
    (dict(returns=A16 + 0x200004), "8-byte"),
    (dict(best_run=A16 + 0x300202), "4-byte"),
    (dict(best0=A16 + 0x400008), "snapshot slab"),
    (dict(best_stride=ROW + 8), "snapshot slab"),
    (dict(best_stride=ROW - 16), "snapshot slab"),
    (dict(l1=300, l2=600, t="tiled"), "t must be NULL"),
    (dict(l1=5000, l2=600), "outside 1..4096"),
    (dict(t="unaligned"), "shems_group_w2t.actor"),
    (dict(t="null"), "shems_group_w2t.actor"),
])
def test_bad_arguments_return_err_arg_with_a_message(built_lib, over, word):
    G = _g()
    if "t" in over:
        over = dict(over, t={"tiled": G.GroupW2T(A16 + 0x800000, A16 + 0xa00000), "unaligned": G.GroupW2T(A16 + 0x800004, A16 + 0xa00000),
                             "null": G.GroupW2T(0, A16 + 0xa00000)}[over["t"]])
    rc, msg = _call(**over)
    assert rc == -1, (over, rc)
    assert FN in msg and word in msg, msg


def test_wide_snapshot_row_follows_the_wide_parameter_count(built_lib):
    G = _g()
    L = G._declare_group()
    na, nc = C.c_int64(0), C.c_int64(0)
    assert L.shems_wide_params(300, 600, C.byref(na), C.byref(nc)) == 0
    row = 4 * (((na.value + 3) & ~3) + 32)
    rc, msg = _call(l1=300, l2=600, best_stride=row - 16)
    assert rc == -1 and str(row) in msg, msg


# ---- the Python checks that precede any device work --------------------------------------------------------------------------------
class _Env:
    def __init__(self, n):
        self.n = n


def _bare_group(count, E):
    G = _g()
    grp = G.LearnerGroup.__new__(G.LearnerGroup)
    grp.count, grp.envs_per_learner = count, E
    return grp


@pytest.fixture
def no_device(monkeypatch):
    import torch
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work"))
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(torch, "zeros", boom)


@pytest.mark.parametrize("n_train,n_eval,kw,word", [
    (4 * 32 - 32, 4 * 128, {}, "env_train holds"),
    (4 * 32, 4 * 128, dict(num_ep=0), "num_ep"),
    (4 * 32, 4 * 128, dict(test_every=0), "test_every"),
    (4 * 32, 4 * 128 + 33, {}, "equal blocks"),
    (4 * 32, 2, {}, "equal blocks"),
    (4 * 32, 4 * 100, dict(test_runs=100), "multiple of 32"),
    (4 * 32, 4 * 96, dict(test_runs=100), "test_runs 100"),
    (4 * 32, 4 * 128, dict(test_runs=0), "test_runs 0"),
])
def test_run_episodes_refuses_before_any_device_work(no_device, n_train, n_eval, kw, word):
    grp = _bare_group(4, 32)
    args = dict(num_ep=3, test_every=2, test_runs=100)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        grp.run_episodes(_Env(n_train), _Env(n_eval), **args)


def test_run_episodes_check_returns_the_eval_block():
    G = _g()
    assert G.run_episodes_check(400, 400 * 128, 400 * 128, 400 * 128, 1001, 100, 100) == 128
    assert G.run_episodes_check(3, 96, 96, 3 * 32, 5, 2, 32) == 32


@pytest.mark.parametrize("args,kw,word", [
    (([np.zeros((2000, 8), np.float32)], [0, 0, 0], 4), {}, "3 entries for 4 learners"),
    (([np.zeros((2000, 8), np.float32)], [0, 1], 2), {}, "names table 1"),
    (([np.zeros((2000, 8), np.float32)], [0, -1], 2), {}, "names table -1"),
    (([], [], 0), {}, ">= 1"),
    (([], [0], 1), {}, "at least one table"),
    (([np.zeros((2000, 8), np.float32)], [0], 1), dict(test_runs=0), ">= 1"),
    (([np.zeros((2000, 8), np.float32)] * 2, [0], 1), dict(charger_ids=[1]), "charger_ids holds 1"),
    (([np.zeros((2000, 8), np.float32)], [0], 1), dict(maxsteps=71), "maxsteps 71"),
])
def test_eval_batch_refuses_before_any_device_work(no_device, args, kw, word):
    G = _g()
    with pytest.raises(ValueError, match=word):
        G.eval_batch(*args, **kw)

"""TD3 for learner groups without a GPU: the ctypes mirror of the new entry points against the header, the slab layout, the schedule,
the constructor's refusals, the per-learner noise streams, and -- on the NumPy twin alone -- the coverage and tie conditions of the cases
tests/test_group_td3_gpu.py runs on the device (tests/group_td3_cases.py holds the cases for both files).

The ctypes, layout and refusal tests exercise the library and the package.  The noise-stream, coverage and tie tests check TEST
INFRASTRUCTURE -- that the case file's seeds and ticks meet their conditions on the twin -- and touch the package only through
_feature(): the constants the cases rest on are the package's (the critic-2 seed offset, the pass width, the published rows)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import group_td3_cases as K
import td3_ref as TR
import util as U


def _T():
    return importlib.import_module(U.PKG_NAME + ".td3")


def _G():
    return importlib.import_module(U.PKG_NAME + ".group")


def _feature():
    """The package side of what the case file assumes: fails where the grouped TD3 update does not exist."""
    T = _T()
    assert issubclass(T.TD3LearnerGroup, _G().LearnerGroup)
    assert K.C2_OFFSET == T.CRITIC2_SEED_OFFSET and T.BP == 128 and T.GROUP_WS2_PUB % 4 == 0
    return T


_CTYPES_OF = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}


def _header_argtypes(name):
    """The ctypes argument list the header's declaration of `name` implies: scalars by width, every pointer a pointer."""
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/shems_hip.h"
    out = []
    for arg in m.group(1).split(","):
        arg = re.sub(r"\bconst\b", " ", arg).strip()
        mm = re.match(r"^(\w+)\s*(\**)\s*(\w+)$", arg)
        assert mm, arg
        out.append("ptr" if mm.group(2) else _CTYPES_OF[mm.group(1)])
    return out


def test_ctypes_mirror_matches_the_header(built_lib, tmp_path):
    T, G = _T(), _G()
    L = T._declare_group()
    for fn in ("shems_td3_group_workspace_floats", "shems_td3_group_update_tp"):
        assert hasattr(L, fn), fn
        want = _header_argtypes(fn)
        got = getattr(L, fn).argtypes
        assert len(got) == len(want), (fn, len(got), len(want))
        for pos, (g, w) in enumerate(zip(got, want)):
            if w == "ptr":
                assert g is C.c_void_p or issubclass(g, C._Pointer), (fn, pos, g)
            else:                                  # (c_int and c_int32 are one ctypes class where int is 32 bits wide)
                assert g is w, (fn, pos, g, w)
        assert getattr(L, fn).restype is C.c_int
    # the position of every pointer-typed struct argument: shems_td3, shems_replay, shems_group, shems_group_w2t
    a = L.shems_td3_group_update_tp.argtypes
    assert a[0]._type_ is T.Td3Args and a[2]._type_ is G.Group and a[3]._type_ is G.GroupW2T
    # gcc lays the header's shems_td3 out; the mirror has its size and offsets, and the published rows begin where the header says
    names = [f[0] for f in T.Td3Args._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shems_hip.h"\nint main(void){printf("%zu %d", sizeof(shems_td3), '
                   'SHEMS_TD3_GROUP_WS2_PUB);' + "".join(f'printf(" %zu", offsetof(shems_td3, {n}));' for n in names) + 'return 0;}\n')
    exe = tmp_path / "o"
    subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(T.Td3Args) and vals[1] == T.GROUP_WS2_PUB
    assert vals[2:] == [getattr(T.Td3Args, n).offset for n in names]
    n = C.c_int64(0)
    assert L.shems_td3_group_workspace_floats(C.byref(n)) == 0 and n.value >= T.GROUP_WS2_PUB + 5 * T.BP and n.value % 4 == 0
    assert L.shems_td3_group_workspace_floats(None) != 0


@pytest.mark.parametrize("tiled", [True, False])
def test_slab_layout_keeps_the_ddpg_offsets_and_appends_the_td3_blocks(tiled):
    T, G = _T(), _G()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    nws, cap = 1902568, K.CAP
    base, n_base = G.slab_layout(D.N_ACTOR, D.N_CRITIC, nws, cap, tiled)
    extra = T.group_extra_blocks(D.N_CRITIC, tiled, 99464)
    lay, n = G.slab_layout(D.N_ACTOR, D.N_CRITIC, nws, cap, tiled, extra)
    assert list(lay)[:len(base)] == list(base) and all(lay[k] == base[k] for k in base)         # every DDPG offset unchanged
    names = [e[0] for e in extra]
    assert names == ["critic2", "critic2_t", "m_critic2", "v_critic2", "grad_critic2", "w2t_critic2", "ws2", "losses2"]
    end_ring = base["ring_done"][0] + base["ring_done"][1]
    assert n_base == (end_ring + 3) & ~3
    spans = sorted((lay[k][0], lay[k][0] + lay[k][1], k) for k in names)
    assert spans[0][0] >= n_base                                                                # after ring_done
    for (lo, hi, k), nxt in zip(spans, spans[1:] + [(n, n, "end")]):
        assert lo % 4 == 0 and hi <= nxt[0], (k, lo, hi, nxt)                                   # 16-byte aligned, non-overlapping
    assert lay["w2t_critic2"][1] == (G.W2T_FLOATS if tiled else 0) and lay["losses2"][1] == 1
    assert all(lay[k][1] == D.N_CRITIC for k in T.CRITIC2_BLOCKS)
    with pytest.raises(ValueError):
        G.slab_layout(D.N_ACTOR, D.N_CRITIC, nws, cap, tiled, (("critic", 4),))


def test_schedule():
    T = _feature()
    with pytest.raises(ValueError):                          # the group's constructor check is the schedule's
        T.group_refusals(policy_delay=0)
    assert [T.is_policy_step(u, 2) for u in range(4)] == [False, True, False, True]
    assert all(T.is_policy_step(u, 1) for u in range(5))
    assert [T.is_policy_step(u, 3) for u in range(6)] == [False, False, True, False, False, True]
    with pytest.raises(ValueError):
        T.is_policy_step(0, 0)


def test_constructor_refusals_come_before_any_device_work():
    """Every refusal names its reason; none of them needs a device (this test runs without one)."""
    T = _T()
    mk = lambda **kw: T.TD3LearnerGroup(2, 32, **kw)
    for kw, exc, word in ((dict(form="latency"), NotImplementedError, "latency"), (dict(form="wide"), NotImplementedError, "wide"),
                          (dict(noise_type="ou"), NotImplementedError, "Ornstein-Uhlenbeck"),
                          (dict(hparams=[{"mem_size": 64}, {}]), NotImplementedError, "mem_size"),
                          (dict(hparams=[{}, {"batch": 129}]), NotImplementedError, "batch 129"),
                          (dict(hparams=[{"hidden": (300, 600)}, {}]), NotImplementedError, "hidden"),
                          (dict(hidden=(300, 600)), NotImplementedError, "hidden="),
                          (dict(sigma_trg=-0.1), ValueError, "sigma_trg"), (dict(clip_trg=float("nan")), ValueError, "clip_trg"),
                          (dict(sigma_trg=float("inf")), ValueError, "sigma_trg"), (dict(policy_delay=0), ValueError, "policy_delay"),
                          (dict(form="fast"), ValueError, "form")):
        with pytest.raises(exc) as ei:
            mk(**kw)
        assert word in str(ei.value), (kw, str(ei.value))


def test_per_learner_noise_streams_are_different_and_reproducible():
    n = _feature().BP
    z = [TR.target_noise(K.RNG_SEED + l, K.TICKS[0], n) for l in range(4)]
    for i in range(4):
        assert np.array_equal(z[i], TR.target_noise(K.RNG_SEED + i, K.TICKS[0], n))
        assert not (z[i] == TR.target_noise(K.RNG_SEED + i, K.TICKS[1], n)).any()
        for j in range(i + 1, 4):
            assert not (z[i] == z[j]).any(), (i, j)
    # the sampler's stream of the same key carries another tag: the draws are not the sampler's words
    ctr, _ = TR.target_words(K.RNG_SEED + 1, K.TICKS[0], 4)
    assert (ctr[:, 3] == TR.STREAM_TARGET).all() and (ctr[:, 4] == K.RNG_SEED + 1).all()


@pytest.mark.parametrize("L,batch,policy", K.STAGE_CASES)
def test_the_gpu_cases_meet_their_coverage_and_tie_conditions_on_the_twin(L, batch, policy):
    assert batch <= _feature().BP
    for l in K.checked(L):
        for tick in K.ticks_of((L, batch, policy)):
            K.assert_coverage(l, tick, batch)
            assert K.initial_ties(l, tick, batch) == [], (l, tick, batch)
    assert K.EXPECTED_TIES[(L, batch, policy)] == []


def test_the_record_case_meets_its_conditions_on_the_twin():
    T = _feature()
    T.group_refusals(hparams=K.RECORD_CASE)                  # the records are ones a TD3 group takes
    for l, rec in enumerate(K.RECORD_CASE):
        for tick in K.TICKS:
            K.assert_coverage(l, tick, rec["batch"])
            assert K.initial_ties(l, tick, rec["batch"]) == []


def test_group_refusals_word_for_word_and_in_order():
    T = _feature()
    rows = U.group_variant_refusal_rows("TD3 learner group", "twin-critic update", "twin-critic update", "shems_td3_group_update_tp", "",
                      "the twin-critic update holds one 128-column pass")
    own = [(dict(sigma_trg=-0.5), ValueError, "TD3 learner group: sigma_trg = -0.5, clip_trg = 0.5 must be finite and >= 0"),
           (dict(policy_delay=0), ValueError, "policy_delay = 0: the actor moves every 1 or more updates"),
           (dict(hparams=[{"hidden": (300, 600)}], sigma_trg=-0.5), NotImplementedError, rows[7][2]),            # the walk before the own numbers
           (dict(sigma_trg=-0.5, policy_delay=0), ValueError, "TD3 learner group: sigma_trg = -0.5, clip_trg = 0.5 must be finite and >= 0")]
    for kw, exc, message in rows + own:
        with pytest.raises(exc) as ei:
            T.group_refusals(**kw)
        assert str(ei.value) == message, kw
    assert T.group_refusals() is None and T.group_refusals(form="throughput", hparams=[{"batch": 128, "hidden": (250, 500)}]) is None

"""Population-based training without a GPU: the NumPy twin (tests/pbt_ref.py) against hand-traced rounds and against a host build of
csrc/shems_pbt_core.h bit for bit on every case the GPU test runs; the parameter check by field; the C structs, prototypes and exports;
the native argument checks; the Python refusals; the ranges a group copies."""
import ctypes as C
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

import pbt_cases as PC
import pbt_ref as PR
import util as U

f32, f64 = np.float32, np.float64


def _hostcheck(tmp_path, sanitize=False):
    exe = str(tmp_path / ("pbt_hostcheck_san" if sanitize else "pbt_hostcheck"))
    src = os.path.join(U.ROOT, "tests", "hostcheck", "pbt_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] +
                          (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + ["-o", exe, src])
    return exe


def _params_struct(p):
    S = U.pkg()
    return S._capi.PbtParams(p["seed"], p["round"], p["permille"], p["fields"], p.get("reserved", 0), p["down"], p["up"],
                             (C.c_double * 4)(*p["lo"]), (C.c_double * 4)(*p["hi"]))


def _run(exe, tmp_path, case):
    path = str(tmp_path / "pbt_in.bin")
    n = len(case["pop"])
    with open(path, "wb") as f:
        f.write(bytes(_params_struct(case["params"])))
        f.write(np.int32(n).tobytes())
        f.write(np.ascontiguousarray(case["pop"], np.int32).tobytes())
        f.write(np.ascontiguousarray(case["score"], f64).tobytes())
        f.write(case["hp"].tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = {}
    for line in out.stdout.strip().split("\n"):
        k, *w = line.split()
        rows[k] = w
    assert rows["check"][0] == "0", rows["check"]
    hp = np.frombuffer(bytes(int(x, 16) for x in rows["hp"]), PR.REC)
    return hp, np.array(rows["parent"], np.int32), np.array(rows["rank"], np.int32)


def _check_all(exe, tmp_path, names=None):
    seen = 0
    for name, case in PC.select_cases():
        if names is not None and name not in names:
            continue
        hp, parent, rank = _run(exe, tmp_path, case)
        w_hp, w_parent, w_rank = PR.round_twin(case["params"], case["pop"], case["score"], case["hp"])
        assert (rank == w_rank).all() and (parent == w_parent).all(), name
        assert hp.tobytes() == w_hp.tobytes(), name
        seen += 1
    return seen


def test_twin_on_hand_traced_rounds():
    """Rounds small enough to trace by hand.  One population of 8, permille 250: q = 2; the order is by score with the lower index
    winning a tie, non-finite last.  The parent draw and the factor bits are read off the Philox block directly."""
    score = np.array([-300.0, -500.0, -300.0, np.nan, -100.0, -900.0, -np.inf, -400.0])
    pop = np.zeros(8, np.int32)
    assert list(PR.ranks(pop, score)) == [1, 4, 2, 6, 0, 5, 7, 3]             # -100 | -300 (l 0) | -300 (l 2) | -400 | -500 | -900 | NaN (l 3) | -inf (l 6)
    hp = PR.records(8)
    p = PR.params(seed=(5 << 32) | 9, round=3, permille=250, fields=15)
    out, parent, rank = PR.round_twin(p, pop, score, hp)
    children = [3, 6]                                                          # rank >= 8 - 2
    assert [l for l in range(8) if parent[l] != l] == children and list(rank) == [1, 4, 2, 6, 0, 5, 7, 3]
    import philox_np as PH
    for l in children:
        x, y, _, _ = PH.philox4x32_10(l, 3, 0, 0x5042545F, 9, 5)
        par = [4, 0][(int(x) * 2) >> 32]                                       # the learners of rank 0 and 1
        assert parent[l] == par
        fac = [1.2 if int(y) >> k & 1 else 0.8 for k in range(4)]
        assert out[l]["eta_act"] == f64(f32(hp[par]["eta_act"] * fac[0])) and out[l]["eta_crit"] == f64(f32(hp[par]["eta_crit"] * fac[1]))
        assert out[l]["tau"] == f32(f64(hp[par]["tau"]) * fac[2]) and out[l]["noise_sigma"] == f32(f64(hp[par]["noise_sigma"]) * fac[3])
        assert all(out[l][k] == hp[par][k] for k in ("gamma", "noise_mu", "batch", "reserved"))          # the parent's whole record
    kept = [l for l in range(8) if l not in children]
    assert out[kept].tobytes() == hp[kept].tobytes()
    # the quota in integers: P = 3 at permille 250 and 333 gives q = 0, P = 7 at 500 gives 3, P = 1 always 0
    for P, pm, q in ((3, 250, 0), (3, 333, 0), (3, 334, 1), (7, 500, 3), (1, 500, 0), (65, 250, 16), (8, 125, 1)):
        assert (P * pm) // 1000 == q
    out, parent, _ = PR.round_twin(PR.params(permille=250), np.array([1, 1, 1], np.int32), np.array([3.0, 2.0, 1.0]), PR.records(3))
    assert list(parent) == [0, 1, 2] and out.tobytes() == PR.records(3).tobytes()
    # a non-finite score that ranks as a parent: two learners, permille 500, q = 1; the only possible parent is NaN (index 0 beats index 1)
    out, parent, rank = PR.round_twin(PR.params(permille=500), np.zeros(2, np.int32), np.array([np.nan, np.inf]), PR.records(2))
    assert list(rank) == [0, 1] and list(parent) == [0, 1] and out.tobytes() == PR.records(2).tobytes()
    # selection never crosses populations: with one finite learner per population nobody has a parent of the other population
    out, parent, _ = PR.round_twin(PR.params(permille=500), np.array([0, 1, 0, 1], np.int32), np.array([1.0, 2.0, 3.0, 4.0]), PR.records(4))
    assert list(parent) == [2, 3, 2, 3]
    # clamping at both ends and exact arithmetic: 1.2 x up past hi, 0.8 x down past lo
    assert PR.explore_eta(1e-3, 1.2, 5e-4, float(f32(1.1e-3))) == float(f32(1.1e-3)) and PR.explore_eta(1e-3, 0.8, float(f32(9e-4)), 1.0) == float(f32(9e-4))
    assert PR.explore_f32(f32(0.9), 1.2, 0.0, 1.0) == f32(1.0) and PR.explore_f32(f32(0.1), 0.8, 0.0, 1.0) == f32(f64(f32(0.1)) * 0.8)


def test_cases_cover_what_the_issue_names():
    cases = dict(PC.select_cases())
    assert {len(c["pop"]) for c in cases.values()} == {1, 7, 8, 65}
    assert {c["params"]["fields"] for c in cases.values()} >= {0, 1, 2, 4, 8, 15}
    kept_nonfinite = clamp_lo = clamp_hi = ties = q0 = lone = nonfinite_child = 0
    for name, c in cases.items():
        p, pop, score, hp = c["params"], c["pop"], c["score"], c["hp"]
        out, parent, rank = PR.round_twin(p, pop, score, hp)
        ch = np.flatnonzero(parent != np.arange(len(pop)))
        assert out[parent == np.arange(len(pop))].tobytes() == hp[parent == np.arange(len(pop))].tobytes()
        for l in range(len(pop)):
            P = int((pop == pop[l]).sum())
            q = P * p["permille"] // 1000
            lone += P == 1
            q0 += P == 3 and q == 0
            if q and rank[l] >= P - q and parent[l] == l:
                kept_nonfinite += 1
            if q and rank[l] >= P - q and not np.isfinite(score[l]):
                nonfinite_child += 1
        for l in ch:
            assert pop[parent[l]] == pop[l] and np.isfinite(score[parent[l]]) and parent[parent[l]] == parent[l]
            for k, f in enumerate(PR.FIELDS):
                if p["fields"] >> k & 1:
                    clamp_lo += float(out[l][f]) == p["lo"][k]
                    clamp_hi += float(out[l][f]) == p["hi"][k]
        fin = score[np.isfinite(score)]
        ties += len(fin) > len(set(fin.tolist()))
    assert min(kept_nonfinite, clamp_lo, clamp_hi, ties, q0, lone, nonfinite_child) > 0, (kept_nonfinite, clamp_lo, clamp_hi, ties, q0, lone,
                                                                                          nonfinite_child)


def test_core_header_on_the_host_equals_the_twin_bit_for_bit(tmp_path):
    """tests/hostcheck/pbt_hostcheck.cpp, g++ -ffp-contract=off, on EVERY case the GPU test runs."""
    assert _check_all(_hostcheck(tmp_path), tmp_path) == len(dict(PC.select_cases())) == 64


def test_core_header_on_the_host_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: clean, and the same bits."""
    names = [n for n, _ in PC.select_cases()]
    pick = [n for n in names if n.startswith(("c65-", "c1-one", "c7-q0p3", "c8-two"))]
    assert _check_all(_hostcheck(tmp_path, sanitize=True), tmp_path, names=pick) == len(pick) >= 20


def test_params_check_by_field(built_lib):
    S = U.pkg()
    L = S._capi.declare_pbt()

    def check(**kw):
        p = dict(PR.params(), **kw)
        rc = L.shems_pbt_params_check(C.byref(_params_struct(p)))
        return rc, L.shems_last_error().decode()
    assert check()[0] == 0 and check(permille=1)[0] == 0 and check(permille=500)[0] == 0 and check(fields=0)[0] == 0
    lo, hi = list(PR.DEFAULT_LO), list(PR.DEFAULT_HI)
    sub = lambda v, k, x: tuple(x if i == k else y for i, y in enumerate(v))
    for kw, word in ((dict(permille=0), "permille outside 1 .. 500"), (dict(permille=501), "permille outside 1 .. 500"),
                     (dict(fields=16), "unknown bits"), (dict(reserved=1), "reserved"), (dict(down=0.0), "down must be finite and > 0"),
                     (dict(down=float("nan")), "down"), (dict(up=float("inf")), "up must be finite and > 0"), (dict(up=-1.0), "up"),
                     (dict(lo=sub(lo, 0, 0.0)), "eta_act: lo must be > 0"), (dict(lo=sub(lo, 1, -1.0)), "eta_crit: lo must be > 0"),
                     (dict(hi=sub(hi, 0, float("inf"))), "eta_act: bounds must be finite"), (dict(lo=sub(lo, 1, float("nan"))), "eta_crit: bounds must be finite"),
                     (dict(lo=sub(lo, 2, 0.0)), "tau: bounds must lie in (0, 1]"), (dict(hi=sub(hi, 2, 1.5)), "tau: bounds must lie in (0, 1]"),
                     (dict(lo=sub(lo, 3, -0.5)), "noise_sigma: lo must be >= 0"), (dict(lo=sub(lo, 3, 11.0)), "noise_sigma: lo above hi"),
                     (dict(lo=sub(lo, 0, 1e-6)), "eta_act: bounds must be Float32 values"), (dict(hi=sub(hi, 2, 0.3)), "tau: bounds must be Float32 values")):
        rc, msg = check(**kw)
        assert rc == S._capi.ERR_ARG and "shems_pbt_params_check" in msg and word in msg, (kw, msg)
    assert L.shems_pbt_params_check(None) == S._capi.ERR_ARG and "params is NULL" in L.shems_last_error().decode()
    # every bound the check passes keeps a clamped value valid for shems_group_hparams_check
    G = importlib.import_module(U.PKG_NAME + ".group")
    LG = G._declare_group()
    for k, edge in ((0, lo[0]), (1, hi[1]), (2, lo[2]), (2, 1.0), (3, 0.0), (3, hi[3])):
        rec = G.HParams(1e-3, 1e-3, 0.99, 0.01, 0.0, 0.1, 64, 0)
        setattr(rec, ("eta_act", "eta_crit", "tau", "noise_sigma")[k], edge)
        assert LG.shems_group_hparams_check((G.HParams * 1)(rec), 1) == 0, (k, edge)


_C_TO_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double,
                "float": C.c_float}


def test_prototypes_structs_and_exports(built_lib, tmp_path):
    S = U.pkg()
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    sigs = S._capi._pbt_sigs()
    assert set(sigs) == {"shems_pbt_params_check", "shems_pbt_select_dev", "shems_pbt_copy_dev"}
    for name, args in sigs.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        decl = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(decl) == len(args), (name, decl)
        for d, a in zip(decl, args):
            if "*" in d:
                base = d.replace("const", "").split("*")[0].strip()
                want = {"shems_pbt_params": (C.POINTER(S._capi.PbtParams),), "shems_pbt_range": (C.POINTER(S._capi.PbtRange),)}.get(base, (C.c_void_p,))
                assert a in want, (name, d, a)
            else:
                assert a is _C_TO_CTYPES[d.split()[0]], (name, d, a)
    pn, rn = [f[0] for f in S._capi.PbtParams._fields_], [f[0] for f in S._capi.PbtRange._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shems_hip.h"\nint main(void){printf("%zu %zu %zu %d %d %d %d", '
                   "sizeof(shems_pbt_params), sizeof(shems_pbt_range), sizeof(shems_group_hparams), SHEMS_PBT_FIELDS, SHEMS_PBT_MAX_RANGES, "
                   "SHEMS_PBT_MAX_COUNT, SHEMS_PBT_CHUNK_VECS);" +
                   "".join(f'printf(" %zu", offsetof(shems_pbt_params, {n}));' for n in pn) +
                   "".join(f'printf(" %zu", offsetof(shems_pbt_range, {n}));' for n in rn) +
                   'printf(" %d %d %d %d", SHEMS_PBT_ETA_ACT, SHEMS_PBT_ETA_CRIT, SHEMS_PBT_TAU, SHEMS_PBT_SIGMA);return 0;}\n')
    exe = tmp_path / "o"
    subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    G = importlib.import_module(U.PKG_NAME + ".group")
    assert vals[:3] == [C.sizeof(S._capi.PbtParams), C.sizeof(S._capi.PbtRange), C.sizeof(G.HParams)] == [104, 16, 40] and PR.REC.itemsize == 40
    assert vals[3:7] == [S._capi.PBT_FIELDS, S._capi.PBT_MAX_RANGES, S._capi.PBT_MAX_COUNT, S._capi.PBT_CHUNK_VECS] == [4, 8, 4096, PC.CHUNK_VECS]
    assert vals[7:7 + len(pn)] == [getattr(S._capi.PbtParams, n).offset for n in pn]
    assert vals[7 + len(pn):7 + len(pn) + 2] == [getattr(S._capi.PbtRange, n).offset for n in rn]
    assert vals[-4:] == [G.PBT_FIELD_BITS[k] for k in ("eta_act", "eta_crit", "tau", "sigma")] == [1, 2, 4, 8]
    assert [PR.REC.fields[n][1] for n in PR.REC.names] == [getattr(G.HParams, n).offset for n in PR.REC.names]
    assert set(sigs) <= set(S._capi.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib]).decode()
    assert set(sigs) <= set(re.findall(r" T (shems_[a-z0-9_]+)", out))
    L = S._capi.declare_pbt()
    assert all(getattr(L, n).argtypes == a for n, a in sigs.items())
    B = importlib.import_module(U.PKG_NAME + "._build")
    assert ("shems_pbt.hip", ["-ffp-contract=off"]) in B.UNITS
    core = open(os.path.join(U.ROOT, U.PKG_NAME, "csrc", "shems_pbt_core.h")).read()
    assert "kPbtMaxCount = 4096" in core and "kPbtMaxRanges = 8" in core
    assert f"kStreamPbt = 0x{PR.STREAM_PBT:08X}u" in open(os.path.join(U.ROOT, U.PKG_NAME, "csrc", "philox.h")).read()


def test_native_argument_checks(built_lib):
    """Every bad argument returns SHEMS_ERR_ARG by name and launches nothing (no device is needed to be refused)."""
    S = U.pkg()
    G = importlib.import_module(U.PKG_NAME + ".group")
    L = S._capi.declare_pbt()
    good = _params_struct(PR.params())

    def select(p=good, count=8, pop=64, score=64, hp=64, parent=64, rank=64):
        rc = L.shems_pbt_select_dev(C.byref(p) if p is not None else None, count, pop, score, hp, parent, rank, None)
        return rc, L.shems_last_error().decode()
    for kw, word in ((dict(count=0), "count = 0"), (dict(count=4097), "count = 4097 outside 1 .. 4096"), (dict(p=None), "NULL"), (dict(pop=None), "NULL"),
                     (dict(score=None), "NULL"), (dict(hp=None), "NULL"), (dict(parent=None), "NULL"), (dict(rank=None), "NULL"),
                     (dict(p=_params_struct(PR.params(permille=0))), "permille outside 1 .. 500"),
                     (dict(p=_params_struct(PR.params(permille=600))), "permille outside 1 .. 500"),
                     (dict(p=_params_struct(PR.params(lo=(0.0,) + PR.DEFAULT_LO[1:]))), "eta_act: lo must be > 0"),
                     (dict(hp=68), "alignment"), (dict(score=60), "alignment"), (dict(pop=66), "alignment"), (dict(rank=62), "alignment")):
        rc, msg = select(**kw)
        assert rc == S._capi.ERR_ARG and "shems_pbt_select_dev" in msg and word in msg, (kw, msg)

    def copy(ranges=((0, 516), (520, 12)), n=None, slab=4096, count=7, stride=4160, parent=64):
        arr = (S._capi.PbtRange * max(1, len(ranges)))(*[S._capi.PbtRange(o, k) for o, k in ranges])
        g = G.Group(count, 0, stride, 32)
        rc = L.shems_pbt_copy_dev(slab, C.byref(g), arr, len(ranges) if n is None else n, parent, None)
        return rc, L.shems_last_error().decode()
    for ranges, n, word in PC.bad_copy_args():
        rc, msg = copy(ranges=ranges, n=n)
        assert rc == S._capi.ERR_ARG and "shems_pbt_copy_dev" in msg and word in msg, (ranges, n, msg)
    for kw, word in ((dict(count=0), "count = 0"), (dict(count=65536), "count = 65536"), (dict(stride=4164), "stride_bytes = 4164"),
                     (dict(stride=0), "stride_bytes = 0"), (dict(slab=4100), "alignment"), (dict(parent=66), "alignment"), (dict(slab=None), "NULL"),
                     (dict(parent=None), "NULL")):
        rc, msg = copy(**kw)
        assert rc == S._capi.ERR_ARG and "shems_pbt_copy_dev" in msg and word in msg, (kw, msg)


def test_python_level_refusals(built_lib):
    """Everything population-based training does not cover is refused by name before any device work."""
    G = importlib.import_module(U.PKG_NAME + ".group")
    full, _ = G._hparams_records(4, [{}] * 4, 0.1, 1000)
    ok = dict(form="throughput", hparams=full, noise_type="gn", sized=False, populations=[0, 0, 1, 1], count=4)
    assert G.pbt_group_refusals(**ok) is None
    for kw, exc, word in ((dict(form="latency"), NotImplementedError, "form='latency'"), (dict(form="wide"), NotImplementedError, "form='wide'"),
                          (dict(hparams=None), ValueError, r"hparams=\[\{\}\] \* count"), (dict(noise_type="ou"), NotImplementedError, r"Ornstein-Uhlenbeck.*\*_x entry points"),
                          (dict(sized=True), NotImplementedError, r"per-learner mem_size.*\*_x entry points"),
                          (dict(populations=[0, 0, 1]), ValueError, "populations holds 3 ids for a group of 4 learners")):
        with pytest.raises(exc, match="population-based training: .*" + word):
            G.pbt_group_refusals(**dict(ok, **kw))
    mixed, _ = G._hparams_records(4, [{}, {"hidden": (100, 200)}, {}, {}], 0.1, 1000)
    with pytest.raises(ValueError, match=r"population 0 mixes hidden sizes \[\(100, 200\), \(250, 500\)\].*zero padding"):
        G.pbt_group_refusals(**dict(ok, hparams=mixed))
    assert G.pbt_group_refusals(**dict(ok, hparams=mixed, populations=[0, 1, 0, 0])) is None              # (alone in its population: nothing to mix)
    for bad in (0.0, 0.6, -0.1, 1, None, "0.25"):
        with pytest.raises(ValueError, match=r"truncation = .* outside \(0, 0.5\]"):
            G.PBT([0, 0], truncation=bad)
    with pytest.raises(ValueError, match="unknown field 'gamma'"):
        G.PBT([0, 0], fields=("eta_act", "gamma"))
    with pytest.raises(ValueError, match="bounds: unknown field 'batch'"):
        G.PBT([0, 0], bounds={"batch": (1, 2)})
    with pytest.raises(ValueError, match="one integer id per learner"):
        G.PBT([0.5, 1.0])
    with pytest.raises(ValueError, match="population-based training: shems_pbt_params_check: tau: bounds must lie in"):
        G.PBT([0, 0], bounds={"tau": (0.0, 1.0)})
    with pytest.raises(ValueError, match="shems_pbt_params_check: down must be finite and > 0"):
        G.PBT([0, 0], down=0.0)
    p = G.PBT([3, 3, 4, 4], truncation=0.5, fields=("sigma", "eta_act"), seed=11, start=7)
    assert (p.permille, p.mask, p.fields, p.seed, p.start) == (500, 9, ("eta_act", "sigma"), 11, 7) and p.populations.dtype == np.int32
    d = G.PBT([0])
    assert (d.permille, d.mask, d.down, d.up, d.seed, d.start) == (250, 15, 0.8, 1.2, None, None)
    assert tuple(d.bounds[k][0] for k in G.PBT_FIELD_BITS) == PR.DEFAULT_LO and tuple(d.bounds[k][1] for k in G.PBT_FIELD_BITS) == PR.DEFAULT_HI
    q = d.params(5, 0x1122334455)
    assert (q.seed, q.round, q.permille, q.fields, q.reserved, list(q.lo), list(q.hi)) == (0x1122334455, 5, 250, 15, 0, list(PR.DEFAULT_LO), list(PR.DEFAULT_HI))
    grp = types.SimpleNamespace(form="latency", hparams=None, noise_type="gn", _x=False, count=2)
    with pytest.raises(NotImplementedError, match="form='latency'"):                  # pbt_round and run_episodes refuse before anything else
        G.LearnerGroup.pbt_round(grp, [0.0, 0.0], d, 0)


def test_ranges_a_group_copies(built_lib):
    """pbt_ranges on the real layouts, tiled on and off, DDPG / TD3 / prioritized / n-step: the prefix actor .. w2t_critic and s_min | s_max
    (and the second critic's blocks), multiples of 4, never a gradient, workspace, ring, priority or n-step block."""
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    T = importlib.import_module(U.PKG_NAME + ".td3")
    ws = C.c_int64()
    assert D._declare().shems_ddpg_workspace_floats(C.byref(ws)) == 0
    copied = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "w2t_actor", "w2t_critic", "s_min", "s_max")
    for tiled in (False, True):
        for cls, extra, more in ((G.LearnerGroup, (), ()), (T.TD3LearnerGroup, tuple(T.group_extra_blocks(D.N_CRITIC, tiled, ws.value)),
                                                           ("critic2", "critic2_t", "m_critic2", "v_critic2", "w2t_critic2")),
                                 (G.PrioritizedLearnerGroup, tuple(G.per_extra_blocks(2400)), ()),
                                 (G.LearnerGroup, tuple(G.nstep_extra_blocks(3, 32)), ())):
            lay, n = G.slab_layout(D.N_ACTOR, D.N_CRITIC, ws.value, 2400, tiled, extra)
            ns = types.SimpleNamespace(layout=lay, _pbt_blocks=lambda cls=cls: cls._pbt_blocks(None))
            rg = G.LearnerGroup.pbt_ranges(ns)
            assert 2 <= len(rg) <= 4 and all(o % 4 == 0 and k % 4 == 0 and k > 0 and o + k <= n for o, k in rg)
            inside = lambda name: any(o <= lay[name][0] and lay[name][0] + lay[name][1] <= o + k for o, k in rg)
            touched = lambda name: any(lay[name][0] < o + k and o < lay[name][0] + lay[name][1] for o, k in rg)
            for name, (o, k) in lay.items():
                if k:
                    assert inside(name) == touched(name) == (name in copied + more), (cls.__name__, tiled, name)
            assert rg[0] == (0, lay["grad_actor"][0]) and rg[1] == (lay["s_min"][0], 24)

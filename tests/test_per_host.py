"""Prioritized replay without a GPU: the NumPy twin (tests/per_ref.py) against a host build of csrc/shems_per_core.h bit for bit, the
draw's distribution, the coverage of every GPU case, the C struct, the exports, the Python-level refusals and the entry-script switch."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ddpg_oracle as DO
import per_cases as PC
import per_ref as PR
import util as U

f32 = np.float32


def _hostcheck(tmp_path, sanitize=False):
    exe = str(tmp_path / ("per_hostcheck_san" if sanitize else "per_hostcheck"))
    src = os.path.join(U.ROOT, "tests", "hostcheck", "per_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] +
                          (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + ["-o", exe, src])
    return exe


def _run_hostcheck(exe, tmp_path, case, prio, diff, alpha=PR.ALPHA, eps_p=PR.EPS_P):
    path = str(tmp_path / "per_in.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4qQIi4f", case["capacity"], case["ring_len"], case["fresh"][0], case["fresh"][1], case["seed"],
                            case["tick"], case["batch"], case["pmax"], case["beta"], alpha, eps_p))
        f.write(np.ascontiguousarray(prio, f32).tobytes())
        f.write(np.ascontiguousarray(diff, f32).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = {}
    for line in out.stdout.strip().split("\n"):
        k, *w = line.split()
        rows[k] = np.array([int(x, 16) for x in w], np.uint64).astype(np.uint32)
    return rows


def _assert_hostcheck_equals_the_twin(rows, case, prio, diff, alpha=PR.ALPHA, eps_p=PR.EPS_P):
    tw = PC.twin(case, prio)
    assert rows["T"][0] == U.bits32(np.array([tw["T"]], f32))[0]
    for k, name in (("S", "S"), ("C", "C"), ("u", "u"), ("t", "t"), ("prio", "prio")):
        assert np.array_equal(rows[k], U.bits32(tw[name])), (k, case)
    assert np.array_equal(rows["idx"].view(np.int32), tw["idx"]), case
    b = case["batch"]
    # the two powers are library functions: held to the float64 evaluation (glibc's powf is correctly rounded to well under 1 ulp)
    w64 = PR.weights(case["ring_len"], tw["prio"][tw["slots"]], tw["T"], case["beta"], b, np.float64)
    w = rows["w"].view(f32)
    assert np.abs(w[:b] / w64[:b] - 1).max() < 4e-7 and not w[b:].any(), case
    if case["beta"] == 0.0:
        assert (w[:b] == 1).all()
    p64 = PR.new_priority(diff, eps_p, alpha, np.float64)
    assert np.abs(rows["pnew"].view(f32) / p64 - 1).max() < 2e-7
    return tw


def _diff(seed=0):
    d = np.random.default_rng(seed).normal(0, 3, PR.COLS).astype(f32)
    d[:3] = [0.0, -0.0, 1e-7]
    return d


def test_core_header_on_the_host_equals_the_twin_bit_for_bit(tmp_path):
    """tests/hostcheck/per_hostcheck.cpp, g++ -ffp-contract=off, on EVERY case the GPU test runs: u_m, t_m, every S_b / C_b, T, the
    slots and the freshly filled priorities equal the twin's bits; the weights and new priorities are held to float64.  The coverage
    conditions of every case are asserted here first."""
    exe = _hostcheck(tmp_path)
    dup = nodup = 0
    for name, case in PC.sampler_cases():
        prio = PC.build(case)
        tw = _assert_hostcheck_equals_the_twin(_run_hostcheck(exe, tmp_path, case, prio, _diff()), case, prio, _diff())
        PC.check_coverage(name, case, prio, tw)
        live = tw["idx"][:case["batch"]]
        dup += len(np.unique(live)) < len(live)
        nodup += len(np.unique(live)) == len(live) and len(live) > 1
    assert dup > 0 and nodup > 0
    lens = {c["ring_len"] for _, c in PC.sampler_cases()}
    assert {1, 255, 256, 257, 1000, 24000} <= lens and {c["batch"] for _, c in PC.sampler_cases()} == {1, 17, 120, 128}


def test_core_header_on_the_host_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: clean, and the same bits."""
    exe = _hostcheck(tmp_path, sanitize=True)
    cases = dict(PC.sampler_cases())
    for name in ("random-1of1-b1", "random-257of1000-b17", "last_block-1000", "fresh-wrap", "zeros-24000"):
        prio = PC.build(cases[name])
        _assert_hostcheck_equals_the_twin(_run_hostcheck(exe, tmp_path, cases[name], prio, _diff(1)), cases[name], prio, _diff(1))


def test_stream_and_sums():
    u = PR.uniforms(11, 3)
    for m in (0, 1, 77, 127):
        ref = DO.philox(m >> 2, 0, 3, 0x50455253, 11, 0)
        assert u[m] == f32(int(ref[m & 3]) >> 8) * f32(2.0 ** -24)
    assert PR.STREAM_PER not in (DO.STREAM_NOISE, DO.STREAM_SAMPLE, DO.STREAM_INIT, DO.STREAM_PERTURB, 0x5452474E)
    assert (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == 128
    # the tree: exact on integers, and NOT the left-to-right sum on values that round
    x = np.arange(64, dtype=f32)[None]
    assert PR.chunk_sums(x)[0] == 2016
    rng = np.random.default_rng(0)
    v = (rng.random((200, 64)) * 1e3).astype(f32)
    seq = np.add.accumulate(v, axis=1)[:, -1]
    tree = PR.chunk_sums(v)
    assert (tree != seq).any() and np.abs(tree / v.astype(np.float64).sum(1) - 1).max() < 1e-6
    S, Cc, T = PR.block_sums(np.ones(1000, f32), 1000)
    assert list(S) == [256, 256, 256, 232] and list(Cc) == [256, 512, 768, 1000] and T == 1000
    with open(os.path.join(U.ROOT, U.PKG_NAME, "csrc", "philox.h")) as f:
        assert "kStreamPer = 0x50455253u" in f.read()


def test_draw_frequencies_follow_the_priorities():
    """2 000 slots with a known pi, 4 000 ticks x 120 columns: each of 40 groups of 50 consecutive slots is drawn with frequency
    mass_g / T.  Bound: |count - n p| <= 2 binomial standard deviations sqrt(n p (1 - p)) per group.  Why 2: a group of consecutive
    slots covers whole strata (drawn with certainty) and at most two partial ones per tick, so its count has a variance of at most
    ticks / 2 = 2 000 (sd <= 44.7), against a binomial sd of 75 to 140 for these groups: 2 binomial sd are more than 3.3 sd of the
    stratified draw for every group, and a sampler that drew with replacement in the wrong proportions by 1 % of a group's mass
    (120 draws of 12 000) would be 0.9 to 1.6 binomial sd off already.  Worst ratio observed on the twin: 0.54."""
    rng = np.random.default_rng(5)
    n, batch, ticks = 2000, 120, 4000
    prio = (rng.random(n) ** 2 * 3 + 0.01).astype(f32)
    S, Cc, T = PR.block_sums(prio, n)
    run = np.concatenate([np.add.accumulate(np.concatenate(([Cc[b - 1] if b else f32(0)], prio[b * 256:(b + 1) * 256])).astype(f32))[1:]
                          for b in range(len(Cc))])
    counts = np.zeros(n, np.int64)
    for tick in range(ticks):
        t = PR.targets(PR.uniforms(7, tick), T, batch)[:batch]
        j = np.minimum(np.searchsorted(run, t, side="right"), n - 1)       # first slot whose running sum exceeds t
        np.add.at(counts, j, 1)
    # the vectorised search is the twin's search
    t = PR.targets(PR.uniforms(7, 5), T, batch)
    assert [PR.search(prio, S, Cc, t[m], n) for m in range(batch)] == list(np.minimum(np.searchsorted(run, t[:batch], side="right"), n - 1))
    N = ticks * batch
    g = counts.reshape(40, 50).sum(1)
    p = prio.astype(np.float64).reshape(40, 50).sum(1) / prio.astype(np.float64).sum()
    ratio = np.abs(g - N * p) / np.sqrt(N * p * (1 - p))
    print("worst |count - n p| / sigma over the 40 slot groups:", ratio.max())
    assert ratio.max() < 2.0


def test_alpha_zero_gives_every_live_slot_equal_mass():
    """alpha = 0: every written priority is (|diff| + eps)^0 = 1, so a ring of such priorities is drawn uniformly (stratified) and
    every weight is 1."""
    pn = PR.new_priority(np.array([0.0, 3.0, -1e-3, 1e6], f32), 1e-6, 0.0)
    assert (pn == 1).all()
    n, batch = 1000, 120
    prio = np.ones(n, f32)
    d = PR.sample(prio, 1.0, n, n, 0, 0, 3, 9, batch, 0.4)
    assert d["T"] == n and (d["w"][:batch] == 1).all()
    seg = n / batch
    assert all(int(m * seg) <= d["idx"][m] <= int((m + 1) * seg) for m in range(batch))


def test_weighted_head_and_write_back_on_the_twin():
    rng = np.random.default_rng(2)
    n, batch = 400, 24
    pa, pc = DO.init_params(3, 9, 2, 0), DO.init_params(3, 11, 1, 1)
    s, s2 = (rng.random((n, 9)) * 5).astype(f32), (rng.random((n, 9)) * 5).astype(f32)
    a, r, done = (rng.random((n, 2)) * 2 - 1).astype(f32), rng.normal(-1, 2, n).astype(f32), rng.random(n) < 0.05
    idx = DO.sample_indices(3, 1, batch, n)
    b = [x[idx] for x in (s, a, r, s2, done)]
    L, P = DO.Learner(pa, pc, s.min(0), s.max(0)), PR.PerLearner(pa, pc, s.min(0), s.max(0))
    lc, la = L.replay(*b)
    lcw, law, diff = P.replay_w(*b, np.ones(batch, f32))
    assert np.array_equal(L.critic, P.critic) and np.array_equal(L.actor, P.actor) and abs(lc - lcw) < 1e-6 * abs(lc) and la == law
    P2 = PR.PerLearner(pa, pc, s.min(0), s.max(0))
    P2.replay_w(*b, np.full(batch, 0.5, f32))
    assert not np.array_equal(P2.critic, P.critic)
    prio = np.ones(n, f32)
    slots = np.array([5, 9, 5, 7], np.int64)
    pm = PR.write_back(prio, 1.0, slots, np.array([1.0, 2.0, 3.0, 0.0], f32), 1e-6, 0.6)
    assert prio[5] == PR.new_priority(f32(3.0), 1e-6, 0.6) and prio[7] == PR.new_priority(f32(0.0), 1e-6, 0.6) and pm == max(1.0, prio[5])
    assert PR.write_back(prio, 9.0, slots, np.zeros(4, f32), 1e-6, 0.6) == 9.0


def test_update_cases_cover_what_they_are_there_for():
    """The rings of the GPU update tests (tests/per_cases.py:update_cases), on the twin at the tick the GPU test uses: four decades of
    priorities and a spread of weights on the 24 000-slot ring with no slot drawn twice; on the 1 000-slot ring with five heavy slots
    some columns share a slot and others do not, and the highest column is the twin's writer."""
    for name, cap, batch, kind, want_dup in PC.update_cases():
        prio = PC.update_priorities(kind, cap)
        tw = PR.sample(prio.copy(), 1.0, cap, cap, 0, 0, PC.UPDATE_SEED, 3, batch, 0.4)
        live = tw["idx"][:batch]
        uniq, counts = np.unique(live, return_counts=True)
        if kind == "decades":
            assert prio.max() / prio.min() >= 1e4, name
        if batch > 1:
            assert tw["w"][:batch].min() < 0.5 and tw["w"][:batch].max() == 1, name
        if want_dup:
            assert (counts > 1).sum() >= 3 and (counts == 1).sum() >= 20, (name, counts)
            p = prio.copy()
            diff = np.arange(batch, dtype=f32) + 1                      # distinct candidates: the highest column's must land
            PR.write_back(p, 1.0, live.astype(np.int64), diff, PR.EPS_P, PR.ALPHA)
            for slot in uniq:
                assert p[slot] == PR.new_priority(diff[np.nonzero(live == slot)[0].max()], PR.EPS_P, PR.ALPHA), (name, slot)
        else:
            assert (counts == 1).all(), (name, counts)


_C_TO_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}


def test_per_prototypes_match_the_header():
    """Every prototype of _capi._per_sigs against its declaration in include/shems_hip.h, argument by argument: scalars by width,
    `shems_per *` / `shems_replay *` by their mirrors, every other pointer as a pointer."""
    S = U.pkg()
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()
    for name, args in S._capi._per_sigs().items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        decl = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(decl) == len(args), (name, decl)
        for d, a in zip(decl, args):
            if "*" in d:
                base = d.replace("const", "").split("*")[0].strip()
                want = {"shems_per": (C.POINTER(S._capi.PerArgs),), "shems_replay": (C.POINTER(S._capi.Replay),),
                        "int64_t": (C.POINTER(C.c_int64), C.c_void_p)}.get(base, (C.c_void_p,))
                assert a in want, (name, d, a)
            else:
                assert a is _C_TO_CTYPES[d.split()[0]], (name, d, a)


def test_per_record_matches_the_c_struct(tmp_path):
    R = importlib.import_module(U.PKG_NAME + ".replay")
    names = [f[0] for f in R.PerArgs._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shems_hip.h"\nint main(void){printf("%zu", sizeof(shems_per));' +
                   "".join(f'printf(" %zu", offsetof(shems_per, {n}));' for n in names) + 'return 0;}\n')
    exe = tmp_path / "o"
    subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(R.PerArgs) == 40
    assert vals[1:] == [getattr(R.PerArgs, n).offset for n in names]
    assert (R.PW_T, R.PW_IDX, R.PW_W, R.PW_U, R.PW_TM, R.PW_S) == (PR.PW_T, PR.PW_IDX, PR.PW_W, PR.PW_U, PR.PW_TM, PR.PW_S)
    hdr = open(os.path.join(U.ROOT, U.PKG_NAME, "csrc", "shems_per_core.h")).read()
    assert "PW_IDX = 4" in hdr and "kPerMaxSlots = 262144" in hdr and R.PER_MAX_SLOTS == 262144


def test_per_entry_points_are_exported(built_lib):
    S = U.pkg()
    want = {"shems_per_workspace_floats", "shems_per_sample_dev", "shems_ddpg_update_given", "shems_ddpg_update_per"}
    assert want <= set(S._capi.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib]).decode()
    assert want <= set(re.findall(r" T (shems_[a-z0-9_]+)", out))
    R = importlib.import_module(U.PKG_NAME + ".replay")
    for cap in (1, 256, 257, 1000, 24000, 262144):
        assert R.per_workspace_floats(cap) == PR.ws_floats(cap)
    with pytest.raises(S._capi.ShemsError):
        R.per_workspace_floats(262145)


def test_anneal_beta():
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    assert [D.anneal_beta(0.4, i - 1, 3) for i in (1, 4)] == [0.4, 1.0]      # run_episodes(num_ep = 4): episode 1 and the last
    assert D.anneal_beta(0.4, 0, 100) == 0.4 and D.anneal_beta(0.4, 100, 100) == 1.0 and D.anneal_beta(0.4, 250, 100) == 1.0
    assert abs(D.anneal_beta(0.4, 50, 100) - 0.7) < 1e-15 and D.anneal_beta(1.0, 3, 10) == 1.0
    for bad in ((-0.1, 0, 10), (1.1, 0, 10), (0.4, -1, 10), (0.4, 0, 0)):
        with pytest.raises(ValueError):
            D.anneal_beta(*bad)


def test_shems_replay_parser():
    M = importlib.import_module(U.PKG_NAME + ".main")
    assert M.parse_replay(None) == ("uniform", None) and M.parse_replay("uniform") == ("uniform", None)
    assert M.replay_from_env({}) == ("uniform", None)
    assert M.parse_replay("per") == ("per", dict(alpha=0.6, beta0=0.4))
    assert M.parse_replay("per:0.7") == ("per", dict(alpha=0.7, beta0=0.4))
    assert M.replay_from_env({"SHEMS_REPLAY": "per:0:1"}) == ("per", dict(alpha=0.0, beta0=1.0))
    for bad in ("PER", "rank", "per:", "per:a", "per:-0.1", "per:0.6:1.5", "per:0.6:-0.1", "per:nan", "per:0.6:0.4:1", ""):
        with pytest.raises(ValueError) as ei:
            M.parse_replay(bad)
        assert "SHEMS_REPLAY" in str(ei.value) and repr(bad) in str(ei.value)
    c = M.config_from_env({"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0"})
    base = c.case
    c.algo_suffix += M.replay_case_suffix(alpha=0.6, beta0=0.4)
    assert c.case == base + "_per-a0.6-b0.4"


class _FakeSync:
    world = 1
    native = None


def _bare_agent(D, **kw):
    """An Agent object without its device state: the refusals come before any device work."""
    ag = object.__new__(D.Agent)
    ag.__dict__.update(dict(batch=120, wide=False, hidden=(D.L1, D.L2), noise_type="gn", sync=_FakeSync(), tiled_mode=False, fused=True,
                            device=None))
    ag.__dict__.update(kw)
    ag._same_device = lambda *a: None
    return ag


def _bare_ring(R):
    ring = object.__new__(R.PrioritizedRing)
    ring.capacity, ring.pushed, ring.covered = 1000, 1000, 0
    return ring


def test_python_level_refusals():
    """Everything the prioritized update does not cover is refused by name before any device work, never run as the uniform update."""
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    R = importlib.import_module(U.PKG_NAME + ".replay")
    T = importlib.import_module(U.PKG_NAME + ".td3")
    ring = _bare_ring(R)
    for kw, call, word in ((dict(), dict(exclude=(0, 10)), "exclude"), (dict(), dict(publish=object()), "publish"),
                           (dict(batch=150), {}, "BATCH_SIZE"), (dict(wide=True), {}, "layer by layer"), (dict(hidden=(300, 600)), {}, "layer by layer"),
                           (dict(noise_type="pn"), {}, "parameter noise"), (dict(tiled_mode=True), {}, "tiled"),
                           (dict(_before_param_write=lambda: None), {}, "learner group")):
        with pytest.raises(NotImplementedError) as ei:
            _bare_agent(D, **kw).replay(ring, **call)
        assert "prioritized replay" in str(ei.value) and word in str(ei.value), (kw, call, str(ei.value))
    two = _FakeSync()
    two.world = 2
    with pytest.raises(NotImplementedError, match="data-parallel"):
        _bare_agent(D, sync=two).replay(ring)
    with pytest.raises(NotImplementedError, match="clone.*PrioritizedRing"):
        _bare_agent(D).clone(ring)
    with pytest.raises(NotImplementedError, match="evaluate.*PrioritizedRing"):
        _bare_agent(D).evaluate(ring)
    td3 = object.__new__(T.TD3Agent)
    with pytest.raises(NotImplementedError, match="TD3.*PrioritizedRing"):
        td3.replay(ring)
    with pytest.raises(NotImplementedError, match="TD3.*replay_given"):
        td3.replay_given(ring, None, None)
    with pytest.raises(NotImplementedError, match="replay_given"):
        _bare_agent(D, fused=False).replay_given(ring, None, None)
    for bad in (dict(alpha=-0.1), dict(beta=1.5), dict(eps=float("nan")), dict(beta=float("inf"))):
        with pytest.raises(ValueError):
            R.PrioritizedRing(16, **bad)
    ring.pushed, ring.covered = 1030, 990
    assert ring.fresh_range() == (990, 40)
    ring.pushed, ring.covered = 5000, 100
    assert ring.fresh_range() == (100, 1000)
    ring.covered = 5000
    assert ring.fresh_range() == (0, 0)


def test_slab_layouts_are_unchanged(built_lib):
    """The learner's arguments and a learner group's slab keep their sizes and offsets (the figures of the commit before prioritized
    replay): the priorities live in the ring's own arrays."""
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    G = importlib.import_module(U.PKG_NAME + ".group")
    ws = C.c_int64()
    assert D._declare().shems_ddpg_workspace_floats(C.byref(ws)) == 0 and ws.value == 1902568
    for tiled, floats, ring_done, ws_off in ((False, 3702636, 3696636, 1290068), (True, 4751212, 4745212, 2338644)):
        lay, n = G.slab_layout(D.N_ACTOR, D.N_CRITIC, ws.value, 24000, tiled)
        assert n == floats and lay["ring_done"] == (ring_done, 6000) and lay["ws"] == (ws_off, ws.value)
        assert not any("prio" in k or "pmax" in k for k in lay)
    assert "prio" not in [f[0] for f in D.DdpgArgs._fields_] and C.sizeof(D.DdpgArgs) == 128

"""The horizon of ADAM's beta powers and the elementwise tail of every update (csrc/shems_adam.h) on the CPU.

The powers are host state, multiplied by 0.9 and 0.999 after every update with no clamp, and every entry point refuses a power outside
the open interval (0, 1).  What these tests found, so that nobody has to redo the arithmetic:
  * 0.9^t (update t receives [0.9, 0.999] advanced t - 1 times) is a subnormal double from update 6 724 on and STICKS at 5 units of the
    smallest subnormal (2.5e-323) from update 7 050 on: 5 x 0.9 = 4.5000000000000001 rounds back to 5 (0.9 as a double lies above 0.9).
    It never reaches 0.0, so the refusal cannot fire in a run of any length.
  * 0.999^t is 4.83e-32 at update 72 072 (a thesis run), subnormal after about 709 000 updates, and sticks at 499 units (2.465e-321).
  * 1 - bp1 == 1.0 exactly from update 356 on and 1 - bp2 == 1.0 from update 37 412 on: eta / (1 - bp1) and 1 / (1 - bp2) are then eta
    and 1 to the last bit.
The real objects (Agent, TD3Agent, LearnerGroup._advance_learners, with the native library stubbed out) and C doubles advanced the way
the native loop's record advances them follow the plain product bit for bit."""
import ctypes as C
import importlib
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

import adam_cases as K
import adam_ref as AR
import util as U

f32, f64 = np.float32, np.float64
SMALLEST = 2.0 ** -1074


# ------------------------------------------------------------------------------------------------------------- 1. the plain product --
def test_the_powers_stay_inside_the_open_interval_for_a_whole_run_and_beyond():
    b1, first_subnormal, settled = 0.9, None, None
    for t in range(1, K.HORIZON + 1):                         # b1 is what update t receives
        assert 0.0 < b1 < 1.0, t
        if first_subnormal is None and b1 < sys.float_info.min:
            first_subnormal = t
        nxt = b1 * 0.9
        if settled is None and nxt == b1:
            settled = t
        b1 = nxt
    assert (first_subnormal, settled) == (6724, 7050)
    assert b1 == K.SETTLED_BP1 == 5 * SMALLEST and b1 * 0.9 == b1
    assert K.powers(7000)[0] == 1009 * SMALLEST and K.powers(K.THESIS_UPDATES) == (K.SETTLED_BP1, 4.829113612666865e-32)
    b2, settled2, first_sub2 = 0.999, None, None
    for t in range(1, 1_000_001):
        assert 0.0 < b2 < 1.0, t
        if first_sub2 is None and b2 < sys.float_info.min:
            first_sub2 = t
        nxt = b2 * 0.999
        if settled2 is None and nxt == b2:
            settled2 = t
        b2 = nxt
    assert b2 == 499 * SMALLEST and b2 * 0.999 == b2 and 700_000 < first_sub2 < settled2 < 1_000_000, (b2 / SMALLEST, first_sub2, settled2)
    # the table the cases are cut from is this product
    tab = K._power_table()
    assert tab[0] == (0.9, 0.999) and tab[1] == (0.9 * 0.9, 0.999 * 0.999) and len(tab) == K.HORIZON
    assert all(0.0 < x < 1.0 and 0.0 < y < 1.0 for x, y in tab)
    # where the factors become 1 to the last bit
    one1 = next(t for t, (x, _) in enumerate(tab, 1) if 1.0 - x == 1.0)
    one2 = next(t for t, (_, y) in enumerate(tab, 1) if 1.0 - y == 1.0)
    assert (one1, one2) == (356, 37412), (one1, one2)
    for step in (7000, K.THESIS_UPDATES):
        x, y = K.powers(step)
        assert 1e-3 / (1.0 - x) == 1e-3 and (1.0 / (1.0 - y) == 1.0) == (step == K.THESIS_UPDATES)


def test_the_tuned_grid_spans_the_etas_the_cases_use():
    G = importlib.import_module(U.PKG_NAME + ".group")
    recs, _, _ = G.tuned_grid(range(81), wide=True)
    etas = {r["eta_act"] for r in recs} | {r["eta_crit"] for r in recs}
    assert (min(etas), max(etas)) == (K.ETA_MIN, K.ETA_MAX) and {K.ETA_ACT, K.ETA_CRIT} <= etas
    assert {r["tau"] for r in recs} == {K.TAU}


# ------------------------------------------------------------------------------------------------------------ 2. the real objects --
class _FakeLib:
    """Every native entry point: returns SHEMS_OK, launches nothing."""
    def __getattr__(self, name):
        if not name.startswith("shems_"):
            raise AttributeError(name)
        return lambda *a: 0


class _Sync:
    world, native, grad_scale = 1, None, 1.0

    def sum_(self, g):
        pass


class _Ring:
    capacity = pushed = covered = 1000

    def __len__(self):
        return 1000

    def struct(self):
        return C.c_int64(0)

    per_struct = struct

    def fresh_range(self):
        return 0, 0


class _Buf:
    def data_ptr(self):
        return 0

    def __getitem__(self, k):
        return self


def _bare(cls, D, **kw):
    ag = object.__new__(cls)
    ag.__dict__.update(dict(L=_FakeLib(), batch=120, wide=False, hidden=(D.L1, D.L2), whidden=(D.L1, D.L2), noise_type="gn", sync=_Sync(),
                            tiled_mode=False, _tiled_current=False, fused=True, device=None, rng_seed=1, eta_act=1e-4, eta_crit=1e-3,
                            bp_actor=[0.9, 0.999], bp_critic=[0.9, 0.999], updates=0, clones=0, evaluations=0, n_step=1, dp_overlap=False,
                            policy_delay=2, grad_actor=_Buf(), grad_critic=_Buf(), losses=_Buf(), ws=_Buf(), n_actor=1, n_critic=1))
    ag.__dict__.update(kw)
    ag._same_device = lambda *a: None
    ag._stream = lambda: None
    ag._enter_tiled = lambda: False
    ag._ddpg_args = lambda *a, **k: D.DdpgArgs()
    return ag


def _follow(call, ag, steps, critic, actor):
    """call() `steps` times; critic / actor: update number -> does that network's power advance.  Before every call both powers are the
    plain product of the advances so far, inside (0, 1)."""
    tab = K._power_table()
    kc = ka = 0
    for t in range(steps):
        assert ag.bp_critic == list(tab[kc]) and ag.bp_actor == list(tab[ka]), (t, kc, ka, ag.bp_critic, ag.bp_actor)
        call()
        kc += bool(critic(t))
        ka += bool(actor(t))
    assert ag.bp_critic == list(tab[kc]) and ag.bp_actor == list(tab[ka])
    return kc, ka


@pytest.fixture()
def mods(monkeypatch):
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    T = importlib.import_module(U.PKG_NAME + ".td3")
    G = importlib.import_module(U.PKG_NAME + ".group")
    fake = _FakeLib()
    monkeypatch.setattr(D, "_declare_per", lambda: fake)
    return D, T, G


STEPS = K.HORIZON - 1                       # the table holds the powers of updates 1 .. HORIZON


def test_agent_bookkeeping_follows_the_plain_product(mods):
    D, T, G = mods
    torch = pytest.importorskip("torch")
    ring, yes, no = _Ring(), (lambda t: True), (lambda t: False)
    per = object.__new__(importlib.import_module(U.PKG_NAME + ".replay").PrioritizedRing)
    per.__dict__.update(capacity=1000, pushed=1000, covered=0, struct=ring.struct, per_struct=ring.struct, fresh_range=ring.fresh_range)
    idx, w = torch.zeros(128, dtype=torch.int32), torch.ones(128, dtype=torch.float32)
    two = _Sync()
    two.world, two.native = 2, object()
    subs = [dict(batch=75, ga=_Buf(), gc=_Buf(), ws=_Buf(), losses=_Buf()) for _ in range(2)]
    forms = (("replay, one call", {}, lambda a: a.replay(ring), yes, yes),
             ("replay, split calls", dict(fused=False), lambda a: a.replay(ring), yes, yes),
             ("replay, wide path", dict(wide=True), lambda a: a.replay(ring), yes, yes),
             ("replay, native data-parallel call", dict(sync=two), lambda a: a.replay(ring), yes, yes),
             ("replay, sub-batches", dict(batch=150, sub_batches=lambda: subs), lambda a: a.replay(ring), yes, yes),
             ("replay, prioritized ring", dict(torch=torch), lambda a: a.replay(per), yes, yes),
             ("replay_given", dict(torch=torch), lambda a: a.replay_given(ring, idx, w), yes, yes),
             ("clone", {}, lambda a: a.clone(ring), no, yes),
             ("evaluate", {}, lambda a: a.evaluate(ring), yes, no))
    for what, kw, call, critic, actor in forms:
        ag = _bare(D.Agent, D, **kw)
        steps = STEPS if what in ("replay, one call", "clone", "evaluate") else 8000      # (0.9^t has settled by update 7 050)
        kc, ka = _follow(lambda: call(ag), ag, steps, critic, actor)
        assert (kc, ka) == (steps * critic(0), steps * actor(0)), what
        assert ag.updates + ag.clones + ag.evaluations == steps, what
        for bp in (ag.bp_critic, ag.bp_actor):
            assert bp[0] in (0.9, K.SETTLED_BP1) and 0.0 < bp[1] < 1.0, what


def test_td3_agent_advances_the_actor_on_policy_steps_only(mods):
    D, T, G = mods
    ag = _bare(T.TD3Agent, D)
    ag._td3_args = lambda: T.Td3Args()
    policy = lambda t: T.is_policy_step(t, 2)
    kc, ka = _follow(lambda: ag.replay(_Ring()), ag, STEPS, lambda t: True, policy)
    assert (kc, ka) == (STEPS, STEPS // 2) and ag.updates == STEPS
    assert ag.bp_actor[0] == ag.bp_critic[0] == K.SETTLED_BP1 and ag.bp_actor[1] > ag.bp_critic[1] > 0.0
    forced = _bare(T.TD3Agent, D)
    forced._td3_args = lambda: T.Td3Args()
    _follow(lambda: forced.replay(_Ring(), update_policy=False), forced, 100, lambda t: True, lambda t: False)
    assert forced.bp_actor == [0.9, 0.999]


def test_group_advance_follows_the_plain_product(mods):
    D, T, G = mods
    mk = lambda: types.SimpleNamespace(bp_actor=[0.9, 0.999], bp_critic=[0.9, 0.999], updates=0, clones=0, evaluations=0)
    grp = types.SimpleNamespace(learners=[mk(), mk(), mk()])
    adv = G.LearnerGroup._advance_learners
    for what, kw, critic, actor in (("updates", dict(critic=True, actor=True, counter="updates"), True, True),
                                    ("clones", dict(critic=False, actor=True, counter="clones"), False, True),
                                    ("evaluations", dict(critic=True, actor=False, counter="evaluations"), True, False)):
        grp.learners = [mk(), mk(), mk()]
        _follow(lambda: adv(grp, **kw), grp.learners[0], STEPS, lambda t: critic, lambda t: actor)
        for ag in grp.learners:                                # in lockstep
            assert ag.bp_critic == grp.learners[0].bp_critic and ag.bp_actor == grp.learners[0].bp_actor and getattr(ag, what) == STEPS


# --------------------------------------------------------------------------------------------------- 3. csrc/shems_adam.h on the host --
def _hostcheck(tmp_path, sanitize=False):
    exe = str(tmp_path / ("adam_hostcheck_san" if sanitize else "adam_hostcheck"))
    d = os.path.join(U.ROOT, "tests", "hostcheck")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", "-I" + os.path.join(d, "hip_host")] +
                          (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) +
                          ["-o", exe, os.path.join(d, "adam_hostcheck.cpp")])
    return exe


def test_c_doubles_advance_like_the_python_floats(tmp_path):
    """The native loop's record (csrc/shems_train.hip: bpc[0] *= 0.9; bpc[1] *= 0.999; after every update) needs a device to run; the same
    statements on C doubles, in the stand-alone program."""
    exe = _hostcheck(tmp_path)
    out = subprocess.run([exe, "horizon", str(K.HORIZON)] + [str(s) for s in K.BP_STEPS], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {(w[0], int(w[1])): int(w[2], 16) for w in (l.split() for l in out) if len(w) == 3 and w[0] in ("bp1", "bp2")}
    for s in K.BP_STEPS:
        b1, b2 = K.powers(s)
        assert got[("bp1", s)] == struct.unpack("<Q", struct.pack("<d", b1))[0] and got[("bp2", s)] == struct.unpack("<Q", struct.pack("<d", b2))[0], s
    assert "subnormal 6724" in out and "settled 7050 0000000000000005" in out and "zero 0" in out


def _run(exe, tmp_path, case, n):
    src, dst = str(tmp_path / "adam_in.bin"), str(tmp_path / "adam_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qddddf", n, case["eta"], case["bp"][0], case["bp"][1], 1.0, case["tau"]))
        for a in case["old"] + (case["g"],):
            f.write(np.ascontiguousarray(a[:n], f32).tobytes())
    out = subprocess.run([exe, src, dst], check=True, capture_output=True, text=True).stdout
    got = np.fromfile(dst, f32).reshape(4, n)
    ld = {w[1]: (float(w[3]), int(w[5])) for w in (l.split() for l in out.split("\n")) if len(w) == 6 and w[0] == "longdouble"}
    return tuple(got), ld


def _check_host(exe, tmp_path, names, n):
    acc = {}
    for critic in (True, False):
        for name in names:
            case = K.apply_case(critic, name)
            got, ld = _run(exe, tmp_path, case, n)
            errs = AR.all_errors([a[:n] for a in case["old"]], got, [a[:n] for a in case["ref"]])
            AR.worst(acc, errs)
            AR.assert_within_bounds(errs, (critic, name))
            # against long double: m and v within one ulp of the operands' resolution (where m and g cancel, long double keeps bits of the
            # sum that the definition's Float64 does not), the step a quotient refined to an ulp of Float64
            assert ld["m"][0] <= 1 and ld["v"][0] <= 1 and ld["p"][0] <= 1 and ld["target"][0] <= 1, (critic, name, ld)
            if case["tau"] == 0.0:
                assert np.array_equal(got[3].view(np.uint32), case["old"][3][:n].view(np.uint32))
            if case["tau"] == 1.0:
                assert np.array_equal(got[3].view(np.uint32), got[0].view(np.uint32))
    return acc


def test_header_on_the_host_meets_the_reference_and_long_double(tmp_path):
    """tests/hostcheck/adam_hostcheck.cpp runs csrc/shems_adam.h's adam_math itself (the reciprocal estimate replaced by a worse one) over
    every case of the apply entry points."""
    names = [c[0] for c in K.apply_cases(True)]
    assert names == [c[0] for c in K.apply_cases(False)] and len(names) == 13
    acc = _check_host(_hostcheck(tmp_path), tmp_path, names, 129_002)
    print("adam_math on the host, worst over all cases:", acc)


def test_header_on_the_host_under_address_and_undefined_sanitizers(tmp_path):
    acc = _check_host(_hostcheck(tmp_path, sanitize=True), tmp_path, ["step1", "step72072", "step72072-tau1", "step100-eta-max"], 16_387)
    assert acc["p"]["n_rel"] > 0


# ----------------------------------------------------------------------------------------------------------- 4. where the bounds come from --
def test_the_bounds_are_four_times_the_fp32_twin():
    """N and R of tests/test_adam_edges_gpu.py: the plain fp32 twin (tests/adam_ref.py:twin) over every case of the apply entry points
    against the float64 reference, the worst value times 4 (the project's convention, tests/test_ddpg_gpu.py:57-62), rounded UP to two
    digits.  The figures are quoted in profiles/adam_edges_errors.txt."""
    acc, plain = {}, {}
    for critic in (True, False):
        blocks = [(lo, hi) for _, lo, hi in AR.DO.blocks(11 if critic else 9, 1 if critic else 2)]
        for name, *_ in K.apply_cases(critic):
            case = K.apply_case(critic, name)
            K.assert_not_vacuous(case, blocks)
            AR.worst(acc, AR.all_errors(case["old"], AR.twin(*case["old"], case["g"], case["eta"], case["tau"], *case["bp"]), case["ref"]))
            AR.worst(plain, AR.all_errors(case["old"], AR.twin(*case["old"], case["g"], case["eta"], case["tau"], *case["bp"], moments="fp32"), case["ref"]))
    print("fp32 twin (Float64 moment statements), worst:", acc)
    print("fp32 twin (fp32 moment statements), worst:", plain)
    for name in AR.NAMES:
        for k in ("ulp", "rel", "rel_resolved"):
            bound, w = AR.BOUNDS[name][k], acc[name][k]
            assert 4 * w <= bound <= 4 * w * 1.05 + 1e-300, (name, k, w, bound)
        assert acc[name]["n_resolved"] > 100_000 or name == "target"
    # plain fp32 moments are no yardstick for the step: cancellation in m1
    assert plain["p"]["rel_resolved"] > 10 and plain["m"]["ulp"] <= 2 and plain["v"]["ulp"] <= 2


# --------------------------------------------------------------------------------- 5. the throughput entry points accept the settled power --
def test_throughput_entry_points_accept_the_settled_power_on_the_host(built_lib):
    """tests/test_group_tp_checks_host.py:79-80 hold the refusals of 0.0, 1.0 and NaN.  The accepted side: the beta-power check is the
    last but one of check_tp (the tiled regions follow it), so a call whose ONLY other fault is a region is refused for the region when
    the powers pass and for the powers when they do not."""
    import test_group_tp_checks_host as TPC
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    D, G, T = mod("ddpg"), mod("group"), mod("td3")
    L = T._declare_group()
    assert S._capi.declare_group_per() is L
    env = (S, D, G, T, L, TPC.Blocks())
    rows, valid = TPC._table(D, G, env[5])
    region = dict(t=G.GroupW2T(env[5].ta, None))
    late = dict(enumerate((K.SETTLED_BP1, K.powers(K.THESIS_UPDATES)[1], K.SETTLED_BP1, K.powers(K.THESIS_UPDATES)[1])))
    for name in TPC.ENTRY:
        for bp, word in ((late, "both regions"), (dict(enumerate((SMALLEST, 499 * SMALLEST, SMALLEST, 499 * SMALLEST))), "both regions"),
                         ({**late, 0: 0.0, 2: 0.0}, "beta powers")):
            rc, msg = TPC._call(env, name, {**valid, **region, "bp": bp})
            assert rc == S._capi.ERR_ARG and name in msg and word in msg, (name, bp, rc, msg)
    assert not env[5].raw.any()

"""The behaviour-regularised actor loss (TD3+BC) without a GPU: the NumPy twin (tests/bc_ref.py) against a float64 finite difference of
loss_act, a host build of csrc/shems_bc_core.h against the twin bit for bit, the C struct and prototypes, the exports, the BC value
class, the SHEMS_BC / SHEMS_FORESIGHT_OFFLINE parsers and the refusals of imitation.offline."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

import bc_ref as BR
import ddpg_oracle as DO
import util as U

f32 = np.float32


def _D():
    return importlib.import_module(U.PKG_NAME + ".ddpg")


def _case(seed=11, n=400, batch=24):
    rng = np.random.default_rng(seed)
    pa, pc = DO.init_params(seed, 9, 2, 0), DO.init_params(seed, 11, 1, 1)
    pc[128250:128750] *= 30.0
    pa[128000:129000] *= 30.0
    s = rng.random((n, 9)).astype(f32) * 5
    a = (rng.random((n, 2)) * 2 - 1).astype(f32)
    L = DO.Learner(pa, pc, s.min(0), s.max(0))
    idx = DO.sample_indices(seed, 3, batch, n)
    return L, s[idx], a[idx]


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,weight", [(2.5, 1.0), (0.0, 1.0), (1.0, 0.0), (2.5, 0.25)])
def test_twin_gradient_is_the_finite_difference_of_the_loss_with_lambda_held(alpha, weight):
    """d loss_act / d theta by central differences in float64, lambda a constant: the twin's gradient is that derivative.  A relu
    that a probe carries across zero would put a kink inside a difference: a step h of one parameter moves a pre-activation by at most
    h times the largest input of its layer (and less downstream: |W| < 1), which is asserted to stay 10 times below the smallest
    pre-activation of the case."""
    L, s, a = _case()
    _, q, _, _ = BR.actor_parts(L, s, a)
    lam = float(BR.lam(alpha, BR.q_abs_mean(q, np.float64), True))
    g, loss, _, nmq, mse = BR.actor_grad(L, s, a, lam, weight)
    assert abs(loss - BR.loss_of(L, L.actor.astype(np.float64), s, a, lam, weight)) < 1e-12 * max(1.0, abs(loss))
    assert abs(loss - (lam * nmq + weight * mse)) < 1e-12
    sn = DO.normalize(s, L.s_min, L.s_max)
    _, (_, z1, h1, z2, _, _) = DO.mlp_forward(L.actor, sn, 9, 2, True, keep=True, dtype=np.float64)
    h = 1e-7
    rng = np.random.default_rng(0)
    blocks = dict((n, (lo, hi)) for n, lo, hi in DO.blocks(9, 2))
    probes = list(range(*blocks["b3"])) + [int(x) for x in rng.integers(*blocks["W3"], 6)] + [int(x) for x in rng.integers(*blocks["b2"], 4)] + \
        [int(x) for x in rng.integers(*blocks["W2"], 4)] + [int(x) for x in rng.integers(*blocks["b1"], 3)]
    assert np.abs(L.actor[:blocks["W3"][0]]).max() < 1
    assert min(np.abs(z1).min(), np.abs(z2).min()) > 10 * h * max(1.0, float(np.abs(sn).max()), float(h1.max())), "a relu sits inside the difference step"
    checked = 0
    for i in probes:
        p = L.actor.astype(np.float64)
        p[i] += h
        up = BR.loss_of(L, p, s, a, lam, weight)
        p[i] -= 2 * h
        fd = (up - BR.loss_of(L, p, s, a, lam, weight)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])) + 1e-9, (i, fd, g[i])
        checked += 1
    assert checked == len(probes) and np.abs(g[list(probes)]).max() > 0


def test_twin_special_cases():
    """weight = 0, lambda = 1: the DDPG oracle's actor gradient; alpha = 0: the cloning gradient, nothing of lambda or q."""
    L, s, a = _case()
    g0, _ = L.actor_grad(s, dtype=np.float64)
    g1, loss, (t_q, t_bc), nmq, mse = BR.actor_grad(L, s, a, 1.0, 0.0)
    assert np.array_equal(g0, g1) and loss == nmq and not t_bc.any()
    g2, loss2, (t_q2, _), _, mse2 = BR.actor_grad(L, s, a, 0.0, 1.0)
    assert not t_q2.any() and loss2 == mse2 > 0
    sn = DO.normalize(s, L.s_min, L.s_max)
    a_pi, ca = DO.mlp_forward(L.actor, sn, 9, 2, True, keep=True, dtype=np.float64)
    gc, _ = DO.mlp_backward(L.actor, ca, (a_pi - a) / len(s), 9, 2, True, dtype=np.float64)
    assert np.array_equal(g2, gc)
    # the floor, and a plain alpha
    assert BR.lam(2.5, 0.0, True) == f32(2.5) / f32(1e-8) and BR.lam(2.5, 0.0, False) == f32(2.5) and BR.lam(2.5, np.nan, True) == f32(2.5) / f32(1e-8)
    assert BR.lam(2.5, 0.5, True) == f32(5.0) and BR.lam(0.0, 0.5, True) == 0.0


# ---- the core header on the host ---------------------------------------------------------------------------------------------------------
def _hostcheck(tmp_path, sanitize=False):
    exe = str(tmp_path / ("bc_hostcheck_san" if sanitize else "bc_hostcheck"))
    src = os.path.join(U.ROOT, "tests", "hostcheck", "bc_hostcheck.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas"] +
                          (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + ["-o", exe, src])
    return exe


def _hostcheck_inputs(n=300, alpha=2.5, weight=1.0, normalise=1, batch=120):
    rng = np.random.default_rng(4)
    qbar = np.abs(rng.normal(0, 0.05, n)).astype(f32)
    qbar[:6] = [0.0, 1e-8, 1.000001e-8, 9.9999999e-9, 1e-30, 3.0e38]     # the floor from both sides, a subnormal quotient's neighbour
    da = rng.normal(0, 1e-2, n).astype(f32)
    diff = (np.tanh(rng.normal(0, 2, n)) - (rng.random(n) * 2 - 1)).astype(f32)
    da[6:9] = [0.0, -0.0, 1e-30]
    diff[9:12] = [0.0, -0.0, 2.0]
    nmq = rng.normal(0, 0.05, n).astype(f32)
    mse = (rng.random(n) * 1.5).astype(f32)
    return dict(n=n, alpha=alpha, weight=weight, normalise=normalise, batch=batch, qbar=qbar, da=da, diff=diff, nmq=nmq, mse=mse)


def _run_hostcheck(exe, tmp_path, h):
    path = str(tmp_path / "bc_in.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<ii4f", h["n"], h["normalise"], h["alpha"], h["weight"], float(h["batch"]), 0.0))
        for k in ("qbar", "da", "diff", "nmq", "mse"):
            f.write(np.ascontiguousarray(h[k], f32).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = np.array([[int(w, 16) for w in line.split()[1:]] for line in out.stdout.strip().split("\n")], np.uint64).astype(np.uint32)
    assert rows.shape == (h["n"], 3)
    return rows


def _assert_hostcheck_equals_the_twin(rows, h):
    with np.errstate(over="ignore", invalid="ignore"):
        lam = np.array([BR.lam(h["alpha"], q, h["normalise"]) for q in h["qbar"]], f32)
        dl = np.array([BR.dloss(l, d, h["weight"], x, h["batch"]) for l, d, x in zip(lam, h["da"], h["diff"])], f32)
        ls = np.array([BR.loss(l, q, h["weight"], m) for l, q, m in zip(lam, h["nmq"], h["mse"])], f32)
    assert np.array_equal(rows[:, 0], U.bits32(lam)), "lambda"
    assert np.array_equal(rows[:, 1], U.bits32(dl)), "the step-4 element"
    assert np.array_equal(rows[:, 2], U.bits32(ls)), "loss_act"
    if h["normalise"] and h["alpha"] > 0:
        assert lam[0] == f32(h["alpha"]) / f32(1e-8) == lam[1] == lam[3] == lam[4] and lam[2] != lam[0]      # Qbar = 0 meets the floor
    if not h["normalise"]:
        assert (lam == f32(h["alpha"])).all()


def test_core_header_on_the_host_equals_the_twin_bit_for_bit(tmp_path):
    """tests/hostcheck/bc_hostcheck.cpp, g++ -ffp-contract=off: lambda, the step-4 element and loss_act.  Cases: the paper's values
    (with Qbar = 0 and its neighbours at the floor), normalise = 0, weight = 0, alpha = 0, batch 1."""
    exe = _hostcheck(tmp_path)
    for kw in (dict(), dict(normalise=0), dict(weight=0.0), dict(alpha=0.0), dict(alpha=1.0, weight=0.0, normalise=0), dict(batch=1, weight=0.3)):
        h = _hostcheck_inputs(**kw)
        _assert_hostcheck_equals_the_twin(_run_hostcheck(exe, tmp_path, h), h)


def test_core_header_on_the_host_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: clean, and the same bits."""
    exe = _hostcheck(tmp_path, sanitize=True)
    h = _hostcheck_inputs(n=64)
    _assert_hostcheck_equals_the_twin(_run_hostcheck(exe, tmp_path, h), h)


# ---- the C surface -------------------------------------------------------------------------------------------------------------------
def test_bc_record_matches_the_c_struct(tmp_path):
    S = U.pkg()
    B = S._capi.BcArgs
    names = [f[0] for f in B._fields_]
    assert names == ["alpha", "weight", "normalise", "reserved", "out"]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shems_hip.h"\nint main(void){printf("%zu %d", sizeof(shems_bc), SHEMS_BC_OUT_FLOATS);' +
                   "".join(f'printf(" %zu", offsetof(shems_bc, {n}));' for n in names) + 'return 0;}\n')
    exe = tmp_path / "o"
    subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(B) == 24 and vals[1] == S._capi.BC_OUT_FLOATS == 132
    assert vals[2:] == [getattr(B, n).offset for n in names] == [0, 4, 8, 12, 16]


_C_TO_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double, "int": C.c_int}


def test_bc_prototypes_match_the_header():
    """Every prototype of _capi._bc_sigs against include/shems_hip.h, argument by argument; each is its plain entry point's argument list
    with `const shems_bc *bc` in front of the stream."""
    S = U.pkg()
    hdr = open(os.path.join(U.ROOT, "include", "shems_hip.h")).read()

    def decl_of(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    for name, args in S._capi._bc_sigs().items():
        decl = decl_of(name)
        assert len(decl) == len(args), (name, decl)
        for d, a in zip(decl, args):
            if "*" in d:
                base = d.replace("const", "").split("*")[0].strip()
                want = {"shems_bc": (C.POINTER(S._capi.BcArgs),), "shems_replay": (C.POINTER(S._capi.Replay),)}.get(base, (C.c_void_p,))
                assert a in want, (name, d, a)
            else:
                assert a is _C_TO_CTYPES[d.split()[0]], (name, d, a)
        plain = decl_of(name[:-3])
        assert decl == plain[:-1] + ["const shems_bc *bc"] + plain[-1:], name


def test_bc_entry_points_are_exported(built_lib):
    S = U.pkg()
    want = {"shems_ddpg_update_bc", "shems_td3_update_bc"}
    assert want <= set(S._capi.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib]).decode()
    assert want <= set(re.findall(r" T (shems_[a-z0-9_]+)", out))


# ---- the value class, the parsers, the refusals ------------------------------------------------------------------------------------------
def test_bc_value_class():
    D = _D()
    b = D.BC()
    assert (b.alpha, b.weight, b.normalise) == (2.5, 1.0, True) and b == D.BC(2.5, 1, True) and b != D.BC(2.5, 0.5)
    assert repr(D.BC(2.5, 0.25, False)) == "BC(alpha=2.5, weight=0.25, normalise=False)"
    assert D.BC(0, 0).alpha == 0.0 and D.BC(normalise=0).normalise is False
    for kw in (dict(alpha=-0.1), dict(weight=-1), dict(alpha=float("nan")), dict(weight=float("inf")), dict(alpha=1e39), dict(alpha="2.5"),
               dict(alpha=True), dict(normalise=2), dict(normalise="yes"), dict(normalise=None)):
        with pytest.raises(ValueError, match="BC:"):
            D.BC(**kw)
    with pytest.raises(AttributeError):
        b.weight = 0.5
    s = b.struct(4096)
    assert (s.alpha, s.weight, s.normalise, s.reserved, s.out) == (2.5, 1.0, 1, 0, 4096)


def test_bc_refusals_name_their_reason():
    D = _D()
    D.bc_refusals("replay")                                   # the defaults: nothing to refuse
    for kw, word in ((dict(prioritized=True), "PrioritizedRing"), (dict(batch=129), "BATCH_SIZE = 129"), (dict(wide=True), "wide network"),
                     (dict(noise_type="pn"), "parameter noise"), (dict(world=2), "data-parallel replicas"), (dict(tiled=True), "tiled"),
                     (dict(grouped=True), "learner group"), (dict(fused=False), "split form")):
        with pytest.raises(NotImplementedError, match=word) as ei:
            D.bc_refusals("replay", **kw)
        assert str(ei.value).startswith("replay: bc ")


def test_shems_bc_parser_and_case():
    D = _D()
    M = importlib.import_module(U.PKG_NAME + ".main")
    assert D.parse_bc(None) is None and M.bc_from_env({}) is None
    assert D.parse_bc("2.5") == D.BC(2.5, 1.0) and D.parse_bc("2.5:0.25") == D.BC(2.5, 0.25) and D.parse_bc("0:0") == D.BC(0, 0)
    assert M.bc_from_env({"SHEMS_BC": "1:2"}) == D.BC(1.0, 2.0)
    for bad in ("", "bc", "2.5:", ":1", "2.5:1:1", "-1", "2.5:-0.5", "nan", "2.5:inf", "1e39", "two"):
        with pytest.raises(ValueError) as ei:
            D.parse_bc(bad)
        assert "SHEMS_BC" in str(ei.value) and repr(bad) in str(ei.value)
    assert D.bc_case_suffix(D.BC(2.5, 1)) == "_bc-a2.5-w1" and D.bc_case_suffix(D.BC(1, 0.25)) == "_bc-a1-w0.25"
    # the entry script: unset leaves the case; set, the suffix goes behind the others; refused combinations by name before any device work
    base = {"JOB_ID": "1179808", "TASK_ID": "1", "GPU_ID": "0", "SHEMS_NUM_EP": "2", "SHEMS_NUM_SEEDS": "1", "SHEMS_SYNTHETIC_DATA": "1"}
    case0 = M.config_from_env(base).case
    assert "_bc-" not in case0
    nowhere = "/nonexistent/bc"
    with pytest.raises(ValueError, match="SHEMS_BC"):
        M.main(dict(base, SHEMS_BC="x"), cwd=nowhere, log=lambda *_: None)
    with pytest.raises(NotImplementedError, match="SHEMS_BC with SHEMS_REPLAY=per"):
        M.main(dict(base, SHEMS_BC="2.5", SHEMS_REPLAY="per"), cwd=nowhere, log=lambda *_: None)
    with pytest.raises(ValueError, match="SHEMS_FORESIGHT_OFFLINE is set without SHEMS_FORESIGHT=1"):
        M.main(dict(base, SHEMS_BC="2.5", SHEMS_FORESIGHT_OFFLINE="10"), cwd=nowhere, log=lambda *_: None)


def test_shems_foresight_offline_parser():
    M = importlib.import_module(U.PKG_NAME + ".main")
    ok = {"SHEMS_FORESIGHT": "1", "SHEMS_BC": "2.5"}
    assert M.foresight_offline({}) is None and M.foresight_offline(ok) is None
    assert M.foresight_offline(dict(ok, SHEMS_FORESIGHT_OFFLINE="200")) == 200
    with pytest.raises(ValueError, match="without SHEMS_FORESIGHT=1"):
        M.foresight_offline({"SHEMS_FORESIGHT_OFFLINE": "5", "SHEMS_BC": "2.5"})
    with pytest.raises(ValueError, match="without SHEMS_BC"):
        M.foresight_offline({"SHEMS_FORESIGHT_OFFLINE": "5", "SHEMS_FORESIGHT": "1"})
    for bad in ("", "0", "-3", "1.5", "ten", "5x2"):
        with pytest.raises(ValueError) as ei:
            M.foresight_offline(dict(ok, SHEMS_FORESIGHT_OFFLINE=bad))
        assert "SHEMS_FORESIGHT_OFFLINE" in str(ei.value) and repr(bad) in str(ei.value)
    assert M.offline_file_name("1179808", "eval", "c") == os.path.join("out/tracker", "1179808_eval_results_c_offline.csv")


def test_offline_refusals_before_anything_is_trained(tmp_path):
    torch = pytest.importorskip("torch")
    I = importlib.import_module(U.PKG_NAME + ".imitation")
    D = _D()
    calls = []

    class Ring:
        def __init__(self, done):
            self.done = torch.tensor(done, dtype=torch.float32)

        def __len__(self):
            return len(self.done)

    agent = types.SimpleNamespace(bc=None, replay=lambda ring: calls.append(ring))
    td = Ring([0.0] * 8)
    with pytest.raises(ValueError, match="agent.bc is None"):
        I.offline(agent, td, 10)
    agent.bc = D.BC()
    for kw in (dict(updates=0), dict(updates=5, record_every=0)):
        with pytest.raises(ValueError, match="at least 1"):
            I.offline(agent, td, **kw)
    with pytest.raises(ValueError, match="'mc' ring"):
        I.offline(agent, Ring([0.0, 0.0, 1.0, 0.0]), 10)
    with pytest.raises(ValueError, match="empty"):
        I.offline(agent, Ring([]), 10)
    assert calls == []
    rows = [(0, 1.0, 2.0, 3.0, 4.0), (7, 0.5, 0.25, 100.0, 0.125)]
    path = I.write_to_offline_file(rows, str(tmp_path / "t" / "x_offline.csv"))
    lines = open(path).read().strip().split("\n")
    assert lines[0] == "update,critic_loss,actor_loss,lambda,mse" and lines[2] == "7,0.5,0.25,100.0,0.125" and len(lines) == 3

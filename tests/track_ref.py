"""Helpers of tests/test_track_edges_gpu.py: a direct launcher for shems_track_dev / shems_wide_track_dev (harness._track always resets
the env, checks the sticky error before it returns the rows and always asks for rows and returns -- the edge cases need each of those
switched off), the oracle walk every case shares, and the exact-arithmetic probe actors.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import importlib

import numpy as np

import util as U
from util import oracle_c
import ddpg_oracle as DO

f32 = np.float32
TUNED = (250, 500)
TOL = 1e-5          # the layers' stated bound (header of csrc/shems_track.hip, tests/test_harness.py): 1e-5 of the float64 evaluation
# The probes' pre-tanh value is exact, so what is left is tanhf (2 ulp in HIP's published table of device math functions), the
# float32 rounding of scale_action's result and nothing else.  An action in [0.5, 1) has ulp 2^-24 = 6e-8, a target (a + 1) / 2 in
# [0.5, 1) the same: 2 ulp of the action halved + half an ulp of the target = 9e-8.  4 ulp = 2.4e-7 leaves a factor ~2.5; the
# smallest slip a probe exists for (one row of 250 counted twice or dropped: 1/256 in p) moves a target by > 4e-4.
PROBE_TOL = 4 * 2.0 ** -24


def mods():
    import torch
    S = U.pkg()
    return torch, S, importlib.import_module(U.PKG_NAME + ".ddpg"), importlib.import_module(U.PKG_NAME + ".harness")


def eval_table():
    """The synthetic eval table (1440 rows), an env config on it, and the (lo, hi) of tests/test_harness.py."""
    S = U.pkg()
    ev = S.tables.synthetic_table("eval", 98)
    st = ev[:, [1, 1, 0, 2, 3, 4, 5, 6, 7]].copy()
    st[:, 0] = np.linspace(0, 6.75, len(st))
    return ev, st.min(0).astype(f32), st.max(0).astype(f32)


def make_env(n, ev):
    S = U.pkg()
    return S.ShemsBatch(n, 1439, [ev], [S.make_config(98, 0, ev.shape[0])])


def net_size(hid):
    h1, h2 = hid
    return 9 * h1 + h1 + h1 * h2 + h2 + 2 * h2 + 2


def blocks(p, hid=TUNED):
    """Writable views (W1 [9][h1], b1, W2 [h1][h2], b2, W3 [h2][2], b3) of a flat Flux-layout actor."""
    h1, h2 = hid
    o = np.cumsum([0, 9 * h1, h1, h1 * h2, h2, 2 * h2, 2])
    assert p.shape == (o[-1],)
    return (p[o[0]:o[1]].reshape(9, h1), p[o[1]:o[2]], p[o[2]:o[3]].reshape(h1, h2), p[o[3]:o[4]], p[o[4]:o[5]].reshape(h2, 2),
            p[o[5]:o[6]])


def glorot(D, seed):
    """The actor of tests/test_harness.py: Glorot weights, the 3e-3 head lifted 50 times."""
    p = D.init_params(seed, 9, 2, 0)
    p[128000:129000] *= 50
    return p


# ---- launching ---------------------------------------------------------------------------------------------------------------------

def make_slab(actors, lo, hi):
    """harness.inference_many's slab: one row per pass, actor | pad to 16 B | s_min[9] | s_max[9] | pad.  lo / hi: [9] or [P][9]."""
    import torch
    A = np.asarray(actors, f32)
    P, na = A.shape
    row = -(-na // 4) * 4 + 32
    host = np.zeros((P, row), f32)
    host[:, :na] = A
    host[:, row - 32:row - 23] = np.asarray(lo, f32)
    host[:, row - 16:row - 7] = np.asarray(hi, f32)
    return torch.from_numpy(host).cuda(), na


def launch(env, slab, na, nsteps, hidden=None, reset=True, results_env=-1, rows=True, returns=True, check=True):
    """One tracking launch, pass e with row e of the slab.  Returns (returns [n] or None, rows [n or 1][nsteps][23] or None); rows the
    kernel did not write stay NaN.  reset=False: the pass goes on from the state the env is in.  check=False: the sticky error is
    left for the caller to read."""
    import torch
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    capi = importlib.import_module(U.PKG_NAME + "._capi")
    L = capi.lib()
    env.use_torch_stream()
    if reset:
        env.reset_(-1)
    assert slab.shape[0] == env.n and slab.is_contiguous()
    row = slab.shape[1]
    res = torch.full((env.n if results_env < 0 else 1, nsteps, 23), float("nan"), dtype=torch.float64, device=slab.device) if rows else None
    tot = torch.full((env.n,), float("nan"), dtype=torch.float64, device=slab.device) if returns else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    base = slab.data_ptr()
    p = D.ActParams(base, base + 4 * (row - 32), base + 4 * (row - 16), 0.0, 0.0, 0, 0, 0, 0, 0.0, 0.0, 0.0, None, None)
    v = env.view()
    if hidden is None:
        rc = L.shems_track_dev(C.byref(v), C.byref(p), 4 * row, 1, nsteps, ptr(res), results_env, ptr(tot), env._stream())
    else:
        L.shems_wide_track_dev.argtypes = [C.POINTER(capi.View), C.POINTER(D.ActParams), C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.shems_wide_track_dev.restype = C.c_int
        rc = L.shems_wide_track_dev(C.byref(v), C.byref(p), int(hidden[0]), int(hidden[1]), 4 * row, nsteps, ptr(res), results_env, ptr(tot),
                                    env._stream())
    capi.check(rc)
    out = (None if tot is None else tot.cpu().numpy(), None if res is None else res.cpu().numpy())
    torch.cuda.synchronize()
    if check:
        env.check_error()
    return out


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------

def seq_sum(x):
    """The float64 sum in hour order, as the kernel's `total += reward` forms it (np.sum adds pairwise)."""
    s = 0.0
    for r in np.asarray(x, np.float64):
        s += float(r)
    return s


def targets64(p):
    """scale_action(tanh(p)) in float64, in the order of the results columns [21, 2] (B_tar, EV_target)."""
    return (np.tanh(np.asarray(p, np.float64)) + 1.0) * 0.5


def follow(ev, res, actor_at=None, lo=None, hi=None, tol=TOL, ref=None, hours=None, want=None):
    """Walk one pass's rows with the C oracle: at every hour (of `hours`, default all) the float64 actor actor_at(t) on the oracle's
    state -- or the fixed float64 targets `want` -- must lie within `tol` of the targets the row holds (neither given: no such check);
    the oracle stepped with the row's targets must give the row bit for bit.  ref: an oracle env to go on with (default: a fresh one from reset).  lo / hi may be
    callables of t.  Returns (ref, worst error, largest |action|, the pre-step states)."""
    if ref is None:
        ref = oracle_c.Batch(1, 1439, ev, oracle_c.profile(98))
        ref.reset(True)
    worst, top, states = 0.0, 0.0, []
    for t in range(len(res)):
        tgt = res[t, [21, 2]].astype(f32)[None]
        assert np.isfinite(res[t]).all(), t
        s = ref.state()
        states.append(s[0].copy())
        if (want is not None or actor_at is not None) and (hours is None or t in hours):
            if want is not None:
                err = float(np.abs(np.asarray(want, np.float64) - res[t, [21, 2]]).max())
            else:
                a = DO.act(actor_at(t), s, lo, hi, False, dtype=np.float64)
                top = max(top, float(np.abs(a).max()))
                err = float(np.abs(oracle_c.scale_action(a) - tgt).max())
            assert err < tol, (t, err, tol)
            worst = max(worst, err)
        rc, _, _, rr = ref.step(tgt, 1, want_results=True)
        assert rc == 0 and (U.bits64(rr[0]) == U.bits64(res[t])).all(), t
    return ref, worst, top, np.array(states)


def check_return(tot, res):
    assert U.bits64(tot) == U.bits64(seq_sum(res[:, 5])), (tot, seq_sum(res[:, 5]))


# ---- exact probes ------------------------------------------------------------------------------------------------------------------
# Every weight is a small dyadic rational and every h1 is 0 or 1, so each product and each partial sum, in any order, is a multiple of
# 2^-18 below 4: exact in float32.  The pre-tanh value is therefore known exactly and a row counted twice or dropped shows in full.

def _blank(hid):
    return np.zeros(net_size(hid), f32)


def probe_row(k):
    """h1 one-hot in row k whatever the observation; W2[k][n] a code of (k, n) in -30/64 .. 30/64 (its period in k is 61 * 29, so no two
    of the 250 rows share a code sequence); W3 signed multiples of 2^-9 keyed by n.  Returns the actor and its exact pre-tanh outputs
    (multiples of 2^-15; every partial sum is below 500 * 30/64 * 7/512 = 3.3, so 17 bits hold it; |p| < 0.21 over all rows)."""
    p = _blank(TUNED)
    W1, b1, W2, b2, W3, b3 = blocks(p)
    b1[:] = -1.0
    b1[k] = 1.0
    W2[:], W3[:] = row_code()
    return p, row_expectations()[k]


def row_code():
    kk, nn = np.meshgrid(np.arange(250), np.arange(500), indexing="ij")
    n = np.arange(500)
    s0, s1 = 1 - 2 * (((n * n) // 7 + n // 3) % 2), 1 - 2 * (((n * n) // 5 + n // 2) % 2)       # signs keyed by n: the rows' sums spread out
    return ((37 * kk + 13 * nn + (kk * nn) % 29) % 61 - 30) / 64.0, np.stack([s0 * ((n % 7) + 1) / 512.0, s1 * ((n % 5) + 1) / 512.0], 1)


def row_expectations():
    """The exact pre-tanh outputs of probe_row(k) for every k: [250][2]."""
    W2, W3 = row_code()
    return np.maximum(W2, 0.0) @ W3


def probe_col(n, hid=TUNED):
    """All h1 = 1, W2 = 1/256: every h2 is l1/256.  W3 one-hot in column n, + on output 0 and - on output 1: p = +- l1/256."""
    p = _blank(hid)
    W1, b1, W2, b2, W3, b3 = blocks(p, hid)
    b1[:] = 1.0
    W2[:] = 1.0 / 256
    W3[n] = [1.0, -1.0]
    return p, np.array([hid[0] / 256.0, -hid[0] / 256.0])


def probe_all(hid=TUNED, b3v=(0.25, -0.5)):
    """All h1 = 1, W2 = 1/256, W3 = 2^-10 everywhere: p = l2 * (l1 / 256) * 2^-10 + b3."""
    p = _blank(hid)
    W1, b1, W2, b2, W3, b3 = blocks(p, hid)
    b1[:] = 1.0
    W2[:] = 1.0 / 256
    W3[:] = 2.0 ** -10
    b3[:] = b3v
    return p, hid[1] * (hid[0] / 256.0) * 2.0 ** -10 + np.asarray(b3v, np.float64)

"""A single learner on the tiled working layout of its layer-2 state (Agent.use_tiled, shems_ddpg_tiled_enter): the five-launch
replay() and the fused step read and write W2, its ADAM moments and the targets' W2 in two tiled regions instead of the Flux-order
blocks.  Same workgroups, summation orders and ADAM function, so everything here is a bit-for-bit comparison with the Flux-order form
(which tests/test_ddpg_gpu.py, test_policy_gpu.py and test_fused_configs_gpu.py hold against the oracles).  There is no host twin of
the W2 addressing: these comparisons are the whole check."""
import ctypes as C
import importlib

import numpy as np
import pytest

import util as U

pytestmark = pytest.mark.gpu

_KEYS = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic", "losses")
ERR_STATE = -6                                     # SHEMS_ERR_STATE
CAP = 600                                          # ring capacity of the replay() cases ("the full capacity")


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    return torch, S, importlib.import_module(U.PKG_NAME + ".ddpg"), importlib.import_module(U.PKG_NAME + ".replay")


def _ring(torch, R, cap, length):
    g = torch.Generator(device="cpu").manual_seed(11)
    ring = R.ReplayRing(cap)
    ring.s.copy_(torch.rand((cap, 9), generator=g))
    ring.s2.copy_(torch.rand((cap, 9), generator=g))
    ring.a.copy_(torch.rand((cap, 2), generator=g) * 2 - 1)
    ring.r.copy_(-torch.rand((cap,), generator=g))
    ring.done.copy_((torch.rand((cap,), generator=g) < 0.1).to(torch.uint8))
    ring.pushed = length
    return ring


def _agent(D, tiled, batch=120):
    ag = D.Agent(seed=31)
    ag.batch = batch
    ag.set_norm(np.zeros(9, np.float32), np.ones(9, np.float32))
    return ag.use_tiled(tiled)


def _same_learner(torch, a, b, what):
    for k in _KEYS:
        x, y = getattr(a, k), getattr(b, k)          # (the accessors bring the Flux-order view up to date)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {k} differs"


def _regions(ag):
    """The two regions as [4 kt][8 nt][4 arrays][64][64] host arrays, and the padded [4 arrays][256][512] view of each."""
    out = []
    for r in ag._w2t.cpu().numpy():
        t = r.reshape(4, 8, 4, 64, 64)
        out.append(t.transpose(2, 0, 3, 1, 4).reshape(4, 256, 512))
    return out


# batch 120 and the edges 1 and 128; ring lengths 1, 119 and the full capacity; the exclusion-window call (a full ring only)
@pytest.mark.parametrize("batch,length,exclude", [(120, CAP, None), (1, CAP, None), (128, CAP, None), (120, 1, None), (120, 119, None),
                                                  (120, CAP, (CAP - 7, 40)), (1, 1, None), (128, 119, None)])
def test_tiled_replay_leaves_the_bits_of_the_flux_order_replay(batch, length, exclude):
    torch, S, D, R = _mods()
    ring = _ring(torch, R, CAP, length)
    flux, tiled = _agent(D, False, batch), _agent(D, True, batch)
    for u in range(3):                               # three updates in a row: the second and third start from tiled state
        flux.replay(ring, exclude=exclude)
        tiled.replay(ring, exclude=exclude)
        assert tiled._tiled_current and not flux._tiled_current
        if u == 0:                                   # the W2 ranges of the Flux-order blocks are stale: an update that read them would show
            for k in D.Agent._W2_BLOCKS:
                w2 = 3000 if "critic" in k else 2500
                tiled._blk(k)[w2:w2 + 125000].fill_(float("nan"))
        if u == 1:
            _same_learner(torch, flux, tiled, f"after update {u + 1}")       # (leaves the tiles; the third update enters again)
    # pads of the regions after updates: rows 250..255 and columns 500..511 exactly zero, in the last k-tile / n-tile and everywhere
    for reg in _regions(tiled):
        assert not reg[:, 250:, :].any() and not reg[:, :, 500:].any()
        assert reg[2, :250, :500].any() and reg[0, :250, :500].any()          # (and the state itself is there)
    _same_learner(torch, flux, tiled, "after update 3")
    assert tiled.updates == flux.updates == 3 and tiled.bp_actor == flux.bp_actor


def test_round_trip_is_the_identity_on_the_flux_ranges_and_zero_on_the_pads():
    torch, S, D, R = _mods()
    ag = _agent(D, True)
    g = torch.Generator(device="cpu").manual_seed(3)
    want = {}
    for k in _KEYS[:8]:                              # every element of the eight blocks distinct from its neighbours
        v = torch.rand(getattr(ag, k).numel(), generator=g) + 0.5
        getattr(ag, k).copy_(v)
        want[k] = v.clone()
    ag._w2t = torch.full((2, D.W2T_FLOATS), 7.0, dtype=torch.float32, device="cuda")      # stale garbage in the regions, pads included
    assert ag._enter_tiled()
    for net, (reg, names, w2) in enumerate(zip(_regions(ag), (("m_actor", "v_actor", "actor", "actor_t"), ("m_critic", "v_critic", "critic", "critic_t")),
                                               (2500, 3000))):
        assert not reg[:, 250:, :].any() and not reg[:, :, 500:].any()            # last k-tile's rows, last n-tile's columns: zeros
        for a, k in enumerate(names):
            flux = want[k].numpy()[w2:w2 + 125000].reshape(250, 500)
            assert np.array_equal(reg[a, :250, :500], flux), (net, k)
            assert np.array_equal(reg[a, 192:250, 448:500], flux[192:, 448:])     # the last tile explicitly
    for k in _KEYS[:8]:                              # the W2 ranges of the Flux-order blocks are stale now: overwrite them, then come back
        w2 = 3000 if "critic" in k else 2500
        ag._blk(k)[w2:w2 + 125000].fill_(-1.0)
    for k in _KEYS[:8]:
        assert torch.equal(getattr(ag, k).cpu(), want[k]), k                      # (the accessor leaves the tiles: to_flux)
    assert not ag._tiled_current


def _fused_steps(tiled, n, window, nsteps=3):
    torch, S, D, R = _mods()
    env, _ref, _tabs, _cfgs, _co, _tab_of = U.mixed_batches(n)                   # mixed per-env configs
    env.use_torch_stream()
    ag = D.Agent(seed=77).use_tiled(tiled)
    p = D.init_params(77, 9, 2, 0)
    p[128000:129000] *= 60.0
    ag.set_params(actor=p)
    env.reset_(5, episode=0)
    st0 = env.state
    ag.set_norm(st0.min(0), st0.max(0))
    ring = R.ReplayRing(2000)
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    rew = torch.empty(n, dtype=torch.float64, device="cuda")
    if tiled:
        assert ag._enter_tiled()
        ag._blk("actor")[2500:127500].fill_(float("nan"))                        # the Flux-order W2 is stale: reading it would show
    outs = []
    for t in range(nsteps):
        w = D.RingWindow((t * 333) % ring.capacity, min(n, 333), (t * 333) % n) if window else None
        ag.act_step(env, train=True, tick=t, a_out=a_out, rewards=rew, ring=ring if window else None, window=w)
        env.check_error()
        outs.append((a_out.clone(), rew.clone(), env.state.copy(), env.idx.copy()))
    assert ag._tiled_current == tiled
    out = (outs, ring.s.clone(), ring.a.clone(), ring.r.clone(), ring.s2.clone())
    env.close()
    return torch, out


# the small-batch forms at 32, 33, 64 and 4 096 + 1 envs; k_act2 (its tiled twin k_act2_t) at 8 192 + 64 and at a count that is no multiple of 64
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("n", [32, 33, 64, 4096 + 1, 8192 + 64, 8192 + 64 + 37])
def test_fused_step_reading_tiles_writes_the_bytes_of_the_flux_order_step(n, window):
    torch, a = _fused_steps(False, n, window)
    _, b = _fused_steps(True, n, window)
    for t, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)), f"actions, step {t}"
        assert torch.equal(x[1].view(torch.int64), y[1].view(torch.int64)), f"rewards, step {t}"
        assert np.array_equal(U.bits32(x[2]), U.bits32(y[2])) and np.array_equal(x[3], y[3]), f"env state, step {t}"
    for k, (x, y) in enumerate(zip(a[1:], b[1:])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"ring array {k}"


def test_train_steps_leave_the_same_state_with_the_mode_on_and_off(monkeypatch):
    torch, S, D, R = _mods()
    ends = []
    for knob in ("0", "1"):
        monkeypatch.setenv("SHEMS_AGENT_TILED", knob)
        wl = D.TrainWorkload(S, torch, 4096 + 32, seed=777, updates=1, loop="native")
        assert wl.tiled == (knob == "1")
        wl.steps(50)
        wl.steps(30)                                 # 80 steps: one episode boundary
        assert wl.agent._tiled_current == (knob == "1")
        wl.finish()
        crc = wl.extra()["learner_crc32"]
        ag = wl.agent
        ends.append(({k: getattr(ag, k).clone() for k in _KEYS}, [x.clone() for x in (wl.ring.s, wl.ring.a, wl.ring.r, wl.ring.s2, wl.rew32)],
                     (wl.env.state.copy(), wl.env.idx.copy(), wl.env.step.copy()), (crc, wl.t, wl.episode, wl.ring.pushed, ag.updates, tuple(ag.bp_actor))))
        wl.close()
    (la, ra, ea, ha), (lb, rb, eb, hb) = ends
    for k in _KEYS:
        assert torch.equal(la[k].view(torch.int32), lb[k].view(torch.int32)), k
    for x, y in zip(ra, rb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert np.array_equal(U.bits32(ea[0]), U.bits32(eb[0])) and np.array_equal(ea[1], eb[1]) and np.array_equal(ea[2], eb[2])
    assert ha == hb, (ha, hb)


def test_flux_order_entry_points_are_refused_while_the_tiles_are_current():
    torch, S, D, R = _mods()
    ring = _ring(torch, R, CAP, CAP)
    ag = _agent(D, True)
    ag.replay(ring)
    assert ag._tiled_current
    cur = C.c_int32(0)
    d = ag._ddpg_args(raw=True)
    assert ag.L.shems_ddpg_tiled_current(C.byref(d), C.byref(cur)) == 0 and cur.value == 1
    raw = lambda k: ag._blk(k) if k in D.Agent._W2_BLOCKS else getattr(ag, k)       # (no accessor: it would leave the tiles)
    before = {k: raw(k).clone() for k in _KEYS}
    regions = ag._w2t.clone()
    st, rs = ag._stream(), ring.struct()
    pub = torch.zeros(ag.n_actor, dtype=torch.float32, device="cuda")
    calls = [lambda: ag.L.shems_ddpg_critic_grad(C.byref(d), C.byref(rs), CAP, 1, 0, st),
             lambda: ag.L.shems_ddpg_critic_apply(C.byref(d), 1e-4, 0.9, 0.999, 1.0, st),
             lambda: ag.L.shems_ddpg_actor_grad(C.byref(d), st),
             lambda: ag.L.shems_ddpg_actor_apply(C.byref(d), 1e-4, 0.9, 0.999, 1.0, st),
             lambda: ag.L.shems_ddpg_critic_update(C.byref(d), C.byref(rs), CAP, 1, 0, 1e-4, 0.9, 0.999, st),
             lambda: ag.L.shems_ddpg_clone_update(C.byref(d), C.byref(rs), CAP, 1, 0, 1e-4, 0.9, 0.999, None, st),
             lambda: ag.L.shems_ddpg_update(C.byref(d), C.byref(rs), CAP, 1, 0, 0, 0, 1e-4, 0.9, 0.999, 1e-4, 0.9, 0.999,
                                            C.c_void_p(pub.data_ptr()), st),                       # the published copy is a Flux-order block
             lambda: ag.L.shems_ddpg_tiled_enter(C.byref(d), C.byref(D.W2T(ag._w2t[0].data_ptr(), ag._w2t[1].data_ptr())), st)]
    for i, call in enumerate(calls):
        assert call() == ERR_STATE, i
    torch.cuda.synchronize()
    for k in _KEYS:
        assert torch.equal(before[k].view(torch.int32), raw(k).view(torch.int32)), k
    assert torch.equal(regions.view(torch.int32), ag._w2t.view(torch.int32)) and not pub.any()
    ag.flux_()
    assert ag.L.shems_ddpg_tiled_current(C.byref(d), C.byref(cur)) == 0 and cur.value == 0
    assert ag.L.shems_ddpg_tiled_leave(C.byref(d), st) == ERR_STATE                                        # not on tiles any more
    assert ag.L.shems_ddpg_critic_grad(C.byref(d), C.byref(rs), CAP, 1, 0, st) == 0                 # and Flux order is served again
    torch.cuda.synchronize()

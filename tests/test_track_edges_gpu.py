"""The tracking pass (csrc/shems_track.hip: k_track<false> for the tuned (250, 500) actor, k_track<true> for any hidden sizes) at the
places where its own thread map, its register prefetch and its pass bookkeeping can go wrong without the Glorot-weight passes of
tests/test_harness.py showing it:

  seams        layer 2's row blocks start at 0, 64, 128 and 186 (rows 186..191 meet six zeros), eight batches of 8 row segments
               alternate between two register buffers, layer 3 clamps threads 500..511 and sums 8 waves -- exact probes
  pass edges   nsteps 1 and 2, a pass continued from the state another left, the actor swapped between two launches, per-pass
               normalisation bounds, results_env / null outputs, the table end in actor mode
  value edges  tanhf saturated to +-1, a dead hidden layer, an observation column with s_max == s_min
  wide kernel  l1 % 4 != 0, l1 < 4, l2 < 64, both sizes above 512, sizes of 1; the same probes at (5, 64) and (513, 7)

Reference, as in test_harness.py: the C oracle stepped with the targets each results row holds must reproduce the row bit for bit;
DDPG_oracle.act in float64 on the oracle's state must lie within the bound of those targets; a pass's return is the float64 sum of
its reward column in hour order (track_ref.follow / check_return).

Bounds.  Probes: track_ref.PROBE_TOL (4 ulp of a float32 target; the pre-tanh value is exact).  Everything else: 1e-5, the layers'
stated bound.  Every non-probe case also evaluates the float32 NumPy oracle on its own inputs and prints its distance from float64
(`f32 oracle`): on the host these were 1.2e-7 or less for every case of this file (profiles/NOTES.md), nowhere near 1e-5, so no
case needs the wider 4 x measured allowance and none takes it.

ReLU ties: relu is continuous, so a pre-activation near zero does not make a forward pass ambiguous -- the float64 action moves by
no more than the pre-activation does.  The one place where the sign of a pre-activation decides what the test expects is the dead
layer cases (the action is tanh(b3) only if every unit is off): there the float64 pre-activations are asserted to stay 1e-4 and
more below zero."""
import numpy as np
import pytest

import util as U
from util import oracle_c
import ddpg_oracle as DO
import track_ref as R
import test_wide_sizes_gpu as TS

pytestmark = pytest.mark.gpu
f32 = np.float32

ROW_K = (0, 7, 8, 63, 64, 127, 128, 185, 186, 191, 192, 249)       # both sides of every batch of 8 and of every row block's start
COL_N = (0, 3, 4, 63, 64, 447, 448, 496, 499)                      # quads, wave 0 / 1, wave 6 / 7, the last quad, the last column
WIDE_SIZES = ((1, 1), (3, 5), (5, 64), (250, 500), (513, 7), (6, 1025), (1023, 513))


def _f32_distance(actor_at, states, lo, hi):
    """The float32 NumPy oracle's distance from float64 over the pre-step states of a pass, in scaled-action units."""
    d = 0.0
    for t, s in enumerate(states):
        a64 = DO.act(actor_at(t), s[None], lo, hi, False, dtype=np.float64)
        a32 = DO.act(actor_at(t), s[None], lo, hi, False, dtype=np.float32)
        d = max(d, float(np.abs(oracle_c.scale_action(a64).astype(np.float64) - oracle_c.scale_action(a32)).max()))
    return d


def _run_probes(probes, hid=None):
    """All probes as the actors of one launch, 2 hours each: hour 0 runs on the batch loaded before the hour loop, hour 1 on the one
    the last load of hour 0 prefetched.  Each target against scale_action(tanh(p_exact)) in float64, each row against the oracle.
    The tuned probes go through harness.inference_many; it sends only sizes above (250, 500) to the wide kernel, so the wide probes
    are launched directly."""
    torch, S, D, H = R.mods()
    ev, lo, hi = R.eval_table()
    env = R.make_env(len(probes), ev)
    actors = np.stack([p for p, _ in probes])
    if hid is None:
        tot, res = H.inference_many(env, actors, lo, hi, num_steps=2)
    else:
        slab, na = R.make_slab(actors, lo, hi)
        tot, res = R.launch(env, slab, na, 2, hidden=hid)
    env.close()
    assert res.shape == (len(probes), 2, 23)
    worst = 0.0
    for e, (_, p_exact) in enumerate(probes):
        _, err, _, _ = R.follow(ev, res[e], want=R.targets64(p_exact), tol=R.PROBE_TOL)
        R.check_return(tot[e], res[e])
        worst = max(worst, err)
    return worst


# ---- exact probes, tuned kernel ----------------------------------------------------------------------------------------------------

def test_row_probes_every_row_counts_once():
    """h1 one-hot in row k: layer 2's output IS row k of W2, which a code of (k, n) makes different from every neighbour's.  A row read
    by two blocks (186..191) doubles, a row paired with the wrong h1 slot or the wrong buffer gives another row's code."""
    probes = [R.probe_row(k) for k in ROW_K]
    every = R.row_expectations()
    assert np.abs(every).max() < 0.25
    # a probed row taken for ANY other row, or its weights for 2 x or 0 x themselves, is 2^-12 and more off in p: 400 x PROBE_TOL in
    # the target (d target = d p * (1 - tanh(p)^2) / 2 >= 0.4 d p for |p| < 0.5)
    for k in ROW_K:
        d = np.abs(every - every[k]).max(1)
        d[k] = np.inf
        assert d.min() >= 2.0 ** -12 and np.abs(every[k]).min() >= 2.0 ** -12, (k, d.min())
    worst = _run_probes(probes)
    print(f"row probes: max |err| {worst:.3g} (bound {R.PROBE_TOL:.3g})")


def test_column_and_all_on_probes():
    """Every h2 = 250/256 exactly (256/256: the seam rows counted twice; 244/256: dropped); W3 picks column n with opposite signs on
    the two outputs, so a column lost by the thread clamp at 500 or by the wave sum gives p = 0, and one taken twice 2 p.  The all-on
    probe sums all 500 columns and adds b3."""
    probes = [R.probe_col(n) for n in COL_N] + [R.probe_all()]
    assert (probes[0][1] == [250 / 256, -250 / 256]).all() and (probes[-1][1] == 125000 * 2.0 ** -18 + np.array([0.25, -0.5])).all()
    worst = _run_probes(probes)
    print(f"column / all-on probes: max |err| {worst:.3g} (bound {R.PROBE_TOL:.3g})")


# ---- pass edges, tuned kernel ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def glorot_actors():
    D = R.mods()[2]
    return [R.glorot(D, seed) for seed in (4, 5, 6, 7, 8)]


def test_short_passes_are_the_first_hours_of_a_longer_one(glorot_actors):
    """nsteps = 1: no load inside the hour loop's last trip at all; 2: exactly one prefetch across hours; 9: the reference pass, held
    to float64 hour by hour."""
    ev, lo, hi = R.eval_table()
    acts = glorot_actors[:2]
    env = R.make_env(2, ev)
    slab, na = R.make_slab(np.stack(acts), lo, hi)
    tot9, res9 = R.launch(env, slab, na, 9)
    worst, d32 = 0.0, 0.0
    for e in range(2):
        _, err, _, states = R.follow(ev, res9[e], lambda t: acts[e], lo, hi)
        R.check_return(tot9[e], res9[e])
        worst, d32 = max(worst, err), max(d32, _f32_distance(lambda t: acts[e], states, lo, hi))
    for n in (1, 2, 9):
        tot, res = R.launch(env, slab, na, n)
        assert res.shape == (2, n, 23) and (U.bits64(res) == U.bits64(res9[:, :n])).all(), n
        for e in range(2):
            R.check_return(tot[e], res[e])
        assert (env.idx == 1 + n).all() and (env.step == n).all()
    env.close()
    print(f"short passes: max |err| {worst:.3g} (bound {R.TOL:.3g}), f32 oracle {d32:.3g}")


def test_pass_continued_over_three_launches_equals_one_pass(glorot_actors):
    """40 hours as 1 + 2 + 37 on the same env without a reset: the rows are the bytes of one 40-hour pass.  Each launch's return is the
    hour-order sum of its own rows; the three add up to the single pass's return to float64 rounding (another summation order:
    40 adds of |reward| <= R each err by at most 40 * 2^-53 * 40 R)."""
    ev, lo, hi = R.eval_table()
    acts = glorot_actors[1:3]
    env = R.make_env(2, ev)
    slab, na = R.make_slab(np.stack(acts), lo, hi)
    tot40, res40 = R.launch(env, slab, na, 40)
    worst = 0.0
    for e in range(2):
        _, err, top, _ = R.follow(ev, res40[e], lambda t: acts[e], lo, hi)
        R.check_return(tot40[e], res40[e])
        worst = max(worst, err)
    parts, tots = [], []
    for k, n in enumerate((1, 2, 37)):
        tot, res = R.launch(env, slab, na, n, reset=(k == 0))
        for e in range(2):
            R.check_return(tot[e], res[e])
        parts.append(res)
        tots.append(tot)
    env_idx, env_step = env.idx, env.step
    env.close()
    assert (U.bits64(np.concatenate(parts, 1)) == U.bits64(res40)).all()
    assert (env_idx == 41).all() and (env_step == 40).all()
    slack = 40 * 2.0 ** -53 * 40 * np.abs(res40[:, :, 5]).max()
    assert (np.abs(tots[0] + tots[1] + tots[2] - tot40) <= slack).all()
    print(f"continued pass: max |err| {worst:.3g} (bound {R.TOL:.3g})")


def test_actor_swapped_between_launches_takes_effect_at_once(glorot_actors):
    """The same 1 + 2 + 37 split, the actor overwritten IN PLACE (same device block) after the first launch: every hour is held to
    the float64 actor in force at that hour, so a weight, a bias or a prefetched batch that outlived its actor shows."""
    ev, lo, hi = R.eval_table()
    first, then = glorot_actors[0], glorot_actors[3]
    env = R.make_env(1, ev)
    slab, na = R.make_slab(first[None], lo, hi)
    import torch
    parts, ref, worst, states = [], None, 0.0, []
    for k, n in enumerate((1, 2, 37)):
        if k == 1:
            slab[0, :na].copy_(torch.from_numpy(then))
        tot, res = R.launch(env, slab, na, n, reset=(k == 0))
        ref, err, _, st = R.follow(ev, res[0], lambda t: first if k == 0 else then, lo, hi, ref=ref)
        R.check_return(tot[0], res[0])
        parts.append(res[0])
        states.append(st)
        worst = max(worst, err)
    env.close()
    rows = np.concatenate(parts)
    # the swap matters: the float64 action of the other actor is far from what hours 0 and 1 took
    st = np.concatenate(states)
    for t, other in ((0, then), (1, first)):
        a = oracle_c.scale_action(DO.act(other, st[t][None], lo, hi, False, dtype=np.float64))
        assert np.abs(a - rows[t, [21, 2]]).max() > 1e-3, t
    print(f"swapped actor: max |err| {worst:.3g} (bound {R.TOL:.3g})")


def _bounds(lo, hi, k):
    """Pass k's own normalisation bounds: wider than the data's by an amount that grows with k (x stays inside [0, 1])."""
    return (lo - f32(0.1 * k) * (1 + np.arange(9, dtype=f32) / 8)).astype(f32), (hi + f32(0.25 * k) * (hi - lo + 1)).astype(f32)


def test_five_passes_each_with_its_own_actor_and_bounds(glorot_actors):
    """harness.inference_many with s_min / s_max of shape [P][9]: pass k is held to float64 with bounds k -- and is far from the
    float64 action under pass 0's bounds, so a kernel that reads the bounds without the per-env stride cannot pass."""
    torch, S, D, H = R.mods()
    ev, lo, hi = R.eval_table()
    P, steps = len(glorot_actors), 40
    los, his = zip(*[_bounds(lo, hi, k) for k in range(P)])
    env = R.make_env(P, ev)
    tot, res = H.inference_many(env, np.stack(glorot_actors), np.stack(los), np.stack(his), num_steps=steps)
    env.close()
    assert res.shape == (P, steps, 23)
    worst, d32 = 0.0, 0.0
    for k in range(P):
        _, err, top, states = R.follow(ev, res[k], lambda t: glorot_actors[k], los[k], his[k])
        R.check_return(tot[k], res[k])
        worst, d32 = max(worst, err), max(d32, _f32_distance(lambda t: glorot_actors[k], states, los[k], his[k]))
        if k:
            a0 = oracle_c.scale_action(DO.act(glorot_actors[k], states, los[0], his[0], False, dtype=np.float64))
            assert np.abs(a0 - res[k][:, [21, 2]]).max() > 1e-3, k
    print(f"per-pass bounds: max |err| {worst:.3g} (bound {R.TOL:.3g}), f32 oracle {d32:.3g}")


def test_results_env_and_null_outputs(glorot_actors):
    """results_env = k writes pass k's rows into row block 0; a null d_results or d_returns changes nothing else."""
    ev, lo, hi = R.eval_table()
    P, steps, k = len(glorot_actors), 12, 2
    env = R.make_env(P, ev)
    slab, na = R.make_slab(np.stack(glorot_actors), lo, hi)
    tot, res = R.launch(env, slab, na, steps)
    assert np.isfinite(res).all() and len({float(t) for t in tot}) == P
    tot_k, res_k = R.launch(env, slab, na, steps, results_env=k)
    assert res_k.shape == (1, steps, 23) and (U.bits64(res_k[0]) == U.bits64(res[k])).all() and (U.bits64(tot_k) == U.bits64(tot)).all()
    tot_n, none = R.launch(env, slab, na, steps, rows=False)
    assert none is None and (U.bits64(tot_n) == U.bits64(tot)).all()
    none, res_n = R.launch(env, slab, na, steps, returns=False)
    assert none is None and (U.bits64(res_n) == U.bits64(res)).all()
    assert (env.idx == 1 + steps).all() and (env.step == steps).all()
    env.close()
    R.follow(ev, res[k], lambda t: glorot_actors[k], lo, hi)


def test_actor_mode_past_the_end_of_the_table(glorot_actors):
    """1445 hours from row 1 of the 1440-row table, 2 envs with their own actors: hour 1440 needs row 1441.  Thread 32's prefetch row
    is clamped, thread 0 raises the sticky bounds error and all 512 threads leave the hour loop together.  The 1439 hours before are
    intact (the oracle reproduces them; the last 20 targets are also held to float64), nothing is written after them, and the handle
    works on once the error was read."""
    torch, S, D, H = R.mods()
    ev, lo, hi = R.eval_table()
    assert ev.shape[0] == 1440
    acts = glorot_actors[:2]
    env = R.make_env(2, ev)
    slab, na = R.make_slab(np.stack(acts), lo, hi)
    tot, res = R.launch(env, slab, na, 1445, check=False)
    with pytest.raises(S._capi.BoundsError):
        env.check_error()
    assert (env.idx == 1440).all() and (env.step == 1439).all()
    assert np.isnan(res[:, 1439:]).all()
    worst = 0.0
    for e in range(2):
        _, err, _, _ = R.follow(ev, res[e, :1439], lambda t: acts[e], lo, hi, hours=range(1419, 1439))
        R.check_return(tot[e], res[e, :1439])
        worst = max(worst, err)
    tot10, res10 = R.launch(env, slab, na, 10)
    assert (U.bits64(res10) == U.bits64(res[:, :10])).all() and (env.idx == 11).all()
    env.close()
    print(f"table end: max |err| over the last 20 hours {worst:.3g} (bound {R.TOL:.3g})")


# ---- value edges, tuned kernel -----------------------------------------------------------------------------------------------------

def test_saturated_head_gives_the_ends_of_scale_action(glorot_actors):
    """b3 = (+20, -20) with W3 = 0: tanh is 1 to float32 beyond 9.1, so the clamp's inputs are exactly +-1 and the targets exactly
    scale_action(+1) = 1 and scale_action(-1) = 0 -- every hour, whatever the hidden layers hold."""
    ev, lo, hi = R.eval_table()
    both = []
    for sign in (1.0, -1.0):
        p = glorot_actors[0].copy()
        W1, b1, W2, b2, W3, b3 = R.blocks(p)
        W3[:] = 0.0
        b3[:] = [20.0 * sign, -20.0 * sign]
        both.append(p)
    env = R.make_env(2, ev)
    slab, na = R.make_slab(np.stack(both), lo, hi)
    tot, res = R.launch(env, slab, na, 30)
    env.close()
    assert (oracle_c.scale_action(np.array([1.0, -1.0], f32)) == [1.0, 0.0]).all()
    assert (res[0][:, [21, 2]] == [1.0, 0.0]).all() and (res[1][:, [21, 2]] == [0.0, 1.0]).all()
    for e in range(2):
        R.follow(ev, res[e], lambda t: both[e], lo, hi)
        R.check_return(tot[e], res[e])


@pytest.mark.parametrize("layer", [1, 2])
def test_dead_hidden_layer_leaves_tanh_of_b3(glorot_actors, layer):
    """b1 = -10 (every relu of layer 1 off) or b2 = -10 (layer 2 off): the action is tanh(b3) for every state -- exact up to tanhf.
    That every float64 pre-activation of the dead layer stays 1e-4 and more below zero is asserted on the pass's own states."""
    ev, lo, hi = R.eval_table()
    p = glorot_actors[1].copy()
    W1, b1, W2, b2, W3, b3 = R.blocks(p)
    (b1 if layer == 1 else b2)[:] = -10.0
    if layer == 2:
        b1[:] = 0.05                                            # layer 1 alive
    b3[:] = [0.3, -0.2]
    env = R.make_env(1, ev)
    slab, na = R.make_slab(p[None], lo, hi)
    tot, res = R.launch(env, slab, na, 30)
    env.close()
    _, err, _, states = R.follow(ev, res[0], want=R.targets64(b3), tol=R.PROBE_TOL)
    R.check_return(tot[0], res[0])
    _, (x, z1, h1, z2, h2, z3) = DO.mlp_forward(p, DO.normalize(states, lo, hi), 9, 2, True, keep=True, dtype=np.float64)
    z = z1 if layer == 1 else z2
    assert z.max() <= -1e-4 and (layer == 1 or h1.max() > 0.05), float(z.max())
    assert np.ptp(states[:, 0]) > 0.1                           # the state moved under the constant action
    print(f"dead layer {layer}: max |err| {err:.3g} (bound {R.PROBE_TOL:.3g}), largest pre-activation {z.max():.3g}")


def test_constant_observation_column_uses_the_1e_8_range(glorot_actors):
    """s_min[3] == s_max[3] while d_e (column 3) moves over 0.2 .. 6 kWh: the range is 1e-8f and x[3] reaches 6e8.  W1's row 3 is
    scaled by 1e-8, so its products are of the size of (s - lo) * w and float32 stays finite.  Held to float64 of the same formula,
    (s - lo) / ((hi - lo) + 1e-8f) with the float32 constant, subtraction and division in float64: the float32 division errs by
    2^-24 relative, 6e-8 * |x w| <= 6e-8 on a pre-activation, so float32 and float64 do not part here (f32 oracle printed below)
    and the 1e-5 bound stands."""
    ev, lo, hi = R.eval_table()
    hi = hi.copy()
    hi[3] = lo[3]
    p = glorot_actors[2].copy()
    W1 = R.blocks(p)[0]
    W1[3] *= f32(1e-8)
    env = R.make_env(1, ev)
    slab, na = R.make_slab(p[None], lo, hi)
    steps = 60
    tot, res = R.launch(env, slab, na, steps)
    env.close()
    _, _, _, states = R.follow(ev, res[0])                      # rows reproduced; the states they were taken in
    R.check_return(tot[0], res[0])
    rng = ((hi - lo) + f32(1e-8)).astype(np.float64)
    assert rng[3] == float(f32(1e-8))
    x = (states.astype(np.float64) - lo.astype(np.float64)) / rng
    assert x[:, 3].max() > 1e8 and np.ptp(x[:, 3]) > 1e8
    a64 = np.tanh(DO.mlp_forward(p, x, 9, 2, False, dtype=np.float64))
    want = (a64 + 1.0) * 0.5
    err = float(np.abs(want - res[0][:, [21, 2]]).max())
    a32 = DO.act(p, states, lo, hi, False, dtype=np.float32)
    d32 = float(np.abs(want - oracle_c.scale_action(a32)).max())
    print(f"constant column: max |err| {err:.3g} (bound {R.TOL:.3g}), f32 oracle {d32:.3g}, max |a| {np.abs(a64).max():.3f}")
    assert np.isfinite(res).all() and err < R.TOL and np.abs(a64).max() > 0.3
    # the column is live: without it the float64 action is elsewhere
    x0 = x.copy()
    x0[:, 3] = 0.0
    assert np.abs(np.tanh(DO.mlp_forward(p, x0, 9, 2, False, dtype=np.float64)) - a64).max() > 1e-3


# ---- wide kernel -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hid", WIDE_SIZES, ids=lambda h: f"{h[0]}x{h[1]}")
def test_wide_pass_matches_float64_at_every_size(monkeypatch, glorot_actors, hid):
    """k_track<true>, one env, 6 hours: l1 = 1, 3, 5, 6 (the 4-wide body runs 0 or 1 times, the scalar tail 1 to 3), l2 = 1, 5, 7 (one
    wave, 63 to 57 idle lanes), 513 / 1023 / 1025 (two and three trips of the stride loops, the last of 1 thread), dynamic LDS of
    4 .. 4096 bytes.  The networks are tests/test_wide_sizes_gpu.py's (non-zero biases in both hidden layers), the float64 forward is
    DDPG_oracle's at that size.  (250, 500) also runs through k_track<false>: the two kernels agree to the bound."""
    torch, S, D, H = R.mods()
    TS._at(monkeypatch, hid)
    ev, lo, hi = R.eval_table()
    pa, _ = TS._nets(D, 4, hid)
    assert pa.shape == (R.net_size(hid),)
    env = R.make_env(1, ev)
    slab, na = R.make_slab(pa[None], lo, hi)
    tot, res = R.launch(env, slab, na, 6, hidden=hid)
    _, err, top, states = R.follow(ev, res[0], lambda t: pa, lo, hi)
    R.check_return(tot[0], res[0])
    d32 = _f32_distance(lambda t: pa, states, lo, hi)
    assert top > 0.3
    if hid == R.TUNED:
        tot_t, res_t = R.launch(env, slab, na, 6)
        assert np.abs(res_t[0][:, [21, 2]] - res[0][:, [21, 2]]).max() < R.TOL
        R.follow(ev, res_t[0], lambda t: pa, lo, hi)
    env.close()
    print(f"wide pass {hid}: max |err| {err:.3g} (bound {R.TOL:.3g}), f32 oracle {d32:.3g}, max |a| {top:.3f}")


@pytest.mark.parametrize("hid,cols", [((5, 64), (0, 3, 4, 63)), ((513, 7), (0, 3, 4, 6))], ids=["5x64", "513x7"])
def test_wide_column_and_all_on_probes(hid, cols):
    """The exact probes on k_track<true>: every h2 = l1/256 (5/256: one 4-wide trip + a tail of 1; 513/256: the same after two trips
    of layer 1's stride loop), column n picked with opposite signs, then all columns + b3."""
    probes = [R.probe_col(n, hid) for n in cols] + [R.probe_all(hid)]
    assert (probes[0][1] == [hid[0] / 256, -hid[0] / 256]).all()
    worst = _run_probes(probes, hid=hid)
    print(f"wide probes {hid}: max |err| {worst:.3g} (bound {R.PROBE_TOL:.3g})")

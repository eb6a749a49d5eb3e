"""The fused act -> step -> remember kernels against the float64 actor and the C env oracle with a config index per env (BASELINE
config 5: ten charger profiles x the discomfort-weight sweep, the tables of env.mixed_profile_setup -- real series of 4 319 and 4 320
rows next to synthetic ones).  The small-tile forms fetch the env's config index, its table row and h_countdown ahead into LDS
(TailPre, csrc/shems_policy.hip); a wrong index there reads a neighbouring profile's row without faulting, so every form, the noise
kinds, the grouped call and the tracking pass meet the oracle here with mixed configs, and the table edges of each config are stepped
through the fused path."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import util as U
from util import oracle_c
import ddpg_oracle as DO

pytestmark = pytest.mark.gpu
ATOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    D = importlib.import_module(U.PKG_NAME + ".ddpg")
    return torch, S, D


def _actor(D, seed):
    p = D.init_params(seed, 9, 2, 0)
    p[128000:129000] *= 60.0                       # layer 3 large enough that tanh and the clamp see their whole range
    return p


def _check_ring(ring, pos, off, count, n, s, a, r_ref, s2):
    rel = (np.arange(n) - off) % n
    sel = np.where(rel < count)[0]
    slots = (pos + rel[sel]) % ring.capacity
    assert (U.bits32(ring.s.cpu().numpy()[slots]) == U.bits32(s[sel])).all()
    assert (U.bits32(ring.s2.cpu().numpy()[slots]) == U.bits32(s2[sel])).all()
    assert (U.bits32(ring.a.cpu().numpy()[slots]) == U.bits32(a[sel])).all()
    assert (ring.r.cpu().numpy()[slots] == r_ref[sel].astype(np.float32)).all()


def fused_mixed_steps(n, nsteps, sums=False, noise="gn"):
    """nsteps fused steps of one learner on n envs with per-env configs: actions against the float64 act() of the pre-step
    observation, transitions bit for bit against the oracle driven by those actions, the ring window exactly.  Returns the charger
    profiles on which an EV got newly connected (h_countdown -1 -> h >= 0)."""
    torch, S, D = _mods()
    R = importlib.import_module(U.PKG_NAME + ".replay")
    env, ref, tabs, cfgs, co, tab_of = U.mixed_batches(n)
    env.use_torch_stream()
    kw = dict(sigma=0.3, theta=0.15, dt=1e-2) if noise == "ou" else dict(eps=0.3) if noise == "en" else {}
    ag = D.Agent(seed=77, noise_type=noise, **kw)
    p = _actor(D, 77)
    ag.set_params(actor=p)
    env.reset_(5, episode=0)
    st0 = env.state
    lo, hi = st0.min(0), st0.max(0)
    ag.set_norm(lo, hi)
    ref.set_state(st0, env.idx)
    ring = R.ReplayRing(5000)
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    rew = torch.empty(n, dtype=torch.float64, device="cuda")
    rew32 = torch.empty(n, dtype=torch.float32, device="cuda")
    blk = torch.zeros(ag.act_step_blocks(n), dtype=torch.float64, device="cuda") if sums else None
    X = np.zeros((n, 2), np.float32) if noise == "ou" else None
    tol = 5e-6 + ATOL if noise == "gn" else 2e-5
    connected = set()
    pos = 0
    for t in range(nsteps):
        pre = env.state
        off = (t * 333) % n
        ag.act_step(env, train=True, tick=t, a_out=a_out, rewards=rew, rewards_f32=rew32, block_reward=blk, ring=ring,
                    window=D.RingWindow(pos % ring.capacity, 333, off))
        env.check_error()
        a = a_out.cpu().numpy()
        want = DO.act(p, pre, lo, hi, True, seed=77, tick=t, sigma=kw.get("sigma", 0.1), noise=noise, ou_state=X,
                      theta=0.15, dt=1e-2, eps=kw.get("eps", 0.5), dtype=np.float64)
        assert np.abs(a - want).max() < tol
        rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
        assert rc == 0
        r = rew.cpu().numpy()
        assert (U.bits64(r) == U.bits64(r_ref)).all() and (U.bits32(env.state) == U.bits32(o_ref)).all()
        assert (rew32.cpu().numpy() == r_ref.astype(np.float32)).all()
        assert (env.idx == ref.idx()).all() and (env.step == t + 1).all()
        if sums:
            assert abs(blk.sum().item() - r.sum()) < 1e-9 * max(1.0, abs(r).sum())
        _check_ring(ring, pos % ring.capacity, off, 333, n, pre, a, r_ref, o_ref)
        connected |= set(tab_of[(pre[:, 2] == -1) & (o_ref[:, 2] >= 0)].tolist())
        pos += 333
    if noise == "ou":
        assert np.abs(ag.ou_state.cpu().numpy() - X).max() < 1e-5 and np.abs(X).std() > 0.01
    env.close()
    return connected


# BASELINE config 5 as benched (65 536, k_act2), k_act2 with per-tile sums on a ragged batch, and the column-group forms: 8 192 / 4 096
# without sums (k_actg<1, 4, 2, 2> / <1, 4, 2, 3>), 6 005 with sums (the 8-wave form), 3 000 (ragged last 32-env tile)
@pytest.mark.parametrize("n,nsteps,sums,kernel", [(65536, 2, False, "shems::k_act2"), (40000 + 7, 2, True, None),
                                                  (8192, 6, False, "shems::k_actg<1, 4, 2, 2>"), (4096, 3, False, "shems::k_actg<1, 4, 2, 3>"),
                                                  (6005, 3, True, None), (3000, 8, False, "shems::k_actg<1, 4, 2, 3>")])
def test_fused_step_with_per_env_configs_equals_act_then_oracle_step(n, nsteps, sums, kernel):
    torch, S, D = _mods()
    if kernel is not None:
        assert D.act_kernel_name(n) == kernel
    connected = fused_mixed_steps(n, nsteps, sums)
    if nsteps >= 6:                                # the newly-connected-EV branch of next_state!, under several profiles
        assert len(connected) >= 3, connected


@pytest.mark.parametrize("noise", ["ou", "en"])
@pytest.mark.parametrize("n", [65536, 4096])
def test_noise_kinds_inside_the_fused_step_with_per_env_configs(noise, n):
    fused_mixed_steps(n, 3, noise=noise)


# ------------------------------------------------------------------------------------------------------------ every forced form --
_FORMS = {"default": {}, "free": {"SHEMS_ACT_FORM": "2"},
          "ring3": {"SHEMS_ACT_FORM": "3"}, "group8": {"SHEMS_ACT_FORM": "8"}, "split": {"SHEMS_ACT_FORM": "9"},
          "two_per_cu_everywhere": {"SHEMS_ACT_FORM": "12"}, "split_ring2": {"SHEMS_ACT_FORM": "10"}}
# what each form runs at 40 007 / 20 005 / 6 005 envs (128-, 64- and 32-env tiles where the form has them)
_FORM_KERNELS = {
    "default": ("k_act2", "k_act2", "k_actg<1, 4, 2, 2>"),
    "free": ("k_act<4, 4, 2>", "k_act<2, 4, 2>", "k_act<1, 4, 2>"),
    "ring3": ("k_act<4, 4, 2>", "k_act<2, 4, 2>", "k_act<1, 4, 3>"),
    "group8": ("k_act<4, 4, 2>", "k_act<2, 4, 2>", "k_actg<1, 8, 1, 3>"),
    "split": ("k_act<4, 4, 2>", "k_act<2, 4, 2>", "k_actg<1, 4, 2, 3>"),
    "two_per_cu_everywhere": ("k_act2", "k_act2", "k_act2"),
    "split_ring2": ("k_act<4, 4, 2>", "k_act<2, 4, 2>", "k_actg<1, 4, 2, 2>"),
}
_CHILD = r"""
import sys, importlib
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import util as U
T = importlib.import_module("test_fused_configs_gpu")
D = importlib.import_module(U.PKG_NAME + ".ddpg")
for n in {sizes!r}:
    print("KERNEL", n, D.act_kernel_name(n), flush=True)
    T.{fn}(n, *{args!r})
print("DONE", flush=True)
"""


def _run_forms(forms, fn, sizes, args=()):
    """Run T.fn(n, *args) for every n under every form, one child process per form (the form is read once per process), all at once."""
    script = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), sizes=tuple(sizes), fn=fn, args=tuple(args))
    procs = {}
    for name in forms:
        e = dict(os.environ)
        e.update(_FORMS[name])
        e["OMP_NUM_THREADS"] = "2"                 # the children share the host's cores for the float64 references
        procs[name] = subprocess.Popen([sys.executable, "-c", script], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    try:
        for name, pr in procs.items():
            so, se = pr.communicate(timeout=300)
            assert pr.returncode == 0 and "DONE" in so, f"{name}: {se[-3000:]}"
            out[name] = [ln.split(" ", 2)[2] for ln in so.splitlines() if ln.startswith("KERNEL")]
    finally:
        for pr in procs.values():
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    return out


def test_every_forced_form_meets_the_oracle_with_per_env_configs():
    """Each form of the act kernel (the all-forms byte test's list) does three mixed-config fused steps at 40 007, 20 005 and 6 005
    envs and is held to the float64 actions, the oracle's transitions and the ring window -- not only to the other forms' bytes."""
    got = _run_forms(list(_FORMS), "fused_mixed_steps", (40000 + 7, 20000 + 5, 6000 + 5), (3,))
    for name, want in _FORM_KERNELS.items():
        assert got[name] == ["shems::" + k for k in want], name


# ------------------------------------------------------------------------------------------------ table edges of every config --
def _edge_layout(n, nrow_env, rng):
    """Start rows: envs of every config on row 1, on nrow - 2 / nrow - 1 of their own table (the last two valid steps) and on nrow
    (one past the end), placed at the first and last env of 32-, 64- and 128-env tiles; the rest on random rows inside."""
    e = np.arange(n)
    kind = np.full(n, -1)
    edge = (e % 32 == 0) | (e % 32 == 31) | (e == n - 1)
    kind[edge] = (e[edge] // 32 + e[edge] // 64) % 4
    kind[:240] = e[:240] // 60                      # with config i mod 60: every (config, edge) pair, tiles 0..7
    idx = rng.integers(1, nrow_env - 72, n)
    for k, off in enumerate((None, 2, 1, 0)):
        idx[kind == k] = 1 if off is None else nrow_env[kind == k] - off
    return idx.astype(np.int32), kind


def bounds_edges_of_every_config(n):
    """One fused step from the table edges of every config: envs with a next row step bit-exact with the oracle, envs past their own
    table's end keep state, idx and step (the oracle's batch step leaves them alone as well), the step raises BoundsError, and the
    handle steps a valid batch correctly afterwards -- k_step's contract (test_env_gpu.py)."""
    torch, S, D = _mods()
    env, ref, tabs, cfgs, co, tab_of = U.mixed_batches(n)
    env.use_torch_stream()
    nrow = np.array([t.shape[0] for t in tabs])
    assert set(nrow.tolist()) == {4319, 4320}
    nrow_env = nrow[tab_of]
    rng = np.random.default_rng(n)
    idx, kind = _edge_layout(n, nrow_env, rng)
    for k in range(4):
        assert set(co[kind == k].tolist()) == set(range(len(cfgs)))
    soc = (rng.random(n) * 6.75).astype(np.float32)
    st = np.empty((n, 9), np.float32)
    for t in range(len(tabs)):
        m = tab_of == t
        st[m] = U.obs_of_rows(tabs[t], idx[m], soc[m])
    step0 = rng.integers(0, 72, n).astype(np.int32)
    env.reset_(0, episode=0)
    env.state, env.idx, env.step = st, idx, step0
    ref.set_state(st, idx, step0)
    ag = D.Agent(seed=31)
    p = _actor(D, 31)
    ag.set_params(actor=p)
    lo, hi = st.min(0), st.max(0)
    ag.set_norm(lo, hi)
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    rew = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    ag.act_step(env, train=True, tick=3, a_out=a_out, rewards=rew)
    with pytest.raises(S.BoundsError):
        env.check_error()
    a = a_out.cpu().numpy()
    assert np.abs(a - DO.act(p, st, lo, hi, True, seed=31, tick=3, dtype=np.float64)).max() < 5e-6 + ATOL
    rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
    assert rc == -1
    past = kind == 3
    ok = ~past
    assert (U.bits32(env.state) == U.bits32(o_ref)).all()
    assert (U.bits32(env.state[past]) == U.bits32(st[past])).all()
    assert (U.bits64(rew.cpu().numpy()[ok]) == U.bits64(r_ref[ok])).all()
    assert (env.idx[ok] == idx[ok] + 1).all() and (env.step[ok] == step0[ok] + 1).all()
    assert (env.idx[past] == idx[past]).all() and (env.step[past] == step0[past]).all()
    assert (env.idx == ref.idx()).all() and (env.step == ref.steps()).all()
    # the handle goes on: a valid batch steps correctly
    env.reset_(7, episode=1)
    st1 = env.state
    ref.set_state(st1, env.idx, env.step)
    ag.act_step(env, train=True, tick=4, a_out=a_out, rewards=rew)
    env.check_error()
    a = a_out.cpu().numpy()
    rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
    assert rc == 0 and (U.bits64(rew.cpu().numpy()) == U.bits64(r_ref)).all() and (U.bits32(env.state) == U.bits32(o_ref)).all()
    assert (env.idx == ref.idx()).all()
    env.close()


@pytest.mark.parametrize("n", [65536, 8192, 4096])
def test_fused_step_at_the_table_edges_of_every_config(n):
    bounds_edges_of_every_config(n)


def test_free_running_form_at_the_table_edges_of_every_config():
    got = _run_forms(["free"], "bounds_edges_of_every_config", (65536, 4096))
    assert got["free"] == ["shems::k_act<4, 4, 2>", "shems::k_act<1, 4, 2>"]


# ------------------------------------------------------------------------------------------------------------- learner groups --
# what the dispatcher runs for each shape (Flux order: tiles that never straddle two learners; beyond the split forms' 512 tiles the
# 8-wave form; one learner above 8 192 envs: k_act2.  Tiled: the free-running k_act, 64-env tiles where the block allows them)
_GROUP_KERNELS = {(40, 128, False): "k_actg<1, 4, 2, 2>", (12, 32, False): "k_actg<1, 4, 2, 3>", (6, 96, False): "k_actg<1, 4, 2, 3>",
                  (300, 96, False): "k_actg<1, 8, 1, 3>", (520, 64, False): "k_act<2, 4, 2>", (1, 16384, False): "k_act2",
                  (40, 128, True): "k_act<1, 4, 2>", (12, 32, True): "k_act<1, 4, 2>", (6, 96, True): "k_act<1, 4, 2>",
                  (300, 96, True): "k_act<1, 4, 2>", (520, 64, True): "k_act<2, 4, 2>", (1, 16384, True): "k_act<2, 4, 2>"}


@pytest.mark.parametrize("tiled", [False, True], ids=["flux", "tiled"])
@pytest.mark.parametrize("L,E", [(40, 128), (12, 32), (6, 96), (300, 96), (520, 64), (1, 16384)])
def test_grouped_fused_step_meets_the_oracle_per_learner(L, E, tiled):
    """The thesis grid (learner l on profile l mod 10, weight point l mod 6; tables of 4 319 / 4 320 rows): three grouped steps, each
    learner's env block against its own actor and norms in float64, the noise by global env index, the oracle bit for bit, and each
    learner's ring window."""
    torch, S, D = _mods()
    G = importlib.import_module(U.PKG_NAME + ".group")
    n = L * E
    env, ref, tabs, cfgs, co, tab_of = U.mixed_batches(n, co=U.learner_grid_cfgs(L, E))
    env.use_torch_stream()
    grp = G.LearnerGroup(L, E, seed=7, rng_seed=11, capacity=720, form="throughput" if tiled else "latency")
    assert grp.tiled == tiled
    env.reset_(3, episode=0)
    st0 = env.state
    ref.set_state(st0, env.idx)
    off, na = grp.layout["actor"]
    grp.slab[:, off + 128000:off + 129000] *= 60.0
    grp.flux_changed()
    lo = np.stack([st0[l * E:(l + 1) * E].min(0) for l in range(L)])
    hi = np.stack([st0[l * E:(l + 1) * E].max(0) for l in range(L)]) + 0.25
    for l, ag in enumerate(grp.learners):
        ag.set_norm(lo[l], hi[l])
    actors = grp.slab[:, off:off + na].cpu().numpy()
    a_out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    for t in range(3):
        grp.tick = t
        pre = env.state
        pos = grp.rings[0].pos
        wc, woff = grp.ring_window(72, None)
        grp.act_step(env, train=True, tick=t, a_out=a_out, window=(pos, wc, woff))
        env.check_error()
        a = a_out.cpu().numpy()
        zn = DO.gauss_noise(grp.rng_seed, t, n)
        for l in range(L):
            sl = slice(l * E, (l + 1) * E)
            clean = DO.act(actors[l], pre[sl], lo[l], hi[l], False, dtype=np.float64)
            assert np.abs(a[sl] - np.clip(clean + 0.1 * zn[sl].astype(np.float64), -1.0, 1.0)).max() < 2e-5, l
        rc, r_ref, o_ref, _ = ref.step(oracle_c.scale_action(a), 0)
        assert rc == 0 and (U.bits32(env.state) == U.bits32(o_ref)).all()
        assert (env.idx == ref.idx()).all() and (env.step == t + 1).all()
        for l, ring in enumerate(grp.rings):
            sl = slice(l * E, (l + 1) * E)
            _check_ring(ring, pos, woff, wc, E, pre[sl], a[sl], r_ref[sl], o_ref[sl])
    assert G.group_act_kernel_name(n, E, tiled) == "shems::" + _GROUP_KERNELS[(L, E, tiled)]
    env.close()


# ------------------------------------------------------------------------------------------------------------- tracking pass --
def test_tracking_passes_with_a_config_per_env():
    """harness.inference_many on ten envs, env i on charger profile i with its own actor: the whole 1 439-hour pass (eval tables padded
    to 1 440 rows) row for row against the oracle on that env's profile, equal to the single-env pass on that profile alone; the
    rule-based pass on the same batch against the oracle's rule episode."""
    torch, S, D = _mods()
    H = importlib.import_module(U.PKG_NAME + ".harness")
    steps = 1439
    w, pot = 0.04, 2.0
    tabs, _, co = S.mixed_profile_setup(10, split="eval", sweep=((w, pot),))
    assert (co == np.arange(10)).all() and {t.shape[0] for t in tabs} == {1439, 1440}
    tabs = [S.tables.pad_rows(t, steps + 1) for t in tabs]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, row0[k], tabs[k].shape[0], w, pot) for k, c in enumerate(U.CHARGER_IDS)]
    env = S.ShemsBatch(10, steps, tabs, cfgs, co)
    actors = np.stack([_actor(D, 40 + k) for k in range(10)])
    allrows = np.concatenate(tabs)
    st = allrows[:, [1, 1, 0, 2, 3, 4, 5, 6, 7]].copy()
    st[:, 0] = np.linspace(0, 6.75, len(st))
    lo, hi = st.min(0), st.max(0)
    tot, res = H.inference_many(env, actors, lo, hi, num_steps=steps)
    assert res.shape == (10, steps, 23) and len({float(x) for x in tot}) == 10
    rule = [H.inference(env, track=-0.5, num_steps=steps, which=k) for k in range(10)]
    env.close()
    ag = D.Agent(seed=1)
    ag.set_norm(lo, hi)
    for k, c in enumerate(U.CHARGER_IDS):
        prof = oracle_c.profile(c, w, pot)
        ref = oracle_c.Batch(1, steps, tabs[k], prof)
        ref.reset(True)
        for t in range(steps):
            rc, _, _, rr = ref.step(res[k][t, [21, 2]].astype(np.float32)[None], 1, want_results=True)
            assert rc == 0 and (U.bits64(rr[0]) == U.bits64(res[k][t])).all(), (c, t)
        one = S.ShemsBatch(1, steps, [tabs[k]], [S.make_config(c, 0, tabs[k].shape[0], w, pot)])
        ag.set_params(actor=actors[k])
        t1, r1 = H.inference(one, ag, track=1, num_steps=steps)
        one.close()
        assert (U.bits64(r1) == U.bits64(res[k])).all() and t1[0] == tot[k], c
        tot_ref, res_ref = oracle_c.Batch(1, steps, tabs[k], prof).rule_episode(0, steps, want_results=True)
        assert (U.bits64(rule[k][1]) == U.bits64(res_ref)).all() and rule[k][0][k] == tot_ref, c

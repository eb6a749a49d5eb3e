"""The input template's grid (RL-SHEMS/input.jl:58-100: 27 points over MEM_SIZE, BATCH_SIZE and (L1, L2, gamma, sigma, theta), all with
Ornstein-Uhlenbeck noise) as ONE wide learner group, measured: (a) the 27 points x 4 seeds as one LearnerGroup(form="wide",
noise_type="ou", capacity=30000) -- vector steps of one fused act/step + one replay() of every learner, (b) a slice of the same learners
one Agent at a time (its own ring of MEM_SIZE, the same envs per learner, act_step + replay per step; extrapolated to the group's
learner count).  Writes profiles/r10_group_input_grid.json (or --out) with learner-updates/s for both and the ratio.

    python tools/group_input_demo.py [--envs 32] [--seeds 4] [--steps 72] [--out PATH]

--step-ab: the cost of the *_x fused step next to the d_hp one.  400 learners x 128 envs with uniform records, one group on
shems_act_step_group_dev with d_hp (k_act_hp) and one on shems_act_step_group_x_dev (k_act_x; a mem_size = capacity record takes the
path), their launches in alternating runs of one process, timed with HIP events here and named apart by a profiler:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/group_input_demo.py --step-ab
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
EP_LEN = 72                        # hours of a training episode (the env batches here are built with maxsteps 72)


def _env(S, n):
    tab = S.tables.synthetic_table("train", 98)
    return S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()


def timed(torch, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_group(S, torch, G, recs, E, steps):
    env = _env(S, len(recs) * E)
    t0 = time.time()
    grp = G.LearnerGroup(len(recs), E, seed=1231, rng_seed=7, capacity=G.INPUT_CAPACITY, form="wide", noise_type="ou", hparams=recs)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    env.reset_(3, episode=1)
    torch.cuda.synchronize()
    setup_s = time.time() - t0

    def step():
        if grp.tick % EP_LEN == 0:                 # an episode has 72 hours: reset before the 73rd step
            env.reset_(3, episode=1 + grp.tick // EP_LEN)
        grp.act_step(env, train=True, tick=grp.tick, window=(grp.rings[0].pos, *grp.ring_window(EP_LEN, 1)))
        grp.replay()
        grp.tick += 1
    ms = timed(torch, step, steps)
    env.check_error()
    ok = bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())
    out = dict(form="one wide group, noise_type ou, per-learner mem_size", learners=len(recs), envs_per_learner=E, ring_capacity=grp.capacity,
               hidden=list(grp.hidden), max_batch=grp.max_batch,
               launches_per_step_by_construction="4 (fused step) + 24 (replay) of the library + 1 elementwise add advancing `pushed`; not counted here",
               setup_s=round(setup_s, 2), ms_per_step=round(ms, 4),
               learner_updates_per_s=round(len(recs) / (ms * 1e-3), 1), finite=ok, steps=steps)
    env.close()
    return out


def baseline(S, torch, D, recs, E, learners, steps):
    env = _env(S, E)
    total_ms = 0.0
    for k in range(learners):
        r = recs[(k * len(recs)) // learners]
        ag = D.Agent(seed=100 + k, hidden=r["hidden"], wide=True, noise_type="ou", sigma=r["sigma"], mu=r["mu"], theta=r["theta"])
        ag.batch, ag.gamma, ag.tau = r["batch"], r["gamma"], r["tau"]
        ring = D.ReplayRing(r["mem_size"])
        ag.populate_memory(env, ring, seed=5)
        ag.min_max_buffer(ring)
        ag._ensure_ou(E)
        tick = [0]

        def step():
            if tick[0] % EP_LEN == 0:
                env.reset_(3, episode=1 + tick[0] // EP_LEN)
            ag.act_step(env, train=True, tick=tick[0], ring=ring, window=D.RingWindow(ring.pos, 1, 0))
            ring.pushed += 1
            ag.replay(ring, tick=tick[0])
            tick[0] += 1
        total_ms += timed(torch, step, steps)
        env.check_error()
    ms = total_ms / learners
    env.close()
    return dict(form="one Agent at a time (single-learner wide path, noise_type ou, its own ring)", sampled_learners=learners, steps_each=steps,
                ms_per_learner_step=round(ms, 4), learner_updates_per_s=round(1e3 / ms, 1), extrapolated_to_learners=len(recs),
                note="the sampled learners' mean time per step; a round of the group's learners takes this x the learner count")


def step_ab(S, torch, G, L, E, runs, reps):
    cap = 400
    groups = {}
    for name, recs in (("d_hp", [{}] * L), ("x", [{"mem_size": cap}] + [{}] * (L - 1))):
        env = _env(S, L * E)
        grp = G.LearnerGroup(L, E, seed=1231, rng_seed=7, capacity=cap, hparams=recs)
        grp.populate_memory(env, seed=5)
        grp.min_max_buffer()
        env.reset_(3, episode=1)
        groups[name] = (env, grp)
    times = {k: [] for k in groups}
    for run in range(runs):
        for name, (env, grp) in groups.items():
            def act():
                grp.act_step(env, train=True, tick=grp.tick, window=(grp.rings[0].pos, *grp.ring_window(EP_LEN)))
                grp.tick += 1
            assert reps + 2 <= EP_LEN                  # warm-up + timed launches of a run stay inside one episode
            env.reset_(3, episode=1 + run)
            times[name].append(round(timed(torch, act, reps) * 1e3, 3))
    for env, _ in groups.values():
        env.check_error()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return dict(learners=L, envs_per_learner=E, kernel=G.group_act_kernel_name(L * E, E, True), runs=runs, launches_per_run=reps,
                us_per_step_d_hp_path=times["d_hp"], us_per_step_x_path=times["x"], median_us=med,
                x_over_d_hp=round(med["x"] / med["d_hp"], 4),
                note="HIP events around each run's launches; the x path includes the one-element-per-learner advance of `pushed`")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=72)
    ap.add_argument("--baseline-learners", type=int, default=9)
    ap.add_argument("--step-ab", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_group_input_grid.json"))
    a = ap.parse_args()
    import importlib
    import torch
    S = importlib.import_module(PKG)
    D = importlib.import_module(PKG + ".ddpg")
    G = importlib.import_module(PKG + ".group")
    if a.step_ab:
        print(json.dumps(step_ab(S, torch, G, 400, 128, 5, 48)), flush=True)
        return
    recs = G.input_grid(G.INPUT_ALL, seeds=a.seeds)[0]
    res = dict(device=torch.cuda.get_device_name(0), envs_per_learner=a.envs, seeds=a.seeds)
    res["a_27_points_one_group"] = run_group(S, torch, G, recs, a.envs, a.steps)
    print(json.dumps(res["a_27_points_one_group"]), flush=True)
    res["b_one_agent_at_a_time"] = baseline(S, torch, D, recs, a.envs, a.baseline_learners, a.steps)
    print(json.dumps(res["b_one_agent_at_a_time"]), flush=True)
    res["a_over_b_learner_updates"] = round(res["a_27_points_one_group"]["learner_updates_per_s"] /
                                            res["b_one_agent_at_a_time"]["learner_updates_per_s"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

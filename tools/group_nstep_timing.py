"""What multi-step returns cost (not a test; nothing is asserted):

  fold        ONE CALL of the fold alone (nstep_fold / NStepWindow.fold) between two HIP events after a warm-up call, the median of five:
              shems_nstep_group_fold_dev at 400 learners x 128 households (window 128, n = 3) and shems_nstep_fold_dev for one Agent at
              window 333 (n = 3), each at an hour that pushes (hour >= n - 1).  The interval holds the host's enqueue path of the call
              (Python views, ctypes records) as well as the kernel: it is a call time, an upper bound of the kernel's, not a kernel time
              (that needs a kernel trace, which this tool does not take);
  step        one training vector step (the fused act/step launch and, with n-step, the fold behind it) with n_step = 1 and with
              n_step = 3: the two groups (the two agents) live in one process, the calls ALTERNATE after a warm-up call of each, every
              call between its own pair of events, medians of five;
  populate    populate_memory both ways (host wall time around a synchronize: it is a handful of launches), ring 24 000.

    python tools/group_nstep_timing.py [out.json]
    (default profiles/r22_nstep_timing.json; needs the GPU, does not read oracle/)
"""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
D = importlib.import_module(PKG + ".ddpg")
G = importlib.import_module(PKG + ".group")

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r22_nstep_timing.json")
CAP, IDS, N = 24000, (1, 2, 3, 4, 5, 6, 7, 8, 9, 98), 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                           # us


def median_of_five(fn):
    fn()                                                    # the warm-up call
    torch.cuda.synchronize()
    t = [timed(fn) for _ in range(5)]
    return {"median_us": statistics.median(t), "spread_us": max(t) - min(t), "all_us": t}


def alternating(fns, n=5):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    return {k: {"median_us": statistics.median(v), "spread_us": max(v) - min(v), "all_us": v} for k, v in t.items()}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3                  # ms


def group_env(L, E):
    tabs = [S.tables.synthetic_table("train", c) for c in IDS]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, int(row0[k]), tabs[k].shape[0]) for k, c in enumerate(IDS)]
    co = ((np.arange(L * E) // E) % len(IDS)).astype(np.uint16)
    return S.ShemsBatch(L * E, 72, tabs, cfgs, co).use_torch_stream()


def group_shape(L, E):
    env = group_env(L, E)
    grps, pop = {}, {}
    for n in (1, N):
        g = G.LearnerGroup(L, E, seed=1231, rng_seed=99, capacity=CAP, form="throughput", n_step=n)
        pop[n] = wall(lambda: g.populate_memory(env))
        g.min_max_buffer()
        grps[n] = g
    env.reset_(7, episode=1)
    hour = [0]

    def step(n):
        g = grps[n]
        g.act_step(env, train=True, tick=hour[0], window=(g.rings[0].pos, *g.ring_window(72, E)))
        if n > 1:
            g.nstep_fold(N - 1 + hour[0] % (72 - N))         # (an hour that pushes; the env itself is not reset between calls)
        hour[0] += 1
    rec = {"learners": L, "households_per_learner": E, "window": E, "n_step": N, "ring_capacity": CAP,
           "step": alternating({"n_step_1": lambda: step(1), f"n_step_{N}": lambda: step(N)})}
    g = grps[N]
    g.act_step(env, train=True, tick=0, window=(g.rings[0].pos, E, 0))
    rec["fold_alone"] = median_of_five(lambda: g.nstep_fold(N - 1))
    rec["populate_memory_ms"] = {"n_step_1": pop[1], f"n_step_{N}": pop[N]}
    rec["step"]["fold_share_of_the_step"] = rec["fold_alone"]["median_us"] / rec["step"][f"n_step_{N}"]["median_us"]
    env.close()
    return rec


def agent_shape(n_envs, window):
    tab = S.tables.synthetic_table("train", 98)
    env = S.ShemsBatch(n_envs, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    ags, rings, pop = {}, {}, {}
    for n in (1, N):
        ags[n], rings[n] = D.Agent(seed=1231, n_step=n), D.ReplayRing(CAP)
        pop[n] = wall(lambda: ags[n].populate_memory(env, rings[n], seed=5))
        ags[n].min_max_buffer(rings[n])
    env.reset_(7, episode=1)
    nsw = ags[N].nstep_window(window)
    hour = [0]

    def step(n):
        ag, ring = ags[n], rings[n]
        if n == 1:
            ag.act_step(env, train=True, tick=hour[0], ring=ring, window=D.RingWindow(ring.pos, window, (hour[0] * window) % n_envs))
            ring.pushed += window
        else:
            ag.act_step(env, train=True, tick=hour[0], ring=nsw.stage, window=D.RingWindow(*nsw.window))
            nsw.fold(ring, N - 1 + hour[0] % (72 - N))
        hour[0] += 1
    rec = {"envs": n_envs, "window": window, "n_step": N, "ring_capacity": CAP,
           "step": alternating({"n_step_1": lambda: step(1), f"n_step_{N}": lambda: step(N)})}
    rec["fold_alone"] = median_of_five(lambda: nsw.fold(rings[N], N - 1))
    rec["populate_memory_ms"] = {"n_step_1": pop[1], f"n_step_{N}": pop[N]}
    env.close()
    return rec


props = torch.cuda.get_device_properties(0)
doc = {"what": "one call of the n-step fold alone between two HIP events (host enqueue path + kernel: a call time, not a kernel time), a training vector step with and without n-step (alternating calls in one process), and "
               "populate_memory both ways; HIP events after a warm-up call, medians of five",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "group_400x128": group_shape(400, 128), "agent_window_333": agent_shape(65536, 333)}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps({k: {"fold_alone_us": v["fold_alone"]["median_us"], "step_us": {a: b["median_us"] for a, b in v["step"].items() if isinstance(b, dict)},
                      "populate_ms": v["populate_memory_ms"]} for k, v in doc.items() if isinstance(v, dict)}))
print("written", out_path)

"""Time one learner update by HIP events, one mode per process, so that parent and new builds can alternate as processes:

    python tools/per_update_time.py ddpg | per | sample  [--updates N] [--envs N]

The setting is tools/td3_update_time.py's (TrainWorkload's at 65 536 envs in Flux order): the synthetic Charger98 train table, a ring
of 24 000 transitions filled by populate_memory, the normalisation of min_max_buffer, seed 1231, batch 120.  After 200 warm-up updates,
N updates (default 4 000) are enqueued back to back between two events; the figure is their mean in microseconds.  ddpg = Agent.replay
on a ReplayRing (with SHEMS_HIP_LIB pointing at a parent build: the parent's); per = Agent.replay on a PrioritizedRing (the six
launches of shems_ddpg_update_per, alpha 0.6, beta 0.4); sample = the sampler launch alone (shems_per_sample_dev) on that ring after
the warm-up updates have written its priorities.  Prints one JSON line.  Needs the GPU.
"""
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
D = importlib.import_module(PKG + ".ddpg")


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


mode = sys.argv[1] if len(sys.argv) > 1 else "ddpg"
if mode not in ("ddpg", "per", "sample"):
    raise SystemExit(__doc__)
updates, envs, warm = arg("--updates", 4000), arg("--envs", 65536), 200
tab = S.tables.synthetic_table("train", 98)
env = S.ShemsBatch(envs, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
agent = D.Agent(seed=1231, rng_seed=7)
agent.batch = 120
ring = D.ReplayRing(24000) if mode == "ddpg" else D.PrioritizedRing(24000)
agent.populate_memory(env, ring, seed=7)
agent.min_max_buffer(ring, 24000, seed=7)
env.close()
for t in range(warm):
    agent.replay(ring, tick=t)
torch.cuda.synchronize()
if mode == "sample":
    R = importlib.import_module(PKG + ".replay")
    L, ps, st = R._declare_per(), ring.per_struct(), agent._stream()
    step = lambda t: S._capi.check(L.shems_per_sample_dev(C.byref(ps), ring.capacity, len(ring), 0, 0, 7, t, agent.batch, st))
else:
    step = lambda t: agent.replay(ring, tick=t)
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter()
a.record()
for t in range(updates):
    step(warm + t)
b.record()
t1 = time.perf_counter()                                   # the host's enqueue time: if it is not well below the device's, the loop is host-bound
b.synchronize()
finite = all(bool(torch.isfinite(getattr(agent, k)).all()) for k in ("actor", "critic", "actor_t", "critic_t"))
print(json.dumps({"mode": mode, "lib": S._capi.LIB_PATH.replace(ROOT, "."), "updates": updates, "us_per_update": 1e3 * a.elapsed_time(b) / updates,
                  "host_enqueue_us_per_update": 1e6 * (t1 - t0) / updates, "finite": finite}), flush=True)

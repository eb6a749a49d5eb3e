"""Time one learner update by HIP events, one mode per process, so that parent and new builds can alternate as processes:

    python tools/td3_update_time.py ddpg | td3_policy | td3_critic | td3_d2  [--updates N] [--envs N]

The setting is TrainWorkload's at 65 536 envs in Flux order: the synthetic Charger98 train table, a ring of 24 000 transitions filled
by populate_memory, the normalisation of min_max_buffer, seed 1231, batch 120.  After 200 warm-up updates, N updates (default 4 000)
are enqueued back to back between two events; the figure is their mean in microseconds (the device time per update as the training
loop sees it: dependent launches, nothing between them).  ddpg = Agent.replay (with SHEMS_HIP_LIB pointing at a parent build: the
parent's); td3_policy / td3_critic = TD3Agent.replay with update_policy forced on / off; td3_d2 = the schedule with policy_delay 2 --
the mix a profiler run names kernel by kernel.  Prints one JSON line.  Needs the GPU.
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import time

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
D = importlib.import_module(PKG + ".ddpg")


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


mode = sys.argv[1] if len(sys.argv) > 1 else "ddpg"
if mode not in ("ddpg", "td3_policy", "td3_critic", "td3_d2"):
    raise SystemExit(__doc__)
updates, envs, warm = arg("--updates", 4000), arg("--envs", 65536), 200
tab = S.tables.synthetic_table("train", 98)
env = S.ShemsBatch(envs, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
if mode == "ddpg":
    agent = D.Agent(seed=1231, rng_seed=7)
else:
    T = importlib.import_module(PKG + ".td3")
    agent = T.TD3Agent(seed=1231, rng_seed=7, policy_delay=2)
agent.batch = 120
ring = D.ReplayRing(24000)
agent.populate_memory(env, ring, seed=7)
agent.min_max_buffer(ring, 24000, seed=7)
env.close()
kw = {"ddpg": {}, "td3_policy": {"update_policy": True}, "td3_critic": {"update_policy": False}, "td3_d2": {}}[mode]
for t in range(warm):
    agent.replay(ring, tick=t, **kw)
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter()
a.record()
for t in range(updates):
    agent.replay(ring, tick=warm + t, **kw)
b.record()
t1 = time.perf_counter()                                   # the host's enqueue time: if it is not well below the device's, the loop is host-bound
b.synchronize()
finite = all(bool(torch.isfinite(getattr(agent, k)).all()) for k in ("actor", "critic", "actor_t", "critic_t"))
print(json.dumps({"mode": mode, "lib": os.path.basename(S._capi.LIB_PATH), "updates": updates, "us_per_update": 1e3 * a.elapsed_time(b) / updates,
                  "host_enqueue_us_per_update": 1e6 * (t1 - t0) / updates,
                  "finite": finite}), flush=True)

"""Time one learner update with and without the behaviour-regularised actor loss by HIP events, one mode per process, so that the
parent's and this build's library can alternate as processes (tools/td3_update_time.py's manner):

    python tools/bc_update_time.py ddpg | ddpg_bc | td3_policy | td3_policy_bc  [--updates N] [--envs N]
    python tools/bc_update_time.py all --parent-lib PATH [--rounds 3] [--out profiles/r24_bc_update_time.jsonl]

The setting is TrainWorkload's at 65 536 envs in Flux order: the synthetic Charger98 train table, a ring of 24 000 transitions filled
by populate_memory, the normalisation of min_max_buffer, seed 1231, batch 120.  After 200 warm-up updates, N updates (default 4 000)
are enqueued back to back between two events; the figure is their mean in microseconds.  ddpg = Agent.replay (with SHEMS_HIP_LIB
pointing at a parent build: the parent's); ddpg_bc = the same with bc = BC(2.5, 1); td3_policy / td3_policy_bc = TD3Agent.replay with
update_policy forced on, without / with bc.  One mode prints one JSON line.

`all` runs the five modes (ddpg on the parent's library first) as fresh child processes, alternating, `--rounds` times, appends every
line to --out and ends with one line of medians per mode and the round-to-round spread (max - min) of each.  Needs the GPU.
"""
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
MODES = ("ddpg", "ddpg_bc", "td3_policy", "td3_policy_bc")


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def drive():
    parent = arg("--parent-lib", None, str)
    if not parent or not os.path.exists(parent):
        raise SystemExit("all: --parent-lib PATH (the parent commit's libshems_hip.so) is needed")
    rounds, out = arg("--rounds", 3), arg("--out", os.path.join(ROOT, "profiles", "r24_bc_update_time.jsonl"), str)
    extra = [a for k in ("--updates", "--envs") if k in sys.argv for a in (k, sys.argv[sys.argv.index(k) + 1])]
    runs = [("ddpg_parent", "ddpg", parent)] + [(m, m, None) for m in MODES]
    got = {name: [] for name, _, _ in runs}
    lines = []
    for r in range(rounds):
        for name, mode, lib in runs:
            env = dict(os.environ)
            env.pop("SHEMS_HIP_LIB", None)
            if lib:
                env["SHEMS_HIP_LIB"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), mode] + extra, env=env, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:                      # a failed child ends the run: nothing more is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{name}: exit status {p.returncode}")
            rec = dict(json.loads(p.stdout.strip().split("\n")[-1]), run=name, round=r)
            got[name].append(rec["us_per_update"])
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    summary = {"summary": {n: {"median_us": statistics.median(v), "spread_us": max(v) - min(v), "runs": v} for n, v in got.items()}, "rounds": rounds}
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "a") as fh:
        for rec in lines + [summary]:
            fh.write(json.dumps(rec) + "\n")


def one(mode):
    sys.path.insert(0, ROOT)
    import torch
    S = importlib.import_module(PKG)
    D = importlib.import_module(PKG + ".ddpg")
    updates, envs, warm = arg("--updates", 4000), arg("--envs", 65536), 200
    tab = S.tables.synthetic_table("train", 98)
    env = S.ShemsBatch(envs, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    if mode.startswith("ddpg"):
        agent = D.Agent(seed=1231, rng_seed=7)
    else:
        T = importlib.import_module(PKG + ".td3")
        agent = T.TD3Agent(seed=1231, rng_seed=7, policy_delay=2)
    agent.batch = 120
    if mode.endswith("_bc"):
        agent.bc = D.BC(2.5, 1.0)
    ring = D.ReplayRing(24000)
    agent.populate_memory(env, ring, seed=7)
    agent.min_max_buffer(ring, 24000, seed=7)
    env.close()
    kw = {} if mode.startswith("ddpg") else {"update_policy": True}
    for t in range(warm):
        agent.replay(ring, tick=t, **kw)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for t in range(updates):
        agent.replay(ring, tick=warm + t, **kw)
    b.record()
    t1 = time.perf_counter()                               # the host's enqueue time: if it is not well below the device's, the loop is host-bound
    b.synchronize()
    finite = all(bool(torch.isfinite(getattr(agent, k)).all()) for k in ("actor", "critic", "actor_t", "critic_t"))
    print(json.dumps({"mode": mode, "lib": os.path.basename(S._capi.LIB_PATH), "updates": updates, "us_per_update": 1e3 * a.elapsed_time(b) / updates,
                      "host_enqueue_us_per_update": 1e6 * (t1 - t0) / updates, "finite": finite}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "all":
        drive()
    elif mode in MODES:
        one(mode)
    else:
        raise SystemExit(__doc__)

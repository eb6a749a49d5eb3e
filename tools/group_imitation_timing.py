"""What the grouped supervised and critic-only updates cost (not a test): at 400 learners x 128 households and at 32 x 2 048, the three
updates of a shape in the same process,

  * one LearnerGroup.clone, one LearnerGroup.evaluate and one LearnerGroup.replay -- HIP events after a warm-up call, the median of
    five -- and whether each new update lies below replay()'s median by more than the spread (max - min) of replay()'s five runs;
  * the same work as single-learner Agent.clone / Agent.evaluate calls, measured on 20 stand-alone agents and EXTRAPOLATED to the
    group's width (count / 20 x the measured time), as DESIGN.md 4d does;
  * at 400 learners, what one imitation.dagger_group round costs on the host side (tracking, audit, the per-learner demos calls):
    round 0 (the foresight passes) and round 1 (the actors' passes and the audit), 1 438 hours per learner on the synthetic eval tables.

    python tools/group_imitation_timing.py [out.json] [--loop N]
    (default profiles/r17_group_imitation_timing.json; --loop N: no measurement, N calls of each update at 400 x 128 for a profiler's
    kernel statistics; needs the GPU, does not read oracle/)
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
H = importlib.import_module(PKG + ".harness")
I = importlib.import_module(PKG + ".imitation")

loop = int(sys.argv[sys.argv.index("--loop") + 1]) if "--loop" in sys.argv else 0
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--loop"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r17_group_imitation_timing.json")
CAP, SINGLES, IDS = 7200, 20, (1, 2, 3, 4, 5, 6, 7, 8, 9, 98)


def median_of_five(fn):
    fn()                                                    # the warm-up call
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(t), "spread_ms": max(t) - min(t), "all_ms": t}


def group(L, E):
    """The thesis grid's shape: learner l on charger profile l mod 10, rings of CAP random-action transitions, demonstrations = the
    rings' own (s, a) in a GroupDemos outside the slabs."""
    tabs = [S.tables.synthetic_table("train", c) for c in IDS]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, int(row0[k]), tabs[k].shape[0]) for k, c in enumerate(IDS)]
    co = ((np.arange(L * E) // E) % len(IDS)).astype(np.uint16)
    env = S.ShemsBatch(L * E, 72, tabs, cfgs, co).use_torch_stream()
    grp = G.LearnerGroup(L, E, seed=1231, rng_seed=99, capacity=CAP, form="throughput")
    grp.populate_memory(env)
    grp.min_max_buffer()
    env.close()
    demos = I.GroupDemos(L, CAP)
    for ring, dm in zip(grp.rings, demos.rings):
        dm.s.copy_(ring.s); dm.a.copy_(ring.a)
        dm.pushed = ring.pushed
    return grp, demos


def shape(L, E):
    grp, demos = group(L, E)
    rec = {"learners": L, "households_per_learner": E, "ring_capacity": CAP, "tiled": grp.tiled,
           "replay": median_of_five(grp.replay), "clone": median_of_five(lambda: grp.clone(demos)), "evaluate": median_of_five(grp.evaluate)}
    for k in ("clone", "evaluate"):
        rec[k]["below_replay_by_ms"] = rec["replay"]["median_ms"] - rec[k]["median_ms"]
        rec[k]["subset_bar_met"] = rec[k]["below_replay_by_ms"] > rec["replay"]["spread_ms"]
    # the same work learner by learner: SINGLES stand-alone agents on rings of their own, extrapolated to L
    agents = []
    for l in range(SINGLES):
        ag, ring = D.Agent(seed=1231 + l), D.ReplayRing(CAP)
        for k in ("s", "a", "r", "s2", "done"):
            getattr(ring, k).copy_(getattr(grp.rings[l], k))
        ring.pushed = CAP
        ag.s_min.copy_(grp.learners[l].s_min); ag.s_max.copy_(grp.learners[l].s_max)
        agents.append((ag, ring))
    for name, call in (("clone", lambda ag, ring: ag.clone(ring)), ("evaluate", lambda ag, ring: ag.evaluate(ring))):
        m = median_of_five(lambda: [call(ag, ring) for ag, ring in agents])
        rec[f"single_learner_{name}"] = {"measured_agents": SINGLES, "measured": m, "extrapolated_to_learners": L,
                                         "extrapolated_median_ms": m["median_ms"] * L / SINGLES}
    finite = bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())
    rec["state_finite"] = finite
    return rec


def dagger_round_host(L=400, T=1438):
    tabs = [S.tables.synthetic_table("eval", c) for c in IDS]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, int(row0[k]), tabs[k].shape[0]) for k, c in enumerate(IDS)]
    env = S.ShemsBatch(L, T, tabs, cfgs, (np.arange(L) % len(IDS)).astype(np.uint16)).use_torch_stream()
    t0 = time.perf_counter()
    values = H.foresight_values(env)
    torch.cuda.synchronize()
    solve_s = time.perf_counter() - t0
    grp = G.LearnerGroup(L, 32, seed=1231, capacity=64, form="throughput")
    demos = I.GroupDemos(L, 2 * T)
    out = I.dagger_group(grp, env, values, demos, 2, 1)
    env.close()
    return {"learners": L, "hours_per_pass": T, "problems": values.n_problems, "foresight_solve_s": solve_s,
            "round_0_host_s": out[0]["host_s"], "round_1_host_s": out[1]["host_s"],
            "what": "wall clock around one round's env reset, tracking launch (foresight.track / harness.inference_many), the audit (round 1) "
                    "and count calls of shems_foresight_demos_dev with their host-to-device copies and status read-backs; round 0 also "
                    "holds the count min_max_buffer launches"}


if loop:
    grp, demos = group(400, 128)
    for _ in range(loop):
        grp.replay(); grp.clone(demos); grp.evaluate()
    torch.cuda.synchronize()
    print("looped", loop)
    sys.exit(0)
props = torch.cuda.get_device_properties(0)
doc = {"what": "LearnerGroup.clone / evaluate / replay, throughput form, the three updates of a shape in the same process; HIP events after a warm-up call, median of five",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "subset_bar": "each new update's median must lie below replay()'s median of the same process by more than the spread (max - min) of "
                     "replay()'s five runs",
       "shapes": {"400x128": shape(400, 128), "32x2048": shape(32, 2048)}, "dagger_round_at_400_learners": dagger_round_host()}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps({k: {n: (v[n]["median_ms"], v[n]["spread_ms"]) for n in ("replay", "clone", "evaluate")} for k, v in doc["shapes"].items()}))
print(json.dumps(doc["dagger_round_at_400_learners"]))
print("written", out_path)

"""What the grouped TD3 update costs (not a test): at 400 learners x 128 households and at 32 x 2 048, the three updates of a shape in
the same process,

  * one LearnerGroup.replay (the DDPG group's eight launches, unchanged by TD3), one TD3LearnerGroup.replay on a policy step (ten
    launches) and one off a policy step (seven) -- HIP events after a warm-up call, the median of five;
  * the same TD3 work as single-learner TD3Agent.replay calls, measured on 20 stand-alone agents and EXTRAPOLATED to the group's width
    (count / 20 x the measured time), as DESIGN.md 4m does.

One call is ONE ROUND; rounds in alternating processes are merged by --merge (medians of the rounds' medians, the per-round values and
the spread between rounds are kept):

    python tools/group_td3_timing.py round.json                  one round (both shapes)
    python tools/group_td3_timing.py --merge out.json r1.json r2.json r3.json
    python tools/group_td3_timing.py --loop N                    no measurement: N calls of each update at 400 x 128, for a profiler's kernel trace
    python tools/group_td3_timing.py --split trace.db out.json   per-kernel dispatch counts and median durations of the update kernels in the
                                                                 database `rocprofv3 --kernel-trace -- python tools/group_td3_timing.py --loop N`
                                                                 wrote (a run of its own); needs neither the GPU nor the package
    (default output profiles/r19_group_td3_timing.json; needs the GPU, does not read oracle/)
"""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UPDATES = ("replay", "td3_policy", "td3_non_policy")


def merge(out_path, paths):
    rounds = [json.load(open(p)) for p in paths]
    doc = {k: rounds[0][k] for k in ("what", "device", "arch", "compute_units")}
    doc["rounds"] = len(rounds)
    doc["shapes"] = {}
    for name in rounds[0]["shapes"]:
        rec = {k: rounds[0]["shapes"][name][k] for k in ("learners", "households_per_learner", "ring_capacity", "tiled")}
        for u in UPDATES:
            per = [r["shapes"][name][u]["median_ms"] for r in rounds]
            within = [r["shapes"][name][u]["spread_ms"] for r in rounds]
            rec[u] = {"median_ms": statistics.median(per), "per_round_median_ms": per, "spread_between_rounds_ms": max(per) - min(per),
                      "spread_within_round_ms": within, "spread_ms": max(max(per) - min(per), max(within))}
        rep, pol, non = rec["replay"], rec["td3_policy"], rec["td3_non_policy"]
        rec["conditions"] = {
            "non_policy_below_policy_by_more_than_the_larger_spread": (pol["median_ms"] - non["median_ms"]) > max(pol["spread_ms"], non["spread_ms"]),
            "policy_below_twice_replay": pol["median_ms"] < 2.0 * rep["median_ms"],
            "policy_over_replay": pol["median_ms"] / rep["median_ms"], "non_policy_over_replay": non["median_ms"] / rep["median_ms"]}
        per = [r["shapes"][name]["single_learner_td3"]["extrapolated_median_ms"] for r in rounds]
        rec["single_learner_td3_extrapolated"] = {"label": "EXTRAPOLATION: 20 stand-alone TD3Agents measured, scaled to the group's width, mean of a "
                                                  "non-policy and a policy update (d = 2)", "median_ms": statistics.median(per), "per_round_ms": per,
                                                  "over_grouped_d2_mean": statistics.median(per) / (0.5 * (pol["median_ms"] + non["median_ms"]))}
        doc["shapes"][name] = rec
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps({k: {u: v[u]["median_ms"] for u in UPDATES} | {"conditions": v["conditions"]} for k, v in doc["shapes"].items()}))
    print("written", out_path)


def split(db_path, out_path):
    """The `kernels` view of a rocprofv3 database -> {kernel: dispatches, median / min / max duration in us, LDS and scratch bytes} for the
    update kernels (shems::tp::).  The tracer's register columns are left out: they count allocation granules of the dispatch, not the
    compiler's registers (profiles/NOTES.md has those, from -Rpass-analysis=kernel-resource-usage)."""
    import collections
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, start, end, lds_size, scratch_size from kernels order by start").fetchall()
    us, meta = collections.defaultdict(list), {}
    for name, start, end, lds, scratch in rows:
        if "shems::tp::" in name:
            us[name].append((end - start) / 1e3)
            meta[name] = (lds, scratch)
    doc = {"what": "rocprofv3 --kernel-trace of `tools/group_td3_timing.py --loop N` at 400 learners x 128 households, tiled layout, a run of its "
                   "own (kernels run slower under the tracer): per kernel the number of dispatches and the median duration in us.  Each loop "
                   "pass is one LearnerGroup.replay, one TD3 policy step and one TD3 non-policy step: k_tp_fwd<false, 4, true> is P1 / T1 of all "
                   "three (three, three and two jobs), k_tp_gw2<11, true> runs once in replay and twice in each TD3 update, k_tp_w2_layout is "
                   "the one-off conversion into the tiled layout (twice for a TD3 group).",
           "produced_by": "tools/group_td3_timing.py --split",
           "kernels": {n: {"dispatches": len(v), "median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                           "lds_bytes": meta[n][0], "scratch_bytes": meta[n][1]} for n, v in sorted(us.items())}}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print("written", out_path, len(doc["kernels"]), "kernels")


if "--split" in sys.argv:
    i = sys.argv.index("--split")
    split(sys.argv[i + 1], sys.argv[i + 2])
    sys.exit(0)
if "--merge" in sys.argv:
    i = sys.argv.index("--merge")
    merge(sys.argv[i + 1], sys.argv[i + 2:])
    sys.exit(0)

import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
D = importlib.import_module(PKG + ".ddpg")
G = importlib.import_module(PKG + ".group")
T = importlib.import_module(PKG + ".td3")

loop = int(sys.argv[sys.argv.index("--loop") + 1]) if "--loop" in sys.argv else 0
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--loop"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r19_group_td3_timing.json")
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


def groups(L, E):
    """The thesis grid's shape: learner l on charger profile l mod 10, rings of CAP random-action transitions; the TD3 group's rings and
    normalisation are the DDPG group's."""
    tabs = [S.tables.synthetic_table("train", c) for c in IDS]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, int(row0[k]), tabs[k].shape[0]) for k, c in enumerate(IDS)]
    co = ((np.arange(L * E) // E) % len(IDS)).astype(np.uint16)
    env = S.ShemsBatch(L * E, 72, tabs, cfgs, co).use_torch_stream()
    grp = G.LearnerGroup(L, E, seed=1231, rng_seed=99, capacity=CAP, form="throughput")
    grp.populate_memory(env)
    grp.min_max_buffer()
    env.close()
    td3 = T.TD3LearnerGroup(L, E, seed=1231, rng_seed=99, capacity=CAP)
    for name in ("ring_s", "ring_a", "ring_r", "ring_s2", "ring_done", "s_min", "s_max"):
        o, n = grp.layout[name]
        o2, _ = td3.layout[name]
        td3.slab[:, o2:o2 + n].copy_(grp.slab[:, o:o + n])
    for a, b in zip(grp.rings, td3.rings):
        b.pushed = a.pushed
    return grp, td3


def shape(L, E):
    grp, td3 = groups(L, E)
    rec = {"learners": L, "households_per_learner": E, "ring_capacity": CAP, "tiled": grp.tiled,
           "replay": median_of_five(grp.replay), "td3_policy": median_of_five(lambda: td3.replay(update_policy=True)),
           "td3_non_policy": median_of_five(lambda: td3.replay(update_policy=False))}
    agents = []
    for l in range(SINGLES):
        ag, ring = T.TD3Agent(seed=1231 + l), D.ReplayRing(CAP)
        for k in ("s", "a", "r", "s2", "done"):
            getattr(ring, k).copy_(getattr(grp.rings[l], k))
        ring.pushed = CAP
        ag.s_min.copy_(grp.learners[l].s_min); ag.s_max.copy_(grp.learners[l].s_max)
        agents.append((ag, ring))
    m = {k: median_of_five(lambda: [ag.replay(ring, update_policy=p) for ag, ring in agents]) for k, p in (("policy", True), ("non_policy", False))}
    mean = 0.5 * (m["policy"]["median_ms"] + m["non_policy"]["median_ms"])
    rec["single_learner_td3"] = {"measured_agents": SINGLES, "measured": m, "extrapolated_to_learners": L, "extrapolated_median_ms": mean * L / SINGLES}
    rec["state_finite"] = bool(torch.isfinite(td3.slab[:, td3.layout["critic2"][0]:td3.layout["w2t_critic2"][0]]).all())
    return rec


if loop:
    grp, td3 = groups(400, 128)
    for _ in range(loop):
        grp.replay(); td3.replay(update_policy=True); td3.replay(update_policy=False)
    torch.cuda.synchronize()
    print("looped", loop)
    sys.exit(0)
props = torch.cuda.get_device_properties(0)
doc = {"what": "LearnerGroup.replay and TD3LearnerGroup.replay (policy / non-policy step), throughput form, the three updates of a shape in the "
               "same process; HIP events after a warm-up call, median of five",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "shapes": {"400x128": shape(400, 128), "32x2048": shape(32, 2048)}}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps({k: {n: (v[n]["median_ms"], v[n]["spread_ms"]) for n in UPDATES} for k, v in doc["shapes"].items()}))
print("written", out_path)

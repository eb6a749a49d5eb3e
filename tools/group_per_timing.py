"""What the grouped prioritized update costs (not a test): at 400 learners x 128 households and at 32 x 2 048, ring capacity 24 000, the
two updates of a shape in the same process -- one LearnerGroup.replay (the DDPG group's eight launches, unchanged by prioritized replay)
and one PrioritizedLearnerGroup.replay (nine launches: the sampler, then the eight with the slot-reading sampler role and the weighted
head) -- HIP events after a warm-up call, the median of five.  tools/group_td3_timing.py's method.  At 400 learners the five samples of
whichever update is measured first still fall from call to call (one warm-up call does not settle a 7 GB working set), so a second
series follows in the same process: five more calls of each update, ALTERNATING, every call timed on its own ("alternating").

One call is ONE ROUND; rounds in processes of their own are merged by --merge (medians of the rounds' medians, the per-round values and
the spread between rounds are kept):

    python tools/group_per_timing.py round.json                  one round (both shapes)
    python tools/group_per_timing.py --merge out.json r1.json r2.json r3.json
    python tools/group_per_timing.py --loop N                    no measurement: N calls of each update at 400 x 128, for a profiler's kernel trace
    python tools/group_per_timing.py --split trace.db out.json   per-kernel dispatch counts and median durations of the update kernels in the
                                                                 database `rocprofv3 --kernel-trace --stats -- python tools/group_per_timing.py
                                                                 --loop N` wrote (a run of its own, no counters); needs neither the GPU nor
                                                                 the package
    (default output profiles/r21_group_per_timing.json; needs the GPU, does not read oracle/)
"""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UPDATES = ("replay", "prioritized")


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
        for u in UPDATES:
            per = [r["shapes"][name]["alternating"][u]["median_ms"] for r in rounds]
            rec.setdefault("alternating", {})[u] = {"median_ms": statistics.median(per), "per_round_median_ms": per,
                                                    "spread_between_rounds_ms": max(per) - min(per),
                                                    "spread_within_round_ms": [r["shapes"][name]["alternating"][u]["spread_ms"] for r in rounds]}
        alt = rec["alternating"]
        alt["prioritized_minus_replay_ms"] = alt["prioritized"]["median_ms"] - alt["replay"]["median_ms"]
        alt["prioritized_over_replay"] = alt["prioritized"]["median_ms"] / alt["replay"]["median_ms"]
        rep, pri = rec["replay"], rec["prioritized"]
        rec["prioritized_minus_replay_ms"] = pri["median_ms"] - rep["median_ms"]
        rec["prioritized_over_replay"] = pri["median_ms"] / rep["median_ms"]
        doc["shapes"][name] = rec
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps({k: {u: v[u]["median_ms"] for u in UPDATES} | {"prioritized_over_replay": v["prioritized_over_replay"]} |
                      {"alternating": {u: v["alternating"][u]["median_ms"] for u in UPDATES}} for k, v in doc["shapes"].items()}))
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
    doc = {"what": "rocprofv3 --kernel-trace --stats of `tools/group_per_timing.py --loop N` at 400 learners x 128 households, ring capacity "
                   "24 000, tiled layout, a run of its own without counters (kernels run slower under the tracer): per kernel the number of "
                   "dispatches and the median duration in us.  Each loop pass is one LearnerGroup.replay and one PrioritizedLearnerGroup.replay: "
                   "k_tp_per_sample, k_tp_prep_per and k_tp_d1_per run once per pass beside k_tp_prep and k_tp_d1<11, ..>, every other update "
                   "kernel twice; k_tp_w2_layout is the one-off conversion into the tiled layout.",
           "produced_by": "tools/group_per_timing.py --split",
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
G = importlib.import_module(PKG + ".group")

loop = int(sys.argv[sys.argv.index("--loop") + 1]) if "--loop" in sys.argv else 0
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--loop"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r21_group_per_timing.json")
CAP, IDS = 24000, (1, 2, 3, 4, 5, 6, 7, 8, 9, 98)


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


def alternating(fns, n=5):
    """n more calls of each update, taken in turn, each between its own pair of events (both updates are warm by now)."""
    t = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[k].append(a.elapsed_time(b))
    return {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": v} for k, v in t.items()}


def groups(L, E):
    """The thesis grid's shape: learner l on charger profile l mod 10, rings of CAP random-action transitions; the prioritized group's rings
    and normalisation are the DDPG group's, every slot fresh at its first update (the warm-up call)."""
    tabs = [S.tables.synthetic_table("train", c) for c in IDS]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, int(row0[k]), tabs[k].shape[0]) for k, c in enumerate(IDS)]
    co = ((np.arange(L * E) // E) % len(IDS)).astype(np.uint16)
    env = S.ShemsBatch(L * E, 72, tabs, cfgs, co).use_torch_stream()
    grp = G.LearnerGroup(L, E, seed=1231, rng_seed=99, capacity=CAP, form="throughput")
    grp.populate_memory(env)
    grp.min_max_buffer()
    env.close()
    per = G.PrioritizedLearnerGroup(L, E, seed=1231, rng_seed=99, capacity=CAP)
    for name in ("ring_s", "ring_a", "ring_r", "ring_s2", "ring_done", "s_min", "s_max"):
        o, n = grp.layout[name]
        o2, _ = per.layout[name]
        per.slab[:, o2:o2 + n].copy_(grp.slab[:, o:o + n])
    for a, b in zip(grp.rings, per.rings):
        b.pushed = a.pushed
    return grp, per


def shape(L, E):
    grp, per = groups(L, E)
    rec = {"learners": L, "households_per_learner": E, "ring_capacity": CAP, "tiled": grp.tiled,
           "replay": median_of_five(grp.replay), "prioritized": median_of_five(per.replay)}
    rec["alternating"] = alternating({"replay": grp.replay, "prioritized": per.replay})
    o, n = per.layout["per_prio"]
    rec["state_finite"] = bool(torch.isfinite(per.slab[:, :per.layout["ws"][0]]).all() and torch.isfinite(per.slab[:, o:o + n]).all())
    rec["updates"] = [grp.updates, per.updates]
    return rec


if loop:
    grp, per = groups(400, 128)
    for _ in range(loop):
        grp.replay(); per.replay()
    torch.cuda.synchronize()
    print("looped", loop)
    sys.exit(0)
props = torch.cuda.get_device_properties(0)
doc = {"what": "LearnerGroup.replay and PrioritizedLearnerGroup.replay, throughput form, ring capacity 24 000, the two updates of a shape in the "
               "same process; HIP events after a warm-up call, median of five",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "shapes": {"400x128": shape(400, 128), "32x2048": shape(32, 2048)}}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps({k: {n: (v[n]["median_ms"], v[n]["spread_ms"], v["alternating"][n]["median_ms"]) for n in UPDATES} for k, v in doc["shapes"].items()}))
print("written", out_path)

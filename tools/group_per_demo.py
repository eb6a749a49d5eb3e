"""Section 4p's open question, asked of learner groups (not a benchmark, not a test: no order between the arms is asserted anywhere):

  1. uniform       DDPG with the uniform draw (group.LearnerGroup);
  2. prioritized   DDPG with proportional prioritized replay (group.PrioritizedLearnerGroup), alpha 0.6, beta 0.4 -> 1 over the episodes.

The protocol of tools/group_td3_demo.py: learner l = seed l // C on charger l % C, C = the chargers that have a real test series (1, 3,
6, 8, 9, 98); default 10 seeds.  Both arms train from freshly initialised networks through run_episodes (ENVS households per learner,
one grouped update per vector step, an evaluation sweep every 25 episodes on the synthetic eval tables).  Per arm: every learner's
return over its charger's real TEST series for the last and for the best-evaluated actor, their mean and spread over the learners, the
wall time of each stage, and the seed list.

    python tools/group_per_demo.py [out.json] [--seeds N] [--episodes N] [--envs N] [--mem N]
    (default profiles/r21_group_per.json; needs the GPU, does not read oracle/)
"""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
H = importlib.import_module(PKG + ".harness")
G = importlib.import_module(PKG + ".group")


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


flags = ("--seeds", "--episodes", "--envs", "--mem")
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r21_group_per.json")
SEEDS, EPISODES, ENVS, BATCH, SEED, MEM, TEST_EVERY = opt("--seeds", 10), opt("--episodes", 400), opt("--envs", 64), 120, 1231, opt("--mem", 24000), 25
ALPHA, BETA0 = 0.6, 0.4
IDS = tuple(c for c in (1, 2, 3, 4, 5, 6, 7, 8, 9, 98) if S.tables.real_series(c, "test") is not None)
C_, L = len(IDS), SEEDS * len(IDS)
charger_of = [l % C_ for l in range(L)]


def batch(tabs, per_learner, steps):
    """count x per_learner envs, learner l's block on tabs[l % C] with its charger's config."""
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, int(row0[k]), tabs[k].shape[0]) for k, c in enumerate(IDS)]
    co = np.repeat(np.asarray(charger_of, np.uint16), per_learner)
    return S.ShemsBatch(L * per_learner, steps, tabs, cfgs, co).use_torch_stream()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def spread(x):
    x = np.asarray(x, np.float64)
    return {"per_learner": [float(v) for v in x], "mean": float(x.mean()), "std": float(x.std()), "min": float(x.min()), "max": float(x.max())}


train_tabs = [S.tables.synthetic_table("train", c) for c in IDS]
eval_tabs = [S.tables.synthetic_table("eval", c) for c in IDS]
test_tabs = [S.tables.real_series(c, "test") for c in IDS]
T_TEST = min(t.shape[0] for t in test_tabs) - 1
env_test, env_train = batch(test_tabs, 1, T_TEST), batch(train_tabs, ENVS, 72)
env_eval = G.eval_batch(eval_tabs, charger_of, L, test_runs=100, maxsteps=1439, charger_ids=IDS)


def test_returns(actors, s_min, s_max):
    return H.inference_many(env_test, actors, s_min, s_max, num_steps=T_TEST)[0]


arms = {}
for arm in ("uniform", "prioritized"):
    per = arm == "prioritized"
    if per:
        grp = G.PrioritizedLearnerGroup(L, ENVS, alpha=ALPHA, beta=BETA0, seed=SEED, capacity=MEM)
    else:
        grp = G.LearnerGroup(L, ENVS, seed=SEED, form="throughput", capacity=MEM)
    for ag in grp.learners:
        ag.batch = BATCH
    rec = {"seeds": [grp.seed + l for l in range(L)], "charger": [IDS[k] for k in charger_of]}
    if per:
        rec.update(alpha=grp.alpha, beta0=BETA0, beta_last_episode=1.0, eps=grp.eps)
    _, rec["populate_s"] = wall(lambda: grp.populate_memory(env_train, seed=SEED))
    grp.min_max_buffer(seed=SEED)
    kw = dict(anneal_beta_from=BETA0) if per else {}
    res, rec["training_s"] = wall(lambda: grp.run_episodes(env_train, env_eval, EPISODES, test_every=TEST_EVERY, test_runs=100, seed=SEED, **kw))
    rec["training_device_s"], rec["sweeps_s"] = res.wall_ms / 1e3, res.sweep_ms / 1e3
    rec["evaluation_score_curve_mean"] = [float(x) for x in np.asarray(res.score_mean).mean(0)]
    if per:
        rec["beta_at_the_end"] = grp.beta
        rec["pmax"] = spread([grp.pmax_of(l).item() for l in range(L)])
    o, n = grp.layout["actor"]
    lo, hi = grp.layout["s_min"][0], grp.layout["s_max"][0]
    rec["return_test_last_actor"] = spread(test_returns(grp.slab[:, o:o + n], grp.slab[:, lo:lo + 9], grp.slab[:, hi:hi + 9]))
    norms = [res.best_norm(l) for l in range(L)]
    rec["return_test_best_evaluated_actor"] = spread(test_returns(res.best[:, :res.n_actor], np.stack([a for a, _ in norms]), np.stack([b for _, b in norms])))
    arms[arm] = rec
    print(arm, json.dumps({k: (v if not isinstance(v, dict) else {"mean": v.get("mean"), "std": v.get("std")}) for k, v in rec.items()
                           if k.startswith("return_test") or k.endswith("_s")}), flush=True)
    del grp
    torch.cuda.empty_cache()
rule_returns = []
for k, c in enumerate(IDS):
    e = S.ShemsBatch(1, T_TEST, [test_tabs[k]], [S.make_config(c, 0, test_tabs[k].shape[0])]).use_torch_stream()
    rule_returns.append(float(H.inference(e, None, track=-1)[0][0]))
    e.close()
u, p = arms["uniform"], arms["prioritized"]
paired = {}
for key in ("return_test_last_actor", "return_test_best_evaluated_actor"):
    d = np.asarray(p[key]["per_learner"]) - np.asarray(u[key]["per_learner"])
    paired[key] = {"prioritized_minus_uniform_mean": float(d.mean()), "std_of_the_differences": float(d.std()),
                   "standard_error_of_the_mean": float(d.std() / np.sqrt(len(d))), "learners_where_prioritized_is_higher": int((d > 0).sum())}
props = torch.cuda.get_device_properties(0)
doc = {"what": "DDPG with the uniform draw and with proportional prioritized replay, each arm as ONE learner group (group.LearnerGroup / "
               "group.PrioritizedLearnerGroup, run_episodes)",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "protocol": f"{SEEDS} seeds x chargers {list(IDS)} = {L} learners x {ENVS} households, ring capacity {MEM}, batch {BATCH}; {EPISODES} training "
                   f"episodes x 72 hours, evaluation sweep every {TEST_EVERY}; prioritized: alpha {ALPHA}, beta {BETA0} -> 1 linearly over the episodes; "
                   f"test returns over the real test series ({T_TEST} hours); the same seeds in both arms",
       "nothing_asserted": "no order between the arms is claimed", "rule_based_return_test": dict(zip(map(str, IDS), rule_returns)),
       "paired_over_learners": paired, "arms": arms}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps(paired))
print("written", out_path)

"""Population-based training on the section 4q protocol, both arms as ONE learner group of seeds x chargers (not a benchmark, not a
test: nothing is asserted about which arm is better):

  fixed   group.LearnerGroup with one default record per learner, trained to the end;
  pbt     the same group, seeds and records with run_episodes(pbt=PBT(one population per charger)): after every evaluation sweep but
          the first and the last, the worst quarter of each charger's learners take over the networks, optimiser state and record of
          one of the best quarter and perturb eta_act, eta_crit, tau and sigma by 0.8 or 1.2.

tools/group_nstep_demo.py's protocol: learner l = seed l // C on charger l % C, C = the chargers that have a real test series; default
10 seeds; ENVS households per learner, one grouped update per vector step, an evaluation sweep every 25 episodes on the synthetic eval
tables.  Per arm: every learner's return over its charger's real TEST series for the last and for the best-evaluated actor, their mean
and spread; the paired differences pbt - fixed learner by learner (the same seeds and chargers) with their standard error
sd / sqrt(L).  The best-evaluated actor of a slot is the slot's history: a child does not inherit its parent's snapshot.

    python tools/group_pbt_demo.py [out.json] [--seeds N] [--episodes N] [--envs N] [--mem N]
    (default profiles/r23_group_pbt.json; needs the GPU, does not read oracle/)
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
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r23_group_pbt.json")
SEEDS, EPISODES, ENVS, BATCH, SEED, MEM, TEST_EVERY = opt("--seeds", 10), opt("--episodes", 400), opt("--envs", 64), 120, 1231, opt("--mem", 24000), 25
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


def paired(x, base):
    d = np.asarray(x, np.float64) - np.asarray(base, np.float64)
    return {"mean_difference": float(d.mean()), "standard_error": float(d.std(ddof=1) / np.sqrt(d.size)), "learners_better": int((d > 0).sum()),
            "learners": int(d.size)}


train_tabs = [S.tables.synthetic_table("train", c) for c in IDS]
eval_tabs = [S.tables.synthetic_table("eval", c) for c in IDS]
test_tabs = [S.tables.real_series(c, "test") for c in IDS]
T_TEST = min(t.shape[0] for t in test_tabs) - 1
env_test, env_train = batch(test_tabs, 1, T_TEST), batch(train_tabs, ENVS, 72)
env_eval = G.eval_batch(eval_tabs, charger_of, L, test_runs=100, maxsteps=1439, charger_ids=IDS)


def test_returns(actors, s_min, s_max):
    return H.inference_many(env_test, actors, s_min, s_max, num_steps=T_TEST)[0]


arms = {}
for name in ("fixed", "pbt"):
    grp = G.LearnerGroup(L, ENVS, seed=SEED, form="throughput", capacity=MEM, hparams=[{"batch": BATCH} for _ in range(L)])
    pbt = G.PBT(charger_of, truncation=0.25, seed=SEED) if name == "pbt" else None
    rec = {"arm": name, "seeds": [grp.seed + l for l in range(L)], "charger": [IDS[k] for k in charger_of]}
    _, rec["populate_s"] = wall(lambda: grp.populate_memory(env_train, seed=SEED))
    grp.min_max_buffer(seed=SEED)
    res, rec["training_s"] = wall(lambda: grp.run_episodes(env_train, env_eval, EPISODES, test_every=TEST_EVERY, test_runs=100, seed=SEED, pbt=pbt))
    rec["training_device_s"], rec["sweeps_s"] = res.wall_ms / 1e3, res.sweep_ms / 1e3
    rec["evaluation_score_curve_mean"] = [float(x) for x in np.asarray(res.score_mean).mean(0)]
    if pbt is not None:
        par = res.pbt_parent
        rec["pbt"] = {"populations": "one per charger", "truncation": pbt.truncation, "fields": list(pbt.fields), "down": pbt.down, "up": pbt.up,
                      "bounds": pbt.bounds, "round_after_episode": res.pbt_episodes, "children_per_round": [int((par[:, r] != np.arange(L)).sum())
                                                                                                           for r in range(par.shape[1])],
                      "parent": par.T.tolist(),
                      "final_records": [{k: h[k] for k in ("eta_act", "eta_crit", "tau", "sigma")} for h in grp.hparams]}
    o, cnt = grp.layout["actor"]
    lo, hi = grp.layout["s_min"][0], grp.layout["s_max"][0]
    rec["return_test_last_actor"] = spread(test_returns(grp.slab[:, o:o + cnt], grp.slab[:, lo:lo + 9], grp.slab[:, hi:hi + 9]))
    norms = [res.best_norm(l) for l in range(L)]
    rec["return_test_best_evaluated_actor"] = spread(test_returns(res.best[:, :res.n_actor], np.stack([a for a, _ in norms]),
                                                                  np.stack([b for _, b in norms])))
    if name == "pbt":
        for k in ("return_test_last_actor", "return_test_best_evaluated_actor"):
            rec[k + "_minus_fixed"] = paired(rec[k]["per_learner"], arms["fixed"][k]["per_learner"])
    arms[name] = rec
    print(name, json.dumps({k: (v if not isinstance(v, dict) else {a: c for a, c in v.items() if a != "per_learner"}) for k, v in rec.items()
                            if k.startswith("return_test") or k.endswith("_s")}), flush=True)
    del grp
    torch.cuda.empty_cache()
props = torch.cuda.get_device_properties(0)
doc = {"what": "fixed default records against population-based training (one population per charger), both arms as ONE learner group",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "protocol": f"{SEEDS} seeds x chargers {list(IDS)} = {L} learners x {ENVS} households; ring {MEM}, batch {BATCH}; {EPISODES} training "
                   f"episodes x 72 hours, evaluation sweep every {TEST_EVERY}; test returns over the real test series ({T_TEST} hours); paired "
                   "differences pbt - fixed, standard error sd / sqrt(learners)",
       "nothing_asserted": "no order between the arms is claimed", "arms": arms}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print("written", out_path)

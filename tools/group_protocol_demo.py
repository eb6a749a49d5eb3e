"""The thesis protocol at its real width, end to end (not a benchmark): 40 seeds x 10 charger profiles = 400 independent DDPG learners
(RL-SHEMS_bs_scheduler_1179_08_on_01-98.sh:67-87; learner l trains on charger profile l mod 10), each on 128 households, trained by the
grouped launches -- fused act/step for all 51 200 households + the throughput form of the grouped replay() (csrc/shems_gupd.hip) -- for
argv[2] episodes of 72 hours (default 1001) through LearnerGroup.run_episodes: every 100 episodes an evaluation sweep scores every
learner on its own charger's eval table (100 starts, 72 hours) and keeps its best actor (DDPG.jl:244-298).  Reported per learner: the
score curve, best_run, and the eval score of the best actor next to the last one; per charger the rule-based controller on the same
starts; the wall time of training next to that of all sweeps, and of one learner-by-learner sweep (400 Agent.episode_ calls) for
comparison.  argv[3] = "latency" runs the same protocol on the five-launch form (fewer episodes advised).  argv[5] = households per
learner (default 128; any multiple of 32: with argv[4] = 1 only household 0 feeds the learner, so 32 -- the smallest tile of the fused
kernel -- is the closest this framework comes to the reference's ONE household per learner).  The optional flag --foresight (anywhere
on the command line) adds group.foresight_scores -- the perfect-foresight return on the same 100 starts -- per learner and per charger.
Writes one JSON document to argv[1]."""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
D = importlib.import_module(PKG + ".ddpg")
G = importlib.import_module(PKG + ".group")

FORESIGHT = "--foresight" in sys.argv
sys.argv = [a for a in sys.argv if a != "--foresight"]
out_path = sys.argv[1] if len(sys.argv) > 1 else "group_protocol.json"
episodes = int(sys.argv[2]) if len(sys.argv) > 2 else 1001
form = sys.argv[3] if len(sys.argv) > 3 else "throughput"
window = int(sys.argv[4]) if len(sys.argv) > 4 and sys.argv[4] not in ("", "default") else None
SEEDS, TEST_EVERY, TEST_RUNS = 40, 100, 100
E = int(sys.argv[5]) if len(sys.argv) > 5 else 128
ids = (1, 2, 3, 4, 5, 6, 7, 8, 9, 98)
L = SEEDS * len(ids)
tabs = [S.tables.synthetic_table("train", c) for c in ids]
row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
cfgs = [S.make_config(c, row0[k], tabs[k].shape[0]) for k, c in enumerate(ids)]
co = ((np.arange(L * E) // E) % len(ids)).astype(np.uint16)
env = S.ShemsBatch(L * E, 72, tabs, cfgs, co).use_torch_stream()
eval_tabs = [S.tables.synthetic_table("eval", c) for c in ids]
env_eval = G.eval_batch(eval_tabs, [l % len(ids) for l in range(L)], L, test_runs=TEST_RUNS, maxsteps=1439, charger_ids=ids)
grp = G.LearnerGroup(L, E, seed=1231, rng_seed=99, form=form)
grp.populate_memory(env)
grp.min_max_buffer()
torch.cuda.synchronize()
t0 = time.perf_counter()
res = grp.run_episodes(env, env_eval, episodes, test_every=TEST_EVERY, test_runs=TEST_RUNS, window_count=window)
wall = time.perf_counter() - t0
finite = bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())
total, score_mean, best_run, best_score = res.total_reward, res.score_mean, res.best_run, res.best_score
last_score = grp.eval_scores(env_eval, TEST_RUNS)            # the last actors on the same starts (run_episodes left flux_() done)
# the learner-by-learner evaluation this replaces: each learner's Agent on its charger's 100-env eval batch, 72 launches per learner
singles = []
for k, cid in enumerate(ids):
    b = S.ShemsBatch(TEST_RUNS, 1439, [eval_tabs[k]], [S.make_config(cid, 0, eval_tabs[k].shape[0])]).use_torch_stream()
    singles.append(b)
torch.cuda.synchronize()
t1 = time.perf_counter()
for l in range(L):
    grp.learners[l].episode_(singles[l % len(ids)], None, train=False, num_steps=72, rng_ep=D.SEED_INI, episode=0)
torch.cuda.synchronize()
per_learner_sweep_s = time.perf_counter() - t1
rule = {}
for k, cid in enumerate(ids):
    singles[k].reset_(D.SEED_INI, episode=0)
    rule[cid] = float(singles[k].rollout("rule", 72).mean().item())
    singles[k].close()
per_charger = {}
for k, cid in enumerate(ids):
    sl = slice(k, L, len(ids))
    per_charger[str(cid)] = {"rule_based": rule[cid], "learners": SEEDS, "best_actor_score_mean": float(best_score[sl].mean()),
                             "last_actor_score_mean": float(last_score[sl].mean()), "best_actor_score_max": float(best_score[sl].max()),
                             "best_beats_rule_based": int((best_score[sl] > rule[cid]).sum()),
                             "last_beats_rule_based": int((last_score[sl] > rule[cid]).sum())}
wc = grp.ring_window(72, window)[0]
sweep_s, run_s = res.sweep_ms / 1e3, res.wall_ms / 1e3
doc = {"protocol": f"40 seeds x 10 chargers = 400 learners x {E} households, grouped launches, run_episodes(test_every={TEST_EVERY}, "
                   f"test_runs={TEST_RUNS})", "households_per_learner": E, "form": grp.form, "tiled": grp.tiled, "episodes": episodes,
       "remembered_transitions_per_learner_update": wc,
       "update_to_data": ("1 update per remembered transition: the reference's ratio (DDPG.jl:229-233)" if wc == 1 else
                          f"1 update per {wc} remembered transitions ({wc} x the reference's data per update)"),
       "updates_per_learner": grp.updates, "learner_updates_total": grp.updates * L, "env_steps": episodes * 72 * L * E,
       "wall_s": wall, "run_episodes_device_s": run_s, "sweeps_per_learner": res.sweeps, "sweeps_s": sweep_s, "train_s": run_s - sweep_s,
       "sweep_share_of_run": sweep_s / run_s, "one_sweep_ms": res.sweep_ms / max(1, res.sweeps),
       "one_learner_by_learner_sweep_s": per_learner_sweep_s, "learner_by_learner_launches_per_sweep": L * 72,
       "timing_method": "HIP events around the whole run_episodes call and around each sweep (reset, 72 fused steps, the scoring launch); "
                        "the learner-by-learner sweep: wall clock around 400 Agent.episode_ calls, synchronised",
       "learner_updates_per_s": grp.updates * L / (run_s - sweep_s), "state_finite": finite,
       "train_return_first_mean": float(total[:, 0].mean()), "train_return_last_mean": float(total[:, -1].mean()),
       "noise_mean_first_mean": float(res.noise_mean[:, 0].mean()),
       "learners_with_best_run": int((best_run > 0).sum()), "per_charger": per_charger,
       "learners": [{"learner": l, "charger": ids[l % len(ids)], "best_run": int(best_run[l]), "best_actor_score": float(best_score[l]),
                     "last_actor_score": float(last_score[l]), "score_mean": [round(float(x), 4) for x in score_mean[l]]} for l in range(L)]}
if FORESIGHT:                                                # the upper yardstick on the sweeps' own starts (discretised: not a bound)
    fs = G.foresight_scores(env_eval, TEST_RUNS)
    for l in range(L):
        doc["learners"][l]["foresight_score"] = float(fs[l])
    for k, cid in enumerate(ids):
        per_charger[str(cid)]["foresight"] = float(fs[k::len(ids)].mean())
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps({k: doc[k] for k in ("form", "episodes", "sweeps_per_learner", "learners_with_best_run", "train_s", "sweeps_s",
                                      "sweep_share_of_run", "one_sweep_ms", "one_learner_by_learner_sweep_s", "learner_updates_per_s",
                                      "state_finite")}))
print(json.dumps({c: (round(v["rule_based"], 1), round(v["best_actor_score_mean"], 1), round(v["last_actor_score_mean"], 1))
                  for c, v in per_charger.items()}))

"""Does prioritized replay change what the DDPG learner reaches on Charger 98?  Two arms with the same seed and the same number of
run_episodes episodes (not a benchmark, not a test: no order between the arms is asserted anywhere; one seed asserts nothing):

  1. ddpg_uniform       DDPG on a ReplayRing (the uniform draw of replay());
  2. ddpg_prioritized   DDPG on a replay.PrioritizedRing (alpha 0.6, beta annealed from 0.4 to 1 over the run, eps 1e-6).

Protocol of tools/td3_demo.py: EPISODES episodes of 72 hours on the synthetic Charger98 train table (ENVS households at once, one
update per vector step, an evaluation sweep every 25 episodes on the synthetic eval table).  Per arm: the evaluation-score curve and
the return of the last and of the best-evaluated actor over the Charger98 TEST series (2 998 hours from the reset!(rng = -1) start);
for the prioritized arm also pmax and the spread of the priorities at the end.

    python tools/per_demo.py [out.json] [--episodes N]
    (default profiles/r20_per.json; needs the GPU, does not read oracle/)
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
H = importlib.import_module(PKG + ".harness")
D = importlib.import_module(PKG + ".ddpg")

args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--episodes"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r20_per.json")
EPISODES = int(sys.argv[sys.argv.index("--episodes") + 1]) if "--episodes" in sys.argv else 400
BATCH, SEED, ENVS, MEM = 120, 1231, 64, 24000
ALPHA, BETA0, EPS_P = 0.6, 0.4, 1e-6

ttab, etab, xtab = S.tables.synthetic_table("train", 98), S.tables.synthetic_table("eval", 98), S.tables.real_series(98, "test")
mk = lambda n, steps, tab: S.ShemsBatch(n, steps, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
env_test, env_train, env_eval = mk(1, xtab.shape[0] - 1, xtab), mk(ENVS, 72, ttab), mk(100, etab.shape[0] - 1, etab)
rule_test = float(H.inference(env_test, None, track=-1)[0][0])
arms = {}
for arm in ("ddpg_uniform", "ddpg_prioritized"):
    per = arm == "ddpg_prioritized"
    agent = D.Agent(seed=SEED)
    agent.batch = BATCH
    ring = D.PrioritizedRing(MEM, alpha=ALPHA, beta=BETA0, eps=EPS_P) if per else D.ReplayRing(MEM)
    agent.populate_memory(env_train, ring, seed=SEED)
    agent.min_max_buffer(ring, MEM, seed=SEED)
    _, score_mean, best_run, best_actor = agent.run_episodes(env_train, env_eval, ring, EPISODES, test_every=25, test_runs=100, seed=SEED,
                                                             **(dict(anneal_beta_from=BETA0) if per else {}))
    rec = dict(updates=int(agent.updates), evaluation_score_curve=[float(x) for x in score_mean], best_evaluated_episode=int(best_run),
               critic_loss_last=float(agent.losses[0].item()), return_test_last_actor=float(H.inference(env_test, agent, track=1)[0][0]))
    if per:
        p = ring.prio.cpu().numpy()
        rec.update(pmax=float(ring.pmax.item()), beta_last=ring.beta, priority_min=float(p.min()), priority_median=float(sorted(p)[len(p) // 2]),
                   priority_max=float(p.max()))
    agent.set_params(actor=best_actor)
    rec["return_test_best_evaluated_actor"] = float(H.inference(env_test, agent, track=1)[0][0])
    arms[arm] = rec
    print(arm, json.dumps(rec), flush=True)
for e in (env_test, env_train, env_eval):
    e.close()
props = torch.cuda.get_device_properties(0)
doc = {"what": "DDPG with the uniform draw next to DDPG with proportional prioritized replay on Charger 98; returns are plain sums of rewards",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName,
       "nothing_asserted": "no order between the arms is claimed; one seed, a short protocol",
       "protocol": f"{EPISODES} training episodes x 72 hours, {ENVS} households at once on the synthetic Charger98 train table, one update per "
                   f"vector step, evaluation sweep (100 starts on the synthetic eval table) every 25 episodes, seed {SEED} in both arms, batch "
                   f"{BATCH}, ring {MEM}; prioritized: alpha {ALPHA}, beta {BETA0} -> 1 linearly over the episodes, eps {EPS_P}",
       "rule_based_return_test": rule_test, "arms": arms}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print("written", out_path)

"""Does TD3 -- twin critics, a smoothed target action, a delayed actor -- change what the learner reaches on Charger 98, from scratch and
from a cloned actor?  Four arms with the same seed and the same number of run_episodes episodes (not a benchmark, not a test: no order
between the arms is asserted anywhere):

  1. ddpg          DDPG from freshly initialised networks;
  2. td3           TD3 (td3.TD3Agent, sigma_trg 0.2, clip_trg 0.5, d = 2) from freshly initialised networks;
  3. clone+ddpg    the actor cloned by imitation.dagger, a fresh critic, then DDPG;
  4. clone+td3     the same cloned actor (TD3Agent.clone is the Agent's), two fresh critics, then TD3.

Protocol of tools/foresight_warmstart_demo.py: demonstrations on the synthetic Charger98 train table (4 318 hours, one foresight.solve
at the default grid), EPISODES episodes of 72 hours on it (ENVS households at once, one update per vector step, an evaluation sweep
every 25 episodes on the synthetic eval table).  Per arm: the evaluation-score curve and the return of the last and of the
best-evaluated actor over the Charger98 TEST series (2 998 hours from the reset!(rng = -1) start).

Update times: tools/td3_update_time.py as child processes, one mode per process, the modes alternating, ROUNDS rounds, the median per
mode: Agent.replay (of --parent-lib PATH where given: the parent commit's build, else of this build), TD3Agent.replay on a policy step
and off one.

    python tools/td3_demo.py [out.json] [--parent-lib PATH] [--timings-only] [--arms-only]
    (default profiles/r18_td3.json; needs the GPU, does not read oracle/)
"""
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
H = importlib.import_module(PKG + ".harness")
D = importlib.import_module(PKG + ".ddpg")
I = importlib.import_module(PKG + ".imitation")
T = importlib.import_module(PKG + ".td3")

args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--parent-lib"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r18_td3.json")
parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
ROUNDS_CLONE, STEPS, BATCH, SEED = 4, 5000, 120, 1231
EPISODES, ENVS, MEM, T_FIT, ROUNDS = 400, 64, 24000, 4318, 3


def arms():
    ttab, etab, xtab = S.tables.synthetic_table("train", 98), S.tables.synthetic_table("eval", 98), S.tables.real_series(98, "test")
    mk = lambda n, steps, tab: S.ShemsBatch(n, steps, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    env_fit, env_test = mk(1, T_FIT, ttab), mk(1, xtab.shape[0] - 1, xtab)
    env_train, env_eval = mk(ENVS, 72, ttab), mk(100, etab.shape[0] - 1, etab)
    values = H.foresight_values(env_fit)
    rule_test = float(H.inference(env_test, None, track=-1)[0][0])
    out = {}
    for arm in ("ddpg", "td3", "clone+ddpg", "clone+td3"):
        agent = T.TD3Agent(seed=SEED) if arm.endswith("td3") else D.Agent(seed=SEED)
        agent.batch = BATCH
        ring = D.ReplayRing(MEM)
        agent.populate_memory(env_train, ring, seed=SEED)
        rec = {}
        if arm.startswith("clone"):                         # the normalisation is dagger's, set from the foresight pass
            figures = I.dagger(agent, env_fit, values, I.Demos(ROUNDS_CLONE * T_FIT), ROUNDS_CLONE, STEPS)
            rec.update(foresight_return_fit=figures[0]["return"], clone_loss_after_round=[r["loss"] for r in figures],
                       return_test_before_training=float(H.inference(env_test, agent, track=1)[0][0]))
        else:
            agent.min_max_buffer(ring, MEM, seed=SEED)
        _, score_mean, best_run, best_actor = agent.run_episodes(env_train, env_eval, ring, EPISODES, test_every=25, test_runs=100, seed=SEED)
        rec.update(updates=int(agent.updates), evaluation_score_curve=[float(x) for x in score_mean], best_evaluated_episode=int(best_run),
                   critic_loss_last=float(agent.losses[0].item()), return_test_last_actor=float(H.inference(env_test, agent, track=1)[0][0]))
        if arm.endswith("td3"):
            rec["critic2_loss_last"] = float(agent.losses2[0].item())
        agent.set_params(actor=best_actor)
        rec["return_test_best_evaluated_actor"] = float(H.inference(env_test, agent, track=1)[0][0])
        out[arm] = rec
        print(arm, json.dumps(rec), flush=True)
    for e in (env_fit, env_test, env_train, env_eval):
        e.close()
    return {"protocol": f"{EPISODES} training episodes x 72 hours, {ENVS} households at once on the synthetic Charger98 train table, one update per "
                        f"vector step, evaluation sweep (100 starts on the synthetic eval table) every 25 episodes, seed {SEED} in every arm; "
                        f"cloning: {ROUNDS_CLONE} rounds x {STEPS} supervised updates on the train table ({T_FIT} hours), batch {BATCH}; TD3: "
                        f"sigma_trg {T.SIGMA_TRG}, clip_trg {T.CLIP_TRG}, policy_delay {T.POLICY_DELAY}; a short run of this script, not the "
                        f"thesis protocol", "rule_based_return_test": rule_test, "arms": out}


def update_times():
    tool = os.path.join(ROOT, "tools", "td3_update_time.py")
    runs = {"ddpg_replay": [], "td3_policy_step": [], "td3_non_policy_step": []}
    for _ in range(ROUNDS):                                 # fresh child processes, the three alternating
        for key, mode in (("ddpg_replay", "ddpg"), ("td3_policy_step", "td3_policy"), ("td3_non_policy_step", "td3_critic")):
            env = dict(os.environ)
            if key == "ddpg_replay" and parent_lib:
                env["SHEMS_HIP_LIB"] = os.path.abspath(parent_lib)
            line = subprocess.check_output([sys.executable, tool, mode], env=env, timeout=300).decode().strip().split("\n")[-1]
            runs[key].append(json.loads(line))
            print(key, line, flush=True)
    out = {k: {"median_us": statistics.median(r["us_per_update"] for r in v), "all_us": [r["us_per_update"] for r in v],
               "host_enqueue_us": [r["host_enqueue_us_per_update"] for r in v]} for k, v in runs.items()}
    out["ddpg_replay"]["library"] = "the parent commit's build" if parent_lib else "this build (the DDPG kernels are the parent's code)"
    out["ratio_policy_step_to_ddpg"] = out["td3_policy_step"]["median_us"] / out["ddpg_replay"]["median_us"]
    out["ratio_non_policy_to_policy_step"] = out["td3_non_policy_step"]["median_us"] / out["td3_policy_step"]["median_us"]
    out["timing_note"] = ("tools/td3_update_time.py: HIP events around 4 000 updates enqueued back to back after 200 warm-up updates, 65 536-env "
                          "TrainWorkload setting (ring 24 000, batch 120, Flux order), one mode per process, the modes alternating, "
                          f"{ROUNDS} rounds, medians")
    return out


props = torch.cuda.get_device_properties(0)
doc = {"what": "TD3 (twin critics, target smoothing, delayed actor) next to DDPG on Charger 98, from scratch and from a cloned actor; returns "
               "are plain sums of rewards", "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName,
       "compute_units": props.multi_processor_count, "nothing_asserted": "no order between the arms is claimed; one seed, a short protocol"}
if os.path.exists(out_path):                                # a second visit (--timings-only / --arms-only) keeps what the first wrote
    try:
        doc.update({k: v for k, v in json.load(open(out_path)).items() if k in ("update_times", "training", "kernel_means_us")})
    except ValueError:
        pass
if "--arms-only" not in sys.argv:
    doc["update_times"] = update_times()
if "--timings-only" not in sys.argv:
    doc["training"] = arms()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print("written", out_path)

"""Does DDPG fine-tuning keep what cloning taught the actor when the critic is fitted first?  Four arms on Charger 98 with the same
seeds and the same number of run_episodes episodes (not a benchmark, not a test: no order between the arms is asserted anywhere):

  1. scratch     DDPG from freshly initialised networks;
  2. clone       the actor cloned by imitation.dagger, a fresh critic;
  3. clone+td    imitation.warm_start(mode="td"): the cloned actor, its critic fitted by critic-only updates on the replay ring after the
                 transitions of one pass of the cloned actor were written into it, and that ring goes on as the replay ring;
  4. clone+mc    imitation.warm_start(mode="mc"): the critic regressed on the returns-to-go of that pass (a ring of its own, done = 1),
                 and the replay ring seeded with the same pass's "td" transitions.

Demonstrations and critic fit are made on the TRAINING table (the synthetic Charger98 train table, 4 318 hours from row 1, one
foresight.solve at the default grid); every arm then trains EPISODES episodes of 72 hours on it (ENVS households at once, one update
per vector step, an evaluation sweep every 25 episodes on the synthetic eval table).  Per arm: the evaluation-score curve and the
return of the last and of the best-evaluated actor over the Charger98 TEST series (2 998 hours from the reset!(rng = -1) start).

Speed, one process, HIP events after a warm-up call, the median of five: shems_foresight_transitions_dev (device-resident rows into a
preallocated ring) for 1 pass x 2 998 hours and 80 passes x 1 438 hours in both modes, next to shems_foresight_demos_dev on the same
rows; one ddpg.Agent.evaluate next to the split form (critic_grad + critic_apply) and to a full replay().

    python tools/foresight_warmstart_demo.py [out.json] [--timings-only]
    (default profiles/r16_foresight_warmstart.json; needs the GPU, does not read oracle/)
"""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
F = importlib.import_module(PKG + ".foresight")
H = importlib.import_module(PKG + ".harness")
D = importlib.import_module(PKG + ".ddpg")
I = importlib.import_module(PKG + ".imitation")

args = [a for a in sys.argv[1:] if not a.startswith("--")]
timings_only = "--timings-only" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r16_foresight_warmstart.json")
ROUNDS, STEPS, CRITIC_STEPS, BATCH, SEED = 4, 5000, 5000, 120, 1231
EPISODES, ENVS, MEM, T_FIT = 400, 64, 24000, 4318


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def median_of_five(fn):
    fn()                                                    # the warm-up call
    torch.cuda.synchronize()
    t = [timed(fn)[1] for _ in range(5)]
    return {"median_ms": statistics.median(t), "all_ms": t}


# ---------------------------------------------------------------------------- the four arms --
def arms():
    ttab, etab, xtab = S.tables.synthetic_table("train", 98), S.tables.synthetic_table("eval", 98), S.tables.real_series(98, "test")
    mk = lambda n, steps, tab: S.ShemsBatch(n, steps, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    env_fit, env_test = mk(1, T_FIT, ttab), mk(1, xtab.shape[0] - 1, xtab)
    env_train, env_eval = mk(ENVS, 72, ttab), mk(100, etab.shape[0] - 1, etab)
    values = H.foresight_values(env_fit)
    rule_fit, rule_test = float(H.inference(env_fit, None, track=-1)[0][0]), float(H.inference(env_test, None, track=-1)[0][0])
    out = {}
    for arm in ("scratch", "clone", "clone+td", "clone+mc"):
        agent = D.Agent(seed=SEED)
        agent.batch = BATCH
        ring = D.ReplayRing(MEM)
        agent.populate_memory(env_train, ring, seed=SEED)
        rec = {}
        if arm == "scratch":
            agent.min_max_buffer(ring, MEM, seed=SEED)
        else:                                               # the normalisation is dagger's, set from the foresight pass
            demos = I.Demos(ROUNDS * T_FIT)
            if arm == "clone":
                figures, critic = I.dagger(agent, env_fit, values, demos, ROUNDS, STEPS), None
            elif arm == "clone+td":
                *figures, critic = I.warm_start(agent, env_fit, values, demos, ring, ROUNDS, STEPS, CRITIC_STEPS, mode="td")
            else:
                fitted = D.ReplayRing(T_FIT)
                *figures, critic = I.warm_start(agent, env_fit, values, demos, fitted, ROUNDS, STEPS, CRITIC_STEPS, mode="mc")
                _, rows = H.inference(env_fit, agent, track=1, num_steps=T_FIT)
                I.transitions(values, rows, ring, mode="td", gamma=agent.gamma)
            rec.update(foresight_return_fit=figures[0]["return"], clone_loss_after_round=[r["loss"] for r in figures], critic_fit=critic,
                       return_fit_before_ddpg=float(H.inference(env_fit, agent, track=1, num_steps=T_FIT)[0][0]),
                       return_test_before_ddpg=float(H.inference(env_test, agent, track=1)[0][0]))
        _, score_mean, best_run, best_actor = agent.run_episodes(env_train, env_eval, ring, EPISODES, test_every=25, test_runs=100, seed=SEED)
        rec.update(evaluation_score_curve=[float(x) for x in score_mean], best_evaluated_episode=int(best_run),
                   return_test_last_actor=float(H.inference(env_test, agent, track=1)[0][0]))
        agent.set_params(actor=best_actor)
        rec["return_test_best_evaluated_actor"] = float(H.inference(env_test, agent, track=1)[0][0])
        out[arm] = rec
        print(arm, json.dumps(rec), flush=True)
    for e in (env_fit, env_test, env_train, env_eval):
        e.close()
    return {"protocol": f"{EPISODES} training episodes x 72 hours, {ENVS} households at once on the synthetic Charger98 train table, one update per "
                        f"vector step, evaluation sweep (100 starts on the synthetic eval table) every 25 episodes, seed {SEED} in every arm; "
                        f"imitation: {ROUNDS} rounds x {STEPS} supervised updates on the train table ({T_FIT} hours), critic fit: {CRITIC_STEPS} "
                        f"critic-only updates, batch {BATCH}; a short run of this script, not the thesis protocol",
            "rule_based_return_fit": rule_fit, "rule_based_return_test": rule_test, "arms": out}


# --------------------------------------------------------------------------------- timings --
def timings():
    L = I._declare(S._capi.lib())
    small = F.Grid(3, 3, 2, 2)                              # the transitions read the problem records and the tables, no plane
    agent = D.Agent(seed=SEED)
    agent.batch = BATCH
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for name, tab, n_pass in (("1x2998", S.tables.real_series(98, "test"), 1), ("80x1438", S.tables.synthetic_table("eval", 98), 80)):
        T = tab.shape[0] - 2 if n_pass > 1 else tab.shape[0] - 1
        env = S.ShemsBatch(1, T, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
        values = H.foresight_values(env, small)
        _, rows = H.inference(env, agent, track=1, num_steps=T)
        d_rows = torch.from_numpy(np.ascontiguousarray(np.repeat(rows[None], n_pass, 0))).cuda()
        d_tgt = torch.from_numpy(np.ascontiguousarray(np.repeat(rows[None][:, :, [21, 2]], n_pass, 0).astype(np.float32))).cuda()
        ring = D.ReplayRing(n_pass * T)
        status = torch.empty(n_pass, dtype=torch.int32, device="cuda")
        d_ret = torch.empty((n_pass, T), dtype=torch.float64, device="cuda")
        g, rs = small.struct(), ring.struct()
        common = (C.c_void_p(env.view().tables), int(values.total_rows), C.c_void_p(values.d_problems.data_ptr()), 1)

        def demos_call():
            S._capi.check(L.shems_foresight_demos_dev(*common, C.byref(g), T, C.c_void_p(d_rows.data_ptr()), n_pass, None,
                                                      C.c_void_p(d_tgt.data_ptr()), None, C.byref(rs), 0, C.c_void_p(status.data_ptr()), stream()))

        def trans_call(mode, ret):
            S._capi.check(L.shems_foresight_transitions_dev(*common, T, C.c_void_p(d_rows.data_ptr()), n_pass, None, mode, float(agent.gamma),
                                                            I.default_tail("mc" if mode else "td", agent.gamma, T),
                                                            C.c_void_p(d_ret.data_ptr()) if ret else None, C.byref(rs), 0,
                                                            C.c_void_p(status.data_ptr()), stream()))

        rec = {"demos": median_of_five(demos_call), "transitions_td": median_of_five(lambda: trans_call(0, False)),
               "transitions_td_with_returns": median_of_five(lambda: trans_call(0, True)), "transitions_mc": median_of_five(lambda: trans_call(1, True))}
        assert int(status.abs().max().item()) == 0 and bool(torch.isfinite(d_ret).all())
        out[name] = rec
        env.close()
    # one critic-only update next to the split form and to a full replay(), a full ring of random transitions
    ttab = S.tables.synthetic_table("train", 98)
    env_train = S.ShemsBatch(ENVS, 72, [ttab], [S.make_config(98, 0, ttab.shape[0])]).use_torch_stream()
    ring = D.ReplayRing(MEM)
    agent.populate_memory(env_train, ring, seed=SEED)
    agent.min_max_buffer(ring, MEM, seed=SEED)
    env_train.close()

    def split():
        d, st, rs = agent._ddpg_args(), agent._stream(), ring.struct()
        agent._critic_grad_ex(d, rs, len(ring), 0, 0, 0, st)
        agent._critic_apply(d, 1.0, st)

    out["update"] = {"evaluate": median_of_five(lambda: agent.evaluate(ring)), "split_critic_grad_plus_apply": median_of_five(split),
                     "replay": median_of_five(lambda: agent.replay(ring))}
    out["timing_note"] = ("HIP events on the current stream around the entry point alone (device-resident rows, a preallocated ring; the "
                          "zeroing of the status words included), resp. around one Agent call; one warm-up call each, then five calls, one "
                          "process; mc tail = imitation.default_tail (459 hours), td tail = 1")
    return out


props = torch.cuda.get_device_properties(0)
doc = {"what": "DDPG fine-tuning of an actor cloned from the perfect-foresight controller, with and without a critic fitted on tracked passes "
               "first (imitation.warm_start); Charger 98, returns are plain sums of rewards",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "nothing_asserted": "no order between the arms is claimed; one seed, a short protocol"}
doc["speed"] = timings()
print("speed", json.dumps(doc["speed"]), flush=True)
if not timings_only:
    doc["fine_tuning"] = arms()
else:
    doc["fine_tuning"] = "not run (--timings-only)"
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print("written", out_path)

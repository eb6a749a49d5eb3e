"""The wide learner-group form (LearnerGroup(form="wide")) on the tuned grid, measured: (a) the 45 points the tuned group forms cannot
hold (BATCH 150 and / or (300, 600)) x 4 seeds as one wide group, (b) all 81 points x 4 seeds as one wide group, (c) the same wide
learners one Agent at a time on the single-learner wide path (a sample of learners x updates, extrapolated), (d) for context the 36
runnable points x 4 seeds as one tuned throughput group.  Writes profiles/r08_group_wide_run.json (or --out).

    python tools/group_wide_demo.py [--envs 128] [--seeds 4] [--reps 20] [--only a] [--out PATH]

FLOPs are counted on every learner's LIVE batch at the group's padded width (what the kernels compute; the zero rows of a pass are
not counted): 10 layer passes per update (4 forwards, the critic's backward with its parameter gradient, the critic forward and
backward of the actor loss, the actor's backward) x 2 x MAC(l1, l2) x batch, MAC = the mean of the actor's and critic's
multiply-adds per sample.  HBM bytes: the ADAM / soft-update sweep and the gradient stores, 40 B per parameter."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
PEAK_FP32_MFMA = 157.3e12          # MI355X fp32 MFMA peak (tools/README.md)
PEAK_HBM = 8.0e12                  # MI355X HBM3E peak


def mac(l1, l2):
    return 0.5 * ((9 * l1 + l1 * l2 + 2 * l2) + (11 * l1 + l1 * l2 + l2))


def update_flops(recs, width):
    return sum(10 * 2 * mac(*width) * r["batch"] for r in recs)


def update_bytes(S, width, count):
    import ctypes as C
    L = S._capi.lib()
    na, nc = C.c_int64(0), C.c_int64(0)
    S._capi.check(L.shems_wide_params(*width, C.byref(na), C.byref(nc)))
    return count * (na.value + nc.value) * 40


def timed(torch, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_group(S, torch, G, recs, E, reps, cap, form="wide"):
    tab = S.tables.synthetic_table("train", 98)
    n = len(recs) * E
    env = S.ShemsBatch(n, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    t0 = time.time()
    grp = G.LearnerGroup(len(recs), E, seed=1231, rng_seed=7, capacity=cap, form=form, hparams=recs)
    grp.populate_memory(env, seed=5)
    grp.min_max_buffer()
    env.reset_(3, episode=1)
    setup_s = time.time() - t0
    tick = [0]

    def upd():
        grp.replay(tick=tick[0])
        tick[0] += 1

    def act():
        grp.act_step(env, train=True, tick=tick[0], window=(grp.rings[0].pos, *grp.ring_window(72)))
        tick[0] += 1
    ms_replay = timed(torch, upd, reps)
    ms_act = timed(torch, act, reps)
    env.check_error()
    ok = bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())     # networks, moments, gradients
    out = dict(form=grp.form, learners=len(recs), envs_per_learner=E, ring_capacity=cap, hidden=list(grp.hidden) if grp.hidden else [250, 500],
               max_batch=getattr(grp, "max_batch", max(r["batch"] for r in recs)), setup_s=round(setup_s, 2), ms_per_replay=round(ms_replay, 4),
               ms_per_act_step=round(ms_act, 4), learner_updates_per_s=round(len(recs) / (ms_replay * 1e-3), 1), finite=ok, reps=reps)
    env.close()
    del grp
    torch.cuda.empty_cache()
    return out


def with_rates(S, out, recs, width):
    fl = update_flops(recs, width)
    by = update_bytes(S, width, len(recs))
    s = out["ms_per_replay"] * 1e-3
    out.update(gflop_per_group_update=round(fl / 1e9, 2), tflops=round(fl / s / 1e12, 2), mfma_fraction=round(fl / s / PEAK_FP32_MFMA, 4),
               adam_grad_gb_per_group_update=round(by / 1e9, 3), adam_grad_tb_per_s=round(by / s / 1e12, 3),
               hbm_fraction_adam_grad=round(by / s / PEAK_HBM, 4))
    return out


def baseline(S, torch, D, recs, E, learners, updates, cap):
    """(c): one Agent at a time on the single-learner wide path, `learners` of the records x `updates`; extrapolated to len(recs)."""
    tab = S.tables.synthetic_table("train", 98)
    env = S.ShemsBatch(E, 72, [tab], [S.make_config(98, 0, tab.shape[0])]).use_torch_stream()
    ring = D.ReplayRing(cap)
    D.Agent(seed=1, hidden=(300, 600)).populate_memory(env, ring, seed=5)
    total_ms, n = 0.0, 0
    for l in range(learners):
        r = recs[(l * len(recs)) // learners]
        ag = D.Agent(seed=100 + l, hidden=r["hidden"], wide=True)
        ag.batch = r["batch"]
        ag.set_norm(ring.s.min(0).values.cpu().numpy(), ring.s.max(0).values.cpu().numpy())
        tick = [0]

        def upd():
            ag.replay(ring, tick=tick[0])
            tick[0] += 1
        total_ms += timed(torch, upd, updates) * updates
        n += updates
    ms_per_update = total_ms / n
    env.close()
    return dict(form="single-learner wide path, one Agent at a time", sampled_learners=learners, updates_each=updates,
                ms_per_learner_update=round(ms_per_update, 4), learner_updates_per_s=round(1e3 / ms_per_update, 1),
                extrapolated_to_learners=len(recs), extrapolated_ms_per_round=round(ms_per_update * len(recs), 3),
                note="extrapolated: the sampled learners' mean time per update times the group's learner count")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cap", type=int, default=2400)
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_group_wide_run.json"))
    a = ap.parse_args()
    import importlib
    import torch
    S = importlib.import_module(PKG)
    D = importlib.import_module(PKG + ".ddpg")
    G = importlib.import_module(PKG + ".group")
    wide_codes = [c for c in G.TUNED_ALL if c not in G.TUNED_RUNNABLE]
    res = dict(device=torch.cuda.get_device_name(0), envs_per_learner=a.envs, seeds=a.seeds, peak_fp32_mfma_tflops=PEAK_FP32_MFMA / 1e12,
               peak_hbm_tbs=PEAK_HBM / 1e12, flop_model=__doc__.split("FLOPs")[1].strip())
    recs_a = G.tuned_grid(wide_codes, seeds=a.seeds, wide=True)[0]
    recs_b = G.tuned_grid(G.TUNED_ALL, seeds=a.seeds, wide=True)[0]
    if "a" in a.only:
        res["a_45_wide_points"] = with_rates(S, run_group(S, torch, G, recs_a, a.envs, a.reps, a.cap), recs_a, (300, 600))
        print(json.dumps(res["a_45_wide_points"]), flush=True)
    if "b" in a.only:
        res["b_all_81_points"] = with_rates(S, run_group(S, torch, G, recs_b, a.envs, a.reps, a.cap), recs_b, (300, 600))
        print(json.dumps(res["b_all_81_points"]), flush=True)
    if "c" in a.only:
        res["c_baseline_single_wide"] = baseline(S, torch, D, recs_a, a.envs, 20, 50, a.cap)
        print(json.dumps(res["c_baseline_single_wide"]), flush=True)
        if "a_45_wide_points" in res:
            res["a_over_c_learner_updates"] = round(res["a_45_wide_points"]["learner_updates_per_s"] /
                                                    res["c_baseline_single_wide"]["learner_updates_per_s"], 2)
    if "d" in a.only:
        recs_d = G.tuned_grid(G.TUNED_RUNNABLE, seeds=a.seeds)[0]
        res["d_36_tuned_points_tuned_group"] = run_group(S, torch, G, recs_d, a.envs, a.reps, a.cap, form=None)
        print(json.dumps(res["d_36_tuned_points_tuned_group"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

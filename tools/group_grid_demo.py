"""A slice of the tuned hyper-parameter grid (input09_08_on_01-09_eval.jl:62-106, main.set_hyperparameters) trained as ONE learner group
with per-learner hyper-parameters: points x seeds x chargers learners (learner (p * seeds + s) * chargers + c runs point p with seed s on
charger profile ids[c]), each on --envs households, trained by the grouped launches for --episodes episodes of 72 hours, then every
learner's deterministic evaluation on its charger's eval table (100 starts, 72 hours) next to the rule-based controller.  Writes one JSON
document: per point and charger the mean / spread of the seeds' scores, wall time, learner-updates/s, and the points the group cannot run.

--timing instead times, in one process and with one clock (time.perf_counter around synchronised runs of --steps fused act/step +
grouped update steps after --warmup):
  (a) the homogeneous 400 x 128 group on the shared entry points,
  (b) the same group through the per-learner entry points with uniform (default) records,
  (c) a heterogeneous 400 x 128 group cycling the 36 runnable tuned points,
alternating a / b / c over --repeats, and
  (d) --slice points x --seeds learners as one group against the same points run one group per point (the shared entry points, the
      point's values in every learner), one after the other.
"""
import argparse
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
G = importlib.import_module(PKG + ".group")
IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 98)
EP = 72


def _env(n, E, charger_of_learner):
    tabs = [S.tables.synthetic_table("train", c) for c in IDS]
    row0 = np.cumsum([0] + [t.shape[0] for t in tabs])
    cfgs = [S.make_config(c, row0[k], tabs[k].shape[0]) for k, c in enumerate(IDS)]
    co = np.repeat(np.asarray(charger_of_learner, np.uint16), E)
    return S.ShemsBatch(n, EP, tabs, cfgs, co).use_torch_stream()


def _points(spec):
    if spec.startswith("runnable"):
        k = int(spec.split(":")[1]) if ":" in spec else len(G.TUNED_RUNNABLE)
        return list(G.TUNED_RUNNABLE[:k])
    return [p.strip() for p in spec.split(",") if p.strip()]


def run(a):
    recs, points, skipped = G.tuned_grid(_points(a.points), a.seeds, a.chargers)
    if not points:
        raise SystemExit(f"no runnable point among {a.points}: {skipped}")
    L, E = len(recs), a.envs
    env = _env(L * E, E, [l % a.chargers for l in range(L)])
    grp = G.LearnerGroup(L, E, seed=1231, rng_seed=99, hparams=recs)
    grp.populate_memory(env)
    grp.min_max_buffer()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for ep in range(1, a.episodes + 1):
        grp.episode_(env, train=True, rng_ep=7, episode=ep, window_count=a.window)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    grp.flux_()
    finite = bool(torch.isfinite(grp.slab[:, :grp.layout["ws"][0]]).all())
    scores, rule = np.zeros(L), {}
    for k, cid in enumerate(IDS[:a.chargers]):
        ev = S.tables.synthetic_table("eval", cid)
        env_eval = S.ShemsBatch(100, 1439, [ev], [S.make_config(cid, 0, ev.shape[0])]).use_torch_stream()
        env_eval.reset_(123, episode=1)
        rule[cid] = float(env_eval.rollout("rule", EP).mean().item())
        for l in range(k, L, a.chargers):
            scores[l] = float(grp.learners[l].episode_(env_eval, None, train=False, num_steps=EP, rng_ep=123, episode=1).mean().item())
        env_eval.close()
    per_point = {}
    for p, jid in enumerate(points):
        rows = {}
        for c, cid in enumerate(IDS[:a.chargers]):
            s = np.array([scores[(p * a.seeds + sd) * a.chargers + c] for sd in range(a.seeds)])
            rows[str(cid)] = dict(mean=float(s.mean()), std=float(s.std()), min=float(s.min()), max=float(s.max()), rule_based=rule[cid])
        h = grp.hparams[p * a.seeds * a.chargers]
        per_point[jid] = dict(hparams={k: (list(v) if isinstance(v, tuple) else v) for k, v in h.items()}, chargers=rows)
    updates = a.episodes * EP
    return dict(learners=L, envs_per_learner=E, points=points, seeds=a.seeds, chargers=list(IDS[:a.chargers]), skipped=skipped,
                episodes=a.episodes, window_count=a.window, train_wall_s=wall, learner_updates_per_s=L * updates / wall,
                finite_state=finite, per_point=per_point, device=torch.cuda.get_device_name(0))


def _steps(grp, env, k, t0=0):
    for t in range(t0, t0 + k):
        if t % EP == 0:
            env.reset_(7, episode=1 + t // EP)
        grp.act_step(env, train=True, tick=t, window=(grp.rings[0].pos, *grp.ring_window(EP, None)))
        grp.replay()
        grp.tick += 1


def _timed(grp, env, a):
    _steps(grp, env, a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _steps(grp, env, a.steps, a.warmup)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _build(L, E, hparams=None, values=None):
    env = _env(L * E, E, [0] * L)
    grp = G.LearnerGroup(L, E, seed=1231, rng_seed=99, form="throughput", hparams=hparams)
    if values is not None:                     # the shared entry points: learner 0's values hold for the whole group
        for ag in grp.learners:
            ag.eta_act, ag.eta_crit, ag.gamma, ag.tau, ag.batch, ag.sigma = (values[k] for k in ("eta_act", "eta_crit", "gamma", "tau", "batch", "sigma"))
    grp.populate_memory(env)
    grp.min_max_buffer()
    env.reset_(7, episode=1)
    return grp, env


def timing(a):
    L, E = 400, 128
    runnable = G.tuned_grid(G.TUNED_RUNNABLE)[0]
    make = {"a_shared": lambda: _build(L, E), "b_hp_uniform": lambda: _build(L, E, hparams=[{}] * L),
            "c_hp_36_points": lambda: _build(L, E, hparams=[runnable[l % 36] for l in range(L)])}
    forms = {k: f() for k, f in make.items() if k[0] in a.forms}
    times = {k: [] for k in forms}
    for r in range(a.repeats):
        for k, (grp, env) in forms.items():
            times[k].append(_timed(grp, env, a))
    abc = {}
    for k, ts in times.items():
        ups = [L * a.steps / t for t in ts]
        abc[k] = dict(step_ms=[1e3 * t / a.steps for t in ts], learner_updates_per_s=ups, median_updates_per_s=float(np.median(ups)))
    med = {k: v["median_updates_per_s"] for k, v in abc.items()}
    del forms
    torch.cuda.empty_cache()
    res = dict(shape=f"{L} x {E}", steps=a.steps, warmup=a.warmup, repeats=a.repeats, clock="time.perf_counter around synchronised runs",
               abc=abc, device=torch.cuda.get_device_name(0))
    if len(med) == 3:
        res.update(b_over_a=med["b_hp_uniform"] / med["a_shared"], c_over_b=med["c_hp_36_points"] / med["b_hp_uniform"])
    if "d" not in a.forms:
        return res
    # (d) a grid slice as one group against one group per point
    pts = _points(a.slice)
    recs, points, _ = G.tuned_grid(pts, a.seeds, 1)
    grp, env = _build(len(recs), E, hparams=recs)
    t_one = _timed(grp, env, a)
    del grp, env
    t_per = []
    for p in range(len(points)):
        grp, env = _build(a.seeds, E, values=recs[p * a.seeds])
        t_per.append(_timed(grp, env, a))
        del grp, env
    n = len(recs)
    d = dict(points=points, seeds=a.seeds, learners=n, one_group_s=t_one, one_group_updates_per_s=n * a.steps / t_one,
             per_point_groups_s=float(sum(t_per)), per_point_groups_updates_per_s=n * a.steps / sum(t_per), per_point_s=t_per,
             gain=float(sum(t_per) / t_one), note="per-point groups: throughput form, the point's values in every learner")
    res["slice"] = d
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="group_grid.json")
    ap.add_argument("--points", default="runnable:6", help="JOB_IDs (comma separated; the last two digits pick the point) or runnable[:N]")
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--chargers", type=int, default=1)
    ap.add_argument("--envs", type=int, default=128, help="households per learner (a multiple of 32)")
    ap.add_argument("--window", type=int, default=None, help="window_count: transitions each learner remembers per step (default: rotating)")
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--steps", type=int, default=72)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forms", default="abcd", help="--timing: which of (a) (b) (c) (d) to run (e.g. bc for a profiler run)")
    ap.add_argument("--slice", default="runnable:12", help="(d): the points of the slice")
    a = ap.parse_args()
    res = timing(a) if a.timing else run(a)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("per_point",)})[:2000])


if __name__ == "__main__":
    main()

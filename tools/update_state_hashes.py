"""The state every update form of the single learner and of the learner groups leaves after three updates, hashed -- once with this tree's
Python and once with another checkout's (`--parent DIR`, a directory that holds the package), both on THIS tree's library (SHEMS_HIP_LIB),
each in a fresh child process.  A refactor of the Python half must leave every hash equal.

    python tools/update_state_hashes.py --parent /path/to/parent/checkout [--out profiles/NAME.txt]
    python tools/update_state_hashes.py --child ROOT          (what the parent process starts: prints one JSON line)

Paths: fused / tiled / split replay, publish, exclude, batch 150 (sub-batches), parameter noise, a PrioritizedRing, replay_given, clone,
evaluate, bc, TD3 over policy and critic steps, TD3 with bc; a LearnerGroup, a PrioritizedLearnerGroup and a TD3LearnerGroup of 2 x 32
envs.  Rings of 400 slots, batch 120 (150 on the sub-batch path).  Hashed: every learner tensor (a group: its whole slab) and the host
state bp_actor, bp_critic, updates, clones, evaluations."""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, UPDATES = 400, 3


def child(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    D, G, T = (importlib.import_module(f"{PKG}.{m}") for m in ("ddpg", "group", "td3"))
    S = importlib.import_module(PKG)
    rng = np.random.default_rng(5)
    data = dict(s=rng.random((CAP, 9), np.float32) * 5, a=rng.random((CAP, 2), np.float32) * 2 - 1, r=rng.random(CAP, np.float32) - 0.5,
                s2=rng.random((CAP, 9), np.float32) * 5, done=(rng.random(CAP) < 0.1).astype(np.uint8))

    def fill(ring):
        for k, v in data.items():
            getattr(ring, k).copy_(torch.from_numpy(v))
        ring.pushed = CAP
        return ring

    def h(t):
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]

    def host(ag):
        return [repr((ag.bp_actor, ag.bp_critic, ag.updates, ag.clones, ag.evaluations))]

    def agent(cls=D.Agent, batch=120, **kw):
        ag = cls(seed=1231, rng_seed=77, **kw)
        ag.batch = batch
        ag.set_norm(data["s"].min(0), data["s"].max(0))
        return ag

    def state(ag, extra=()):
        return [h(getattr(ag, k)) for k in ag._LEARNER_TENSORS] + [h(x) for x in extra] + host(ag)

    out = {}

    def single(name, step, setup=None, ring=None, cls=D.Agent, **kw):
        ag = agent(cls, **kw)
        ring = fill(D.ReplayRing(CAP)) if ring is None else ring
        extra = setup(ag) if setup else ()
        for _ in range(UPDATES):
            step(ag, ring)
        out[name] = state(ag, extra)

    pub = torch.zeros(D.N_ACTOR, device="cuda")
    per = fill(D.PrioritizedRing(CAP))
    ones = torch.ones(128, device="cuda")

    def given(ag, ring):
        idx = np.full(128, -1, np.int32)
        idx[:ag.batch] = ag.sample_indices(ag.updates, len(ring))
        ag.replay_given(ring, torch.from_numpy(idx).cuda(), ones)

    single("replay fused, Flux", lambda ag, r: ag.replay(r))
    single("replay fused, tiled", lambda ag, r: ag.replay(r), setup=lambda ag: ag.use_tiled(True) and ())
    single("replay split (fused=False)", lambda ag, r: ag.replay(r), setup=lambda ag: setattr(ag, "fused", False) or ())
    single("replay publish", lambda ag, r: ag.replay(r, publish=pub), setup=lambda ag: (pub,))
    single("replay exclude", lambda ag, r: ag.replay(r, exclude=(CAP - 20, 40)))
    single("replay batch 150", lambda ag, r: ag.replay(r), batch=150)
    single("replay pn", lambda ag, r: ag.replay(r), noise_type="pn")
    single("prioritized replay", lambda ag, r: ag.replay(r), ring=per, setup=lambda ag: (per.prio,))
    single("replay_given", given)
    single("clone", lambda ag, r: ag.clone(r))
    single("evaluate", lambda ag, r: ag.evaluate(r))
    single("replay bc", lambda ag, r: ag.replay(r), bc=D.BC(2.5, 1.0))
    single("TD3 (updates 0..2: critic, policy, critic)", lambda ag, r: ag.replay(r), cls=T.TD3Agent)
    single("TD3 policy steps", lambda ag, r: ag.replay(r, update_policy=True), cls=T.TD3Agent)
    single("TD3 bc", lambda ag, r: ag.replay(r), cls=T.TD3Agent, bc=D.BC(2.5, 0.5))

    for name, make in (("LearnerGroup 2 x 32", lambda: G.LearnerGroup(2, 32, seed=1231, rng_seed=77, capacity=CAP)),
                       ("LearnerGroup 2 x 32, latency", lambda: G.LearnerGroup(2, 32, seed=1231, rng_seed=77, capacity=CAP, form="latency")),
                       ("PrioritizedLearnerGroup 2 x 32", lambda: G.PrioritizedLearnerGroup(2, 32, seed=1231, rng_seed=77, capacity=CAP)),
                       ("TD3LearnerGroup 2 x 32", lambda: T.TD3LearnerGroup(2, 32, seed=1231, rng_seed=77, capacity=CAP))):
        grp = make()
        for ag, ring in zip(grp.learners, grp.rings):
            ag.set_norm(data["s"].min(0), data["s"].max(0))
            fill(ring)
        for _ in range(UPDATES):
            grp.replay()
        if name == "LearnerGroup 2 x 32":                     # the two half updates of the throughput form ride on the same group
            grp.clone(None)
            grp.evaluate(None)
        grp.flux_()
        out[name] = [h(grp.slab)] + [x for ag in grp.learners for x in host(ag)] + [repr((grp.updates, grp.clones, grp.evaluations))]
    torch.cuda.synchronize()
    print("HASHES " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    env = dict(os.environ, SHEMS_HIP_LIB=os.path.join(HERE, PKG, "libshems_hip.so"))
    got = {}
    for who, root in (("tree", HERE), ("parent", os.path.abspath(a.parent))):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], env=env, capture_output=True, text=True, timeout=600)
        lines = [x for x in p.stdout.splitlines() if x.startswith("HASHES ")]
        if p.returncode != 0 or not lines:
            sys.exit(f"{who}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        got[who] = json.loads(lines[-1][7:])
    rows, total, equal = [], 0, 0
    for name in got["tree"]:
        t, q = got["tree"][name], got["parent"][name]
        n, e = len(t), sum(x == y for x, y in zip(t, q)) if len(t) == len(q) else 0
        total, equal = total + n, equal + e
        digest = lambda v: hashlib.sha256("".join(v).encode()).hexdigest()[:16]
        rows.append(f"{name:46s} {n:3d} hashes  equal {e:3d}  tree {digest(t)}  parent {digest(q)}")
    rows.append(f"total: {total} hashes, {equal} equal")
    text = "\n".join(rows) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if equal == total else 1)


if __name__ == "__main__":
    main()

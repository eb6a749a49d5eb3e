"""NumPy twin of one round of population-based training (include/shems_hip.h): the order, the quota, the parent draw and the
explore arithmetic, written independently of csrc/shems_pbt_core.h (test infrastructure)."""
import math

import numpy as np

import philox_np as PH

f32, f64 = np.float32, np.float64
STREAM_PBT = 0x5042545F
FIELDS = ("eta_act", "eta_crit", "tau", "noise_sigma")             # bits 0 .. 3 of the mask and of the draw's word y
REC = np.dtype([("eta_act", "<f8"), ("eta_crit", "<f8"), ("gamma", "<f4"), ("tau", "<f4"), ("noise_mu", "<f4"), ("noise_sigma", "<f4"),
                ("batch", "<i4"), ("reserved", "<i4")])            # shems_group_hparams
assert REC.itemsize == 40
DEFAULT_LO = (float(f32(1e-6)), float(f32(1e-6)), float(f32(1e-4)), 0.0)
DEFAULT_HI = (float(f32(1e-1)), float(f32(1e-1)), 1.0, 10.0)


def params(seed=7, round=0, permille=250, fields=15, down=0.8, up=1.2, lo=DEFAULT_LO, hi=DEFAULT_HI):
    return dict(seed=int(seed), round=int(round), permille=int(permille), fields=int(fields), down=float(down), up=float(up),
                lo=tuple(float(x) for x in lo), hi=tuple(float(x) for x in hi))


def records(count, rng=None):
    """`count` distinct valid records (every field differs between learners, so a wrong parent shows in every byte)."""
    hp = np.zeros(count, REC)
    l = np.arange(count)
    hp["eta_act"] = (f32(1e-4) * (1 + l).astype(f32)).astype(f64)
    hp["eta_crit"] = (f32(1e-3) * (1 + l % 5).astype(f32) + f32(1e-5) * l.astype(f32)).astype(f64)
    hp["gamma"] = f32(0.99) - f32(0.001) * l.astype(f32)
    hp["tau"] = f32(0.001) * (1 + l % 7).astype(f32)
    hp["noise_mu"] = f32(0.01) * (l % 3).astype(f32)
    hp["noise_sigma"] = f32(0.05) * (1 + l % 4).astype(f32)
    hp["batch"] = 16 + (l % 100)
    return hp


def better(sa, a, sb, b):
    fa, fb = math.isfinite(sa), math.isfinite(sb)
    if fa != fb:
        return fa
    if fa and sa != sb:
        return sa > sb
    return a < b


def ranks(pop, score):
    pop, score = np.asarray(pop), np.asarray(score, f64)
    n = len(pop)
    return np.array([sum(1 for m in range(n) if m != l and pop[m] == pop[l] and better(float(score[m]), m, float(score[l]), l))
                     for l in range(n)], np.int32)


def explore_eta(eta, f, lo, hi):
    v = f64(f32(f64(eta) * f64(f)))
    return f64(min(max(v, f64(lo)), f64(hi)))


def explore_f32(x, f, lo, hi):
    v = f64(f32(f64(f32(x)) * f64(f)))
    return f32(min(max(v, f64(lo)), f64(hi)))


def round_twin(p, pop, score, hp):
    """(records after the round, parent int32 [count], rank int32 [count]); hp is not modified."""
    pop, score = np.asarray(pop, np.int32), np.asarray(score, f64)
    n = len(pop)
    rank = ranks(pop, score)
    out, parent = hp.copy(), np.arange(n, dtype=np.int32)
    for l in range(n):
        members = [m for m in range(n) if pop[m] == pop[l]]
        P = len(members)
        q = (P * p["permille"]) // 1000
        if q == 0 or rank[l] < P - q:
            continue
        x, y, _, _ = PH.philox4x32_10(l, p["round"], 0, STREAM_PBT, p["seed"] & 0xFFFFFFFF, (p["seed"] >> 32) & 0xFFFFFFFF)
        j = (int(x) * q) >> 32
        par = next(m for m in members if rank[m] == j)
        if par == l or not math.isfinite(float(score[par])):
            continue
        parent[l] = par
        rec = hp[par].copy()
        y = int(y)
        for k, name in enumerate(FIELDS):
            if not p["fields"] >> k & 1:
                continue
            f = p["up"] if y >> k & 1 else p["down"]
            rec[name] = explore_eta(rec[name], f, p["lo"][k], p["hi"][k]) if k < 2 else explore_f32(rec[name], f, p["lo"][k], p["hi"][k])
        out[l] = rec
    return out, parent, rank


def copy_twin(slab, ranges, parent):
    """slab [count][stride] float32 after shems_pbt_copy_dev: every child's ranges are its parent's pre-round bytes."""
    out = slab.copy()
    for l, p in enumerate(parent):
        if p != l:
            for o, n in ranges:
                out[l, o:o + n] = slab[p, o:o + n]
    return out

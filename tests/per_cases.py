"""The sampler cases of prioritized replay, shared by tests/test_per_host.py (which asserts on the NumPy twin that every case covers
what it is there for) and tests/test_per_gpu.py (which runs them on the device).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import per_ref as PR

f32 = np.float32
RINGS = ((1, 1), (255, 300), (256, 256), (257, 1000), (1000, 1000), (24000, 24000))      # (ring_len, capacity)
BATCHES = (1, 17, 120, 128)


def priorities(kind, capacity, ring_len, rng):
    """prio [capacity]; the slots outside [0, ring_len) hold a sentinel the sampler must neither read into a sum nor overwrite."""
    p = np.full(capacity, f32(-7.5), f32)
    if kind == "random":
        v = (rng.random(ring_len) ** 3 * 4 + 1e-3).astype(f32)
    elif kind == "decades":                       # four decades
        v = (10.0 ** rng.uniform(-2, 2, ring_len)).astype(f32)
        v[ring_len // 3], v[ring_len // 2] = f32(1e-2), f32(1e2)       # the span is four decades exactly
    elif kind == "heavy":                         # a few slots that each cover several strata: some columns share a slot, others do not
        v = (rng.random(ring_len) * 0.5 + 0.01).astype(f32)
        v[rng.choice(ring_len, 5, replace=False)] = f32(60.0)
    elif kind == "zeros":
        v = (rng.random(ring_len) * 2).astype(f32)
        v[rng.random(ring_len) < 0.3] = 0
        v[0] = 0
        v[ring_len - 1] = 0
    elif kind == "one_slot":
        v = np.zeros(ring_len, f32)
        v[(ring_len * 5) // 8] = f32(3.25)
    elif kind == "last_block":
        v = np.zeros(ring_len, f32)
        lo = (PR.n_blocks(ring_len) - 1) * PR.BLOCK
        v[lo:] = (rng.random(ring_len - lo) + 0.5).astype(f32)
    else:
        raise ValueError(kind)
    p[:ring_len] = v
    return p


def sampler_cases():
    """[(name, dict(capacity, ring_len, batch, kind, fresh=(pos, count), pmax, beta, seed, tick))]"""
    out = []
    k = 0
    for ring_len, cap in RINGS:
        for batch in BATCHES:
            out.append((f"random-{ring_len}of{cap}-b{batch}", dict(capacity=cap, ring_len=ring_len, batch=batch, kind="random", fresh=(0, 0),
                                                                   pmax=1.0, beta=0.4, seed=11 + k, tick=3 + 7 * k)))
            k += 1
    for ring_len, cap in ((1000, 1000), (24000, 24000)):
        for kind in ("zeros", "one_slot", "last_block", "decades"):
            out.append((f"{kind}-{ring_len}", dict(capacity=cap, ring_len=ring_len, batch=120, kind=kind, fresh=(0, 0), pmax=1.0, beta=0.4,
                                                   seed=(5 << 32) | 7, tick=0xFFFFFFFF if kind == "zeros" else 21)))
    for name, ring_len, fresh in (("empty", 1000, (5, 0)), ("one", 1000, (999, 1)), ("wrap", 1000, (990, 30)), ("all", 1000, (3, 1000)),
                                  ("more", 1000, (3, 5000)), ("partial", 600, (580, 20))):
        out.append((f"fresh-{name}", dict(capacity=1000, ring_len=ring_len, batch=17, kind="random", fresh=fresh, pmax=2.5, beta=1.0, seed=3,
                                          tick=1)))
    out.append(("beta0", dict(capacity=1000, ring_len=1000, batch=120, kind="decades", fresh=(0, 0), pmax=1.0, beta=0.0, seed=3, tick=2)))
    return out


UPDATE_SEED = 11                                  # tests/test_per_gpu.py:_setup: the learner's seed; the priorities' generator takes seed + 1


def update_cases():
    """The rings of the update tests (every stage, write-back): [(name, capacity, batch, kind, want_duplicates)].  The 24 000-slot ring
    with priorities over four decades at the four batches (no column shares a slot), and a 1 000-slot ring with five heavy slots at
    batch 120, where some columns share a slot and others do not."""
    return [(f"decades-b{b}", 24000, b, "decades", False) for b in BATCHES] + [("heavy-b120", 1000, 120, "heavy", True)]


def update_priorities(kind, capacity, seed=UPDATE_SEED):
    return priorities(kind, capacity, capacity, np.random.default_rng(seed + 1))


def build(case, rng_seed=0):
    """The inputs of a case: prio [capacity] (before the fresh fill)."""
    rng = np.random.default_rng(rng_seed + case["ring_len"] + 13 * case["batch"])
    return priorities(case["kind"], case["capacity"], case["ring_len"], rng)


def twin(case, prio):
    p = prio.copy()
    d = PR.sample(p, case["pmax"], case["capacity"], case["ring_len"], case["fresh"][0], case["fresh"][1], case["seed"], case["tick"],
                  case["batch"], case["beta"])
    d["prio"] = p
    return d


def check_coverage(name, case, prio, tw):
    """What each case is there for, asserted on the twin."""
    b, n, cap = case["batch"], case["ring_len"], case["capacity"]
    live = tw["idx"][:b]
    assert (live >= 0).all() and (live < n).all() and (tw["idx"][b:] == -1).all(), name
    assert (tw["w"][:b] > 0).all() and tw["w"][:b].max() == 1 and not tw["w"][b:].any(), name
    assert np.array_equal(tw["prio"][n:], prio[n:]), name
    assert (np.diff(live) >= 0).all(), (name, "stratified targets ascend")
    kind = case["kind"]
    if kind == "zeros":
        assert (tw["prio"][live] > 0).all() and (prio[:n] == 0).mean() > 0.2, name
    if kind == "one_slot":
        assert (live == (n * 5) // 8).all(), name
    if kind == "last_block":
        assert (live >= (PR.n_blocks(n) - 1) * PR.BLOCK).all() and n % PR.BLOCK != 0, name
    if kind == "decades":
        assert prio[:n].max() / prio[:n].min() >= 1e4, name
    if name.startswith("fresh-"):
        fm = tw["fresh"]
        want = {"empty": 0, "one": 1, "wrap": 30, "all": n, "more": n, "partial": 20}[name[6:]]
        assert fm.sum() == want and (tw["prio"][:n][fm] == f32(case["pmax"])).all() and np.array_equal(tw["prio"][:n][~fm], prio[:n][~fm]), name
        if name == "fresh-wrap":
            assert fm[0] and fm[n - 1] and not fm[500], name
    if case["beta"] == 0.0:
        assert (tw["w"][:b] == 1).all(), name

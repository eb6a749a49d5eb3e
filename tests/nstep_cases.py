"""The cases of the n-step tests, shared by the host build (tests/test_nstep_host.py) and the GPU tests (tests/test_nstep_gpu.py): every
case the GPU test runs is held to the twin on the host too.  Shapes are the smallest at which the kernels can go wrong: windows of 1,
33 (no multiple of anything, wraps the ring mid-window from position 90 of 100) and 64, n at both ends of its range, T = n."""
import numpy as np

import nstep_ref as NR

f32 = np.float32
CAPACITY, POS0, GAMMA = 100, 90, f32(0.99)
FOLD_N, FOLD_WINDOWS, EPISODES = (1, 2, 3, 5, 16), (1, 33, 64), 2


def fold_cases():
    """(name, dict(n, window, T, capacity, pos0, episodes, gamma)): T = 6 (16 for n = 16) and T = n (one push per episode; for n = 1
    that is an episode of one hour)."""
    out = []
    for n in FOLD_N:
        for w in FOLD_WINDOWS:
            for T in sorted({max(6, n), n}):
                out.append((f"n{n}-w{w}-T{T}", dict(n=n, window=w, T=T, capacity=CAPACITY, pos0=POS0, episodes=EPISODES, gamma=GAMMA)))
    return out


def staging(case, seed=0):
    """The hand-made staging rings of a fold case, one per hour of every episode: [episodes * T] dicts of s [w][9], a [w][2], r [w],
    s2 [w][9], done [w].  Rewards span six decades and both signs (so the float32 rounding of G matters); s carries (episode, hour,
    household) so that a window crossing a reset or a household shows; done is set now and then (the fold copies the newest byte)."""
    rng = np.random.default_rng(1000 * case["n"] + case["window"] + seed)
    w, out = case["window"], []
    for e in range(case["episodes"]):
        for h in range(case["T"]):
            s = rng.normal(0, 1, (w, 9)).astype(f32)
            s[:, 0], s[:, 1], s[:, 2] = e, h, np.arange(w)
            r = (rng.normal(0, 1, w) * 10.0 ** rng.integers(-3, 3, w)).astype(f32)
            out.append(dict(s=s, a=rng.uniform(-1, 1, (w, 2)).astype(f32), r=r, s2=(s + f32(0.5)).astype(f32),
                            done=(rng.random(w) < 0.2).astype(np.uint8)))
    return out


def fold_twin(case, stages):
    """(ring, pushed) after every hour of every episode went through the twin's fold."""
    ring, pushed = NR.new_ring(case["capacity"]), case["pos0"]
    fold = NR.Fold(case["n"], case["window"], case["gamma"])
    for i, st in enumerate(stages):
        pushed = fold.fold(st, ring, pushed, i % case["T"])
    return ring, pushed


def bulk_cases():
    """Capacity 100, T = 6, n in {1, 3, 6}; episodes * m below the capacity (5 episodes) and above it (40: m = 6, 4, 1 -> 240, 160, 40
    pushes for n = 1, 3, 6 -- so n = 6 gets 120 episodes for its skip case)."""
    out = []
    for n in (1, 3, 6):
        m = 6 - n + 1
        for episodes in (5, 40 if 40 * m > CAPACITY else 120):
            out.append((f"n{n}-e{episodes}", dict(n=n, T=6, episodes=episodes, capacity=CAPACITY, pos0=POS0, gamma=GAMMA,
                                                   skips=episodes * m > CAPACITY)))
    return out


def bulk_source(case, seed=0):
    rng = np.random.default_rng(77 * case["n"] + case["episodes"] + seed)
    N = case["episodes"] * case["T"]
    s = rng.normal(0, 1, (N, 9)).astype(f32)
    s[:, 0], s[:, 1] = np.arange(N) // case["T"], np.arange(N) % case["T"]
    return dict(s=s, a=rng.uniform(-1, 1, (N, 2)).astype(f32), r=(rng.normal(0, 1, N) * 10.0 ** rng.integers(-3, 3, N)).astype(f32),
                s2=(s + f32(0.5)).astype(f32), done=(rng.random(N) < 0.2).astype(np.uint8))


def bulk_twin(case, src):
    ring = NR.new_ring(case["capacity"])
    pushed = NR.from_episodes(src, case["episodes"], case["T"], case["n"], case["gamma"], ring, case["pos0"])
    return ring, pushed


def ring_bytes(ring):
    """s, a, r, s2, done of a ring (dict of arrays) as one bytes object: what "the ring equals" compares."""
    return b"".join(np.ascontiguousarray(ring[k]).tobytes() for k in ("s", "a", "r", "s2", "done"))

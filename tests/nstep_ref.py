"""NumPy twin of multi-step (n-step) returns (include/shems_hip.h, csrc/shems_nstep_core.h): the Horner return, the host-side discount,
the per-step fold with its per-episode history and the bulk conversion of whole episodes.  A ring is a dict of arrays s [cap][9],
a [cap][2], r [cap], s2 [cap][9] (float32) and done [cap] (uint8).  Everything here is IEEE float64 multiply / add and float32
rounding in a fixed order, so the device and the host build must equal it bit for bit."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
NSTEP_MAX = 16
SENT_F, SENT_B = f32(-777.25), np.uint8(0xAB)          # what an untouched slot keeps in the tests


def nstep_gamma(gamma, n):
    """float32(g64 * g64 * ... * g64), n factors, left to right in float64."""
    g = f64(f32(gamma))
    p = g
    for _ in range(int(n) - 1):
        p = f64(p * g)
    return f32(p)


def horner(r, gamma):
    """r [n, ...] float32, oldest first -> G float32 [...]: acc = r[n-1]; acc = r[k] + gamma64 * acc for k = n-2 .. 0 (float64, the
    product rounded on its own)."""
    r = np.asarray(r, f32)
    g = f64(f32(gamma))
    acc = r[-1].astype(f64)
    for k in range(r.shape[0] - 2, -1, -1):
        p = g * acc                                      # (NumPy rounds every operation: no fused multiply-add)
        acc = r[k].astype(f64) + p
    return acc.astype(f32)


def direct_sum(r, gamma):
    """sum_k gamma64^k r_k for ONE window r [n]: math.fsum over products formed in float64 (the yardstick of the 1-ulp test)."""
    g = float(f32(gamma))
    return math.fsum(float(x) * g ** k for k, x in enumerate(np.asarray(r, f32)))


def new_ring(capacity, sentinel=True):
    z = (lambda *s: np.full(s, SENT_F, f32)) if sentinel else (lambda *s: np.zeros(s, f32))
    return dict(s=z(capacity, 9), a=z(capacity, 2), r=z(capacity), s2=z(capacity, 9),
                done=np.full(capacity, SENT_B if sentinel else 0, np.uint8))


class Fold:
    """The fold's state for one learner: history [n][window][9 | 2 | 1] of the current episode."""

    def __init__(self, n, window, gamma):
        assert 1 <= n <= NSTEP_MAX and window >= 1
        self.n, self.window, self.gamma = int(n), int(window), f32(gamma)
        self.hist_s = np.zeros((n, window, 9), f32)
        self.hist_a = np.zeros((n, window, 2), f32)
        self.hist_r = np.zeros((n, window), f32)

    def fold(self, stage, ring, pushed, hour):
        """stage: the one-step transitions of hour `hour` (counted from the reset) of households [0, window) in slots [0, window).
        Returns the ring's new push count."""
        n, W = self.n, self.window
        slot, old = hour % n, (hour + 1) % n
        cur_s, cur_a, cur_r = stage["s"][:W].copy(), stage["a"][:W].copy(), stage["r"][:W].copy()
        if hour >= n - 1:
            cap = len(ring["r"])
            d = (pushed % cap + np.arange(W)) % cap
            self.hist_s[slot], self.hist_a[slot], self.hist_r[slot] = cur_s, cur_a, cur_r     # (slot != old unless n = 1)
            ring["s"][d], ring["a"][d] = self.hist_s[old], self.hist_a[old]
            ring["r"][d] = horner(np.stack([self.hist_r[(old + k) % n] for k in range(n)]), self.gamma)
            ring["s2"][d], ring["done"][d] = stage["s2"][:W], stage["done"][:W]
            return pushed + W
        self.hist_s[slot], self.hist_a[slot], self.hist_r[slot] = cur_s, cur_a, cur_r
        return pushed


def from_episodes(src, episodes, steps, n, gamma, ring, pushed):
    """src: episode e's hour t at slot e * steps + t.  Pushes episodes * (steps - n + 1) transitions in episode-major order; the ones
    a later push of the same call would overwrite are skipped.  Returns the new push count."""
    m = steps - n + 1
    assert m >= 1
    total, cap = episodes * m, len(ring["r"])
    for q in range(max(0, total - cap), total):
        e, t = divmod(q, m)
        a0 = e * steps + t
        d = (pushed + q) % cap
        ring["s"][d], ring["a"][d] = src["s"][a0], src["a"][a0]
        ring["r"][d] = horner(src["r"][a0:a0 + n], gamma)
        ring["s2"][d], ring["done"][d] = src["s2"][a0 + n - 1], src["done"][a0 + n - 1]
    return pushed + total

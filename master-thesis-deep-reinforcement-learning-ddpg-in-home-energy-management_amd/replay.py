"""GPU-resident circular replay buffer (host-side bookkeeping; the data lives in HBM).

Reference: `memory = CircularBuffer{Any}(MEM_SIZE)` of `[s, a, r, s', done]` (input.jl:139-140),
`remember` (memory_plotting_saving.jl:46-47), `getData` (:31-42).  Here: struct-of-arrays device
tensors (PyTorch is only the allocator) + a host push counter; kernels receive the raw pointers
through `shems_replay` (include/shems_hip.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi


class ReplayRing:
    def __init__(self, capacity, device=None, tensors=None):
        """tensors = (s, a, r, s2, done): views into memory the caller owns (a learner group's slab) instead of new buffers."""
        import torch
        self.capacity = int(capacity)
        if tensors is not None:
            self.s, self.a, self.r, self.s2, self.done = tensors
            self.device = self.s.device
            assert self.s.shape == (self.capacity, _capi.NSTATE) and self.done.dtype == torch.uint8 and self.done.shape == (self.capacity,)
        else:
            # default = the CURRENT device (one process per GPU: bench.py/run_charger.py call set_device(LOCAL_RANK) first);
            # a ring on another GPU than the env/agent would make every kernel dereference unmapped peer memory
            self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            self.s = torch.zeros((self.capacity, _capi.NSTATE), dtype=torch.float32, device=self.device)
            self.a = torch.zeros((self.capacity, _capi.NACTION), dtype=torch.float32, device=self.device)
            self.r = torch.zeros((self.capacity,), dtype=torch.float32, device=self.device)
            self.s2 = torch.zeros((self.capacity, _capi.NSTATE), dtype=torch.float32, device=self.device)
            self.done = torch.zeros((self.capacity,), dtype=torch.uint8, device=self.device)
        self.pushed = 0                      # total transitions ever pushed (host state)

    def __len__(self):                       # length(memory)
        return min(self.pushed, self.capacity)

    @property
    def pos(self):
        return self.pushed % self.capacity

    def struct(self):
        return _capi.Replay(self.capacity, self.s.data_ptr(), self.a.data_ptr(), self.r.data_ptr(),
                            self.s2.data_ptr(), self.done.data_ptr())


PerArgs, PER_MAX_SLOTS, PER_COLS = _capi.PerArgs, _capi.PER_MAX_SLOTS, _capi.PER_COLS
PW_T, PW_IDX, PW_W, PW_U, PW_TM, PW_S = _capi.PW_T, _capi.PW_IDX, _capi.PW_W, _capi.PW_U, _capi.PW_TM, _capi.PW_S
_declare_per = _capi.declare_per


def per_workspace_floats(capacity):
    out = C.c_int64(0)
    _capi.check(_declare_per().shems_per_workspace_floats(int(capacity), C.byref(out)))
    return out.value


class PrioritizedRing(ReplayRing):
    """A replay ring with proportional priorities (Schaul et al. 2016; include/shems_hip.h): prio [capacity] holds
    pi = p^alpha, pmax [1] the running maximum (1.0 at the start), ws the sampler's workspace.  Agent.replay(ring) takes the prioritized
    update when it is handed one: pushes since the last update receive pmax before the draw (`covered` counts the pushes whose
    priorities are set; a ring filled by populate_memory is all fresh at its first update), the drawn slots receive (|q - y| + eps)^alpha
    after it.  beta is read at every update, so the caller may anneal it (ddpg.anneal_beta).  `sampled` / `weights` are views of the
    last draw's slots (-1 in the pad columns) and importance weights."""

    def __init__(self, capacity, alpha=0.6, beta=0.4, eps=1e-6, device=None, tensors=None):
        import math
        import torch
        for name, v in (("alpha", alpha), ("beta", beta), ("eps", eps)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"PrioritizedRing: {name} = {v!r} must be finite and >= 0")
        if beta > 1.0:
            raise ValueError(f"PrioritizedRing: beta = {beta!r} must be in [0, 1]")
        if int(capacity) > PER_MAX_SLOTS:
            raise NotImplementedError(f"PrioritizedRing: capacity {int(capacity)} > {PER_MAX_SLOTS}: the sampler's one workgroup keeps every block sum in LDS")
        super().__init__(capacity, device=device, tensors=tensors)
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        self.prio = torch.zeros((self.capacity,), dtype=torch.float32, device=self.device)
        self.pmax = torch.ones((1,), dtype=torch.float32, device=self.device)
        self.ws = torch.zeros((per_workspace_floats(self.capacity),), dtype=torch.float32, device=self.device)
        self.covered = 0                     # pushes whose priorities are set (host state)

    @property
    def sampled(self):
        import torch
        return self.ws[PW_IDX:PW_IDX + PER_COLS].view(torch.int32)

    @property
    def weights(self):
        return self.ws[PW_W:PW_W + PER_COLS]

    def fresh_range(self):
        """(fresh_pos, fresh_count) of the next update: the pushes since `covered`."""
        n = self.pushed - self.covered
        if n < 0:
            raise ValueError("PrioritizedRing: pushed went backwards")
        return self.covered % self.capacity, min(n, self.capacity)

    def per_struct(self):
        return PerArgs(self.prio.data_ptr(), self.pmax.data_ptr(), self.ws.data_ptr(), self.alpha, self.beta, self.eps, 0)


# ---- multi-step (n-step) returns (include/shems_hip.h) -------------------------------------------------------------------
NSTEP_MAX = _capi.NSTEP_MAX


def check_n_step(n_step, what="n_step"):
    """1 <= n_step <= NSTEP_MAX, an integer: refused by name.  Host only."""
    if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)) or not 1 <= int(n_step) <= NSTEP_MAX:
        raise ValueError(f"{what} = {n_step!r}: the steps of a multi-step return are an integer in 1 .. {NSTEP_MAX}")
    return int(n_step)


def nstep_gamma(gamma, n):
    """gamma_n = float32(g64 * g64 * ... * g64), g64 = float64(float32(gamma)), n factors multiplied left to right in float64: the discount
    every update of an n-step learner bootstraps with.  Computed on the host, once; there is no device pow.  nstep_gamma(g, 1) ==
    float32(g)."""
    n = check_n_step(n, "n")
    g = float(np.float32(gamma))
    p = g
    for _ in range(n - 1):
        p = p * g
    return float(np.float32(p))


class NStepWindow:
    """What an n-step learner keeps beside its ring: the staging ring the unchanged fused step writes the one-step transitions of the
    stationary window of households [0, window_count) into (`window`: the step's shems_ring_window), and the history hist_s / hist_a /
    hist_r [n][window_count][9 | 2 | 1] of the current episode.  fold(ring, hour) runs shems_nstep_fold_dev behind the step of hour
    `hour` (counted from the episode's reset): from hour n - 1 on it pushes window_count n-step transitions at ring.pos and advances
    ring.pushed; before that it only records history.  gamma: the one-step discount; gamma_n: what the updates bootstrap with."""

    def __init__(self, n, window_count, gamma, device=None):
        import torch
        self.n, self.window_count = check_n_step(n, "n"), int(window_count)
        if self.window_count < 1:
            raise ValueError(f"NStepWindow: window_count = {window_count!r} must be >= 1")
        self.gamma = float(np.float32(gamma))
        self.gamma_n = nstep_gamma(self.gamma, self.n)
        self.stage = ReplayRing(self.window_count, device=device)
        self.device = self.stage.device
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.hist_s, self.hist_a = z(self.n, self.window_count, _capi.NSTATE), z(self.n, self.window_count, _capi.NACTION)
        self.hist_r = z(self.n, self.window_count)
        self.window = (0, self.window_count, 0)     # shems_ring_window of the step that fills the staging ring
        self._L = _capi.declare_nstep()

    def struct(self):
        return _capi.NStepArgs(self.n, 0, self.window_count, self.gamma, 0, self.hist_s.data_ptr(), self.hist_a.data_ptr(), self.hist_r.data_ptr())

    def fold(self, ring, hour, stream=None):
        """Returns True when the fold pushed (hour >= n - 1)."""
        import torch
        if ring.capacity < self.window_count:
            raise ValueError(f"NStepWindow.fold: a ring of {ring.capacity} slots cannot take {self.window_count} transitions per step")
        if ring.s.device != self.device:
            raise ValueError(f"NStepWindow.fold: the ring lives on {ring.s.device}, the window on {self.device}")
        ns, ss, rs = self.struct(), self.stage.struct(), ring.struct()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
        _capi.check(self._L.shems_nstep_fold_dev(C.byref(ns), C.byref(ss), C.byref(rs), ring.pos, int(hour), st))
        pushed = int(hour) >= self.n - 1
        if pushed:
            ring.pushed += self.window_count
        return pushed


def nstep_from_episodes(src, episodes, steps, n, gamma, ring, stream=None):
    """shems_nstep_from_episodes_dev: `episodes` episodes of `steps` one-step transitions in src (episode e's hour t at slot e * steps + t)
    become episodes * (steps - n + 1) n-step pushes at ring.pos; ring.pushed advances by that many."""
    import torch
    n = check_n_step(n, "n")
    if int(steps) < n:
        raise ValueError(f"nstep_from_episodes: episodes of {steps} hours hold no window of n = {n} steps")
    L = _capi.declare_nstep()
    ss, rs = src.struct(), ring.struct()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    _capi.check(L.shems_nstep_from_episodes_dev(C.byref(ss), int(episodes), int(steps), n, float(np.float32(gamma)), C.byref(rs), ring.pos, st))
    ring.pushed += int(episodes) * (int(steps) - n + 1)
    return ring

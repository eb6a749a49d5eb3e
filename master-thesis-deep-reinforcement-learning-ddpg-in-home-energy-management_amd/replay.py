"""GPU-resident circular replay buffer (host-side bookkeeping; the data lives in HBM).

Reference: `memory = CircularBuffer{Any}(MEM_SIZE)` of `[s, a, r, s', done]` (input.jl:139-140),
`remember` (memory_plotting_saving.jl:46-47), `getData` (:31-42).  Here: struct-of-arrays device
tensors (PyTorch is only the allocator) + a host push counter; kernels receive the raw pointers
through `shems_replay` (include/shems_hip.h).
"""
from __future__ import annotations

import ctypes as C

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

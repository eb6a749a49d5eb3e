"""ctypes mirror of include/shems_hip.h -- the only way this package reaches the GPU.

The library is loaded from the package directory (built in-tree by `_build.py`).  If it is missing
or cannot be loaded the import FAILS: there is deliberately no NumPy/PyTorch fallback path.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SHEMS_HIP_LIB") or os.path.join(HERE, "libshems_hip.so")   # override: A/B builds of the library

OK, ERR_ARG, ERR_HIP, ERR_INDEX, ERR_NOMEM, ERR_NODEVICE, ERR_STATE = 0, -1, -2, -3, -4, -5, -6
NSTATE, NACTION, NCOL, NRESULT = 9, 2, 8, 23
TRACK_OFF, TRACK_DRL, TRACK_RULE = 0, 1, -1
ROLLOUT_RULE, ROLLOUT_RANDOM = 0, 1


class ShemsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[shems {code}] {msg}")
        self.code = code


class BoundsError(ShemsError, IndexError):
    """The reference raises Julia's BoundsError when next_state! reads row idx+1 > nrow (LU1:265-279)."""


class Config(C.Structure):
    _fields_ = [("cap_ev", C.c_float), ("soc_max", C.c_float), ("rate_max", C.c_double),
                ("disc_weight", C.c_double), ("disc_pot", C.c_double), ("penalty_weight", C.c_float),
                ("table_row0", C.c_int32), ("nrow", C.c_int32), ("reserved", C.c_int32)]


class View(C.Structure):
    _fields_ = [("n_envs", C.c_int64), ("maxsteps", C.c_int32), ("n_cfg", C.c_int32),
                ("obs", C.c_void_p), ("idx", C.c_void_p), ("step", C.c_void_p),
                ("cfg_of_env", C.c_void_p), ("cfgs", C.c_void_p), ("tables", C.c_void_p),
                ("total_rows", C.c_int64), ("err", C.c_void_p)]


class Replay(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("s", C.c_void_p), ("a", C.c_void_p), ("r", C.c_void_p),
                ("s2", C.c_void_p), ("done", C.c_void_p)]


assert C.sizeof(Config) == 48

_lib = None


def _declare(L):
    vp, i32, i64, u64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_uint32
    PV = C.POINTER(View)
    sigs = {
        "shems_abi_version": ([], C.c_int),
        "shems_last_error": ([], C.c_char_p),
        "shems_device_count": ([C.POINTER(C.c_int)], C.c_int),
        "shems_create": ([i64, i32, C.c_int, C.POINTER(vp)], C.c_int),
        "shems_destroy": ([vp], C.c_int),
        "shems_n_envs": ([vp, C.POINTER(i64)], C.c_int),
        "shems_set_tables": ([vp, vp, i64], C.c_int),
        "shems_set_configs": ([vp, C.POINTER(Config), i32, vp], C.c_int),
        "shems_reset": ([vp, C.c_int, vp, vp], C.c_int),
        "shems_reset_seeded": ([vp, u64, u32], C.c_int),
        "shems_step": ([vp, vp, C.c_int, vp, vp, vp], C.c_int),
        "shems_action": ([vp, vp, vp], C.c_int),
        "shems_rule_action": ([vp, vp], C.c_int),
        "shems_finished": ([vp, vp], C.c_int),
        "shems_get_state": ([vp, vp, vp, vp], C.c_int),
        "shems_set_state": ([vp, vp, vp, vp], C.c_int),
        "shems_get_view": ([vp, PV], C.c_int),
        "shems_set_stream": ([vp, vp], C.c_int),
        "shems_check_error": ([vp], C.c_int),
        "shems_step_dev": ([PV, vp, C.c_int, vp, vp, vp, vp, vp], C.c_int),
        "shems_action_dev": ([PV, vp, C.c_int, vp, vp], C.c_int),
        "shems_reset_dev": ([PV, C.c_int, vp, vp, vp], C.c_int),
        "shems_reset_seeded_dev": ([PV, u64, u32, vp], C.c_int),
        "shems_scale_action_dev": ([vp, i64, vp, vp], C.c_int),
        "shems_rollout_dev": ([PV, C.c_int, i32, u64, vp, C.POINTER(Replay), i64, i64, vp], C.c_int),
        "shems_track_dev": ([PV, vp, i64, C.c_int, i32, vp, i64, vp, vp], C.c_int),
        "shems_track": ([vp, vp, vp, vp, C.c_int, i32, vp, vp], C.c_int),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)          # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes = args
        fn.restype = res
    return sigs


class PerArgs(C.Structure):            # shems_per
    _fields_ = [("prio", C.c_void_p), ("pmax", C.c_void_p), ("ws", C.c_void_p),
                ("alpha", C.c_float), ("beta", C.c_float), ("eps_p", C.c_float), ("reserved", C.c_int32)]


PER_MAX_SLOTS = 262144                 # kPerMaxSlots: the sampler's one workgroup keeps every block sum in LDS
PER_COLS = 128
PW_T, PW_IDX, PW_W, PW_U, PW_TM, PW_S = 0, 4, 132, 260, 388, 516     # the workspace carve of csrc/shems_per_core.h (floats)


def _per_sigs():
    vp, i64, i32, u64, u32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint32, C.c_double
    PP, PR_ = C.POINTER(PerArgs), C.POINTER(Replay)
    return {                                    # (shems_ddpg * is passed as a void pointer: its mirror lives in ddpg.py)
        "shems_per_workspace_floats": [i64, C.POINTER(i64)],
        "shems_per_sample_dev": [PP, i64, i64, i64, i64, u64, u32, i32, vp],
        "shems_ddpg_update_given": [vp, PR_, i64, vp, vp, dbl, dbl, dbl, dbl, dbl, dbl, vp],
        "shems_ddpg_update_per": [vp, PR_, PP, i64, i64, i64, u64, u32, dbl, dbl, dbl, dbl, dbl, dbl, vp],
    }


def declare_per():
    """The prototypes of the prioritized-replay entry points (_per_sigs: compared with include/shems_hip.h by tests/test_per_host.py)."""
    L = lib()
    if getattr(L, "_per_declared", False):
        return L
    for name, args in _per_sigs().items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L._per_declared = True
    return L


TP_STORE_GRAD, TP_PER_GIVEN = 1, 2     # flags of the grouped throughput updates (SHEMS_TP_*)


def _group_per_sigs():
    """Prioritized replay for learner groups (shems_ddpg *, shems_group *, shems_group_w2t * and the record array go as void pointers:
    their mirrors live in ddpg.py / group.py)."""
    vp, i64, i32, u64, u32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint32, C.c_double
    PP, PR_ = C.POINTER(PerArgs), C.POINTER(Replay)
    return {
        "shems_ddpg_group_update_per_tp": [vp, PR_, vp, vp, vp, PP, i64, i64, i64, u64, u32, dbl, dbl, dbl, dbl, dbl, dbl, i32, vp],
        "shems_per_group_sample_dev": [PP, vp, vp, i64, i64, i64, i64, u64, u32, i32, vp],
    }


def declare_group_per():
    """The prototypes of _group_per_sigs (compared with include/shems_hip.h by tests/test_group_per_host.py)."""
    L = declare_per()
    if getattr(L, "_group_per_declared", False):
        return L
    for name, args in _group_per_sigs().items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L._group_per_declared = True
    return L


class NStepArgs(C.Structure):          # shems_nstep
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("window", C.c_int64), ("gamma", C.c_float), ("reserved2", C.c_int32),
                ("hist_s", C.c_void_p), ("hist_a", C.c_void_p), ("hist_r", C.c_void_p)]


NSTEP_MAX = 16                         # SHEMS_NSTEP_MAX


def _nstep_sigs():
    """Multi-step returns (shems_group * goes as a void pointer: its mirror lives in group.py)."""
    vp, i64, i32, f = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    PN, PR_ = C.POINTER(NStepArgs), C.POINTER(Replay)
    return {
        "shems_nstep_fold_dev": [PN, PR_, PR_, i64, i32, vp],
        "shems_nstep_group_fold_dev": [PN, PR_, PR_, vp, vp, i64, i32, vp],
        "shems_nstep_from_episodes_dev": [PR_, i64, i64, i32, f, PR_, i64, vp],
    }


def declare_nstep():
    """The prototypes of _nstep_sigs (compared with include/shems_hip.h by tests/test_nstep_host.py)."""
    L = lib()
    if getattr(L, "_nstep_declared", False):
        return L
    for name, args in _nstep_sigs().items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L._nstep_declared = True
    return L


PBT_FIELDS, PBT_MAX_RANGES, PBT_MAX_COUNT, PBT_CHUNK_VECS = 4, 8, 4096, 2048       # SHEMS_PBT_*


class PbtParams(C.Structure):          # shems_pbt_params
    _fields_ = [("seed", C.c_uint64), ("round", C.c_uint32), ("permille", C.c_int32), ("fields", C.c_uint32), ("reserved", C.c_int32),
                ("down", C.c_double), ("up", C.c_double), ("lo", C.c_double * PBT_FIELDS), ("hi", C.c_double * PBT_FIELDS)]


class PbtRange(C.Structure):           # shems_pbt_range
    _fields_ = [("offset_floats", C.c_int64), ("floats", C.c_int64)]


assert C.sizeof(PbtParams) == 104 and C.sizeof(PbtRange) == 16


def _pbt_sigs():
    """Population-based training (shems_group * and the record array go as void pointers: their mirrors live in group.py)."""
    vp, i32 = C.c_void_p, C.c_int32
    PP = C.POINTER(PbtParams)
    return {
        "shems_pbt_params_check": [PP],
        "shems_pbt_select_dev": [PP, i32, vp, vp, vp, vp, vp, vp],
        "shems_pbt_copy_dev": [vp, vp, C.POINTER(PbtRange), i32, vp, vp],
    }


def declare_pbt():
    """The prototypes of _pbt_sigs (compared with include/shems_hip.h by tests/test_pbt_host.py)."""
    L = lib()
    if getattr(L, "_pbt_declared", False):
        return L
    for name, args in _pbt_sigs().items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L._pbt_declared = True
    return L


class BcArgs(C.Structure):             # shems_bc
    _fields_ = [("alpha", C.c_float), ("weight", C.c_float), ("normalise", C.c_int32), ("reserved", C.c_int32), ("out", C.c_void_p)]


BC_OUT_FLOATS = 4 + 128                # SHEMS_BC_OUT_FLOATS: lambda, Qbar, -mean q, mse, q [128]
assert C.sizeof(BcArgs) == 24


def _bc_sigs():
    """The behaviour-regularised updates (shems_ddpg * and shems_td3 * go as void pointers: their mirrors live in ddpg.py / td3.py)."""
    vp, i64, u64, u32, dbl = C.c_void_p, C.c_int64, C.c_uint64, C.c_uint32, C.c_double
    PB, PR_ = C.POINTER(BcArgs), C.POINTER(Replay)
    return {
        "shems_ddpg_update_bc": [vp, PR_, i64, u64, u32, i64, i64, dbl, dbl, dbl, dbl, dbl, dbl, vp, PB, vp],
        "shems_td3_update_bc": [vp, PR_, i64, u64, u32, dbl, dbl, dbl, dbl, dbl, dbl, C.c_int, PB, vp],
    }


def declare_bc():
    """The prototypes of _bc_sigs (compared with include/shems_hip.h by tests/test_bc_host.py)."""
    L = lib()
    if getattr(L, "_bc_declared", False):
        return L
    for name, args in _bc_sigs().items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L._bc_declared = True
    return L


def exported_symbols():
    """Names include/shems_hip.h declares (used by the CPU-side ABI test)."""
    import re
    hdr = os.path.join(os.path.dirname(HERE), "include", "shems_hip.h")
    txt = open(hdr).read()
    return sorted(set(re.findall(r"\b(shems_[a-z0-9_]+)\s*\(", txt)))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64
        # (torch/lib, SONAME libamdhip64.so.7).  If /opt/rocm's copy is mapped first and torch's
        # second, the second HSA runtime finds no GPU.  Loading torch first makes our DT_NEEDED
        # libamdhip64.so.7 resolve to the copy torch already mapped, so tensors, streams and our
        # kernels share one runtime.  Without torch (e.g. a Julia host) /opt/rocm's runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        _declare(L)
        _lib = L
    return _lib


def check(rc):
    if rc == OK:
        return
    msg = lib().shems_last_error().decode("utf-8", "replace")
    if rc == ERR_INDEX:
        raise BoundsError(rc, msg)
    raise ShemsError(rc, msg)

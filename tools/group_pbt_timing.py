"""One round of population-based training at the protocol's size, by HIP events (not a benchmark, not a test: no bar is fixed):

  400 learners x 128 households on the tiled layout, 10 populations of 40 (one per charger), truncation 0.25 -> 100 children.

After a warm-up round: five rounds on fresh random scores, each timed as its two launches -- shems_pbt_select_dev, then
shems_pbt_copy_dev with the bytes it moved -- and, in the same process, the same (parent -> child) pairs and ranges as a torch copy
(slab[dst, a:b] = slab[src, a:b]).  Medians of five.

    python tools/group_pbt_timing.py [out.json] [--learners N] [--envs N]
    (default profiles/r23_pbt_timing.json; needs the GPU, does not read oracle/)
"""
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

PKG = "master-thesis-deep-reinforcement-learning-ddpg-in-home-energy-management_amd"
S = importlib.import_module(PKG)
G = importlib.import_module(PKG + ".group")
_capi = S._capi


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


flags = ("--learners", "--envs")
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "r23_pbt_timing.json")
L, ENVS, POPS, REPS = opt("--learners", 400), opt("--envs", 128), 10, 5

grp = G.LearnerGroup(L, ENVS, seed=1231, capacity=24000, tiled=True, hparams=[{} for _ in range(L)])
grp.slab.normal_()                                     # the copy does not care what it moves; no zeros, so nothing compresses or is skipped
pbt = G.PBT([l % POPS for l in range(L)], truncation=0.25, seed=7)
rng = np.random.default_rng(0)
grp.pbt_round(rng.normal(-450.0, 250.0, L), pbt, 0)    # warm-up: both kernels loaded, the group's buffers made
_, d_pop, d_parent, d_rank, ranges = grp._pbt_dev
LB = _capi.declare_pbt()
ptr = lambda x: C.c_void_p(x.data_ptr())
ev = lambda: torch.cuda.Event(enable_timing=True)
floats = sum(int(r.floats) for r in ranges)
rows = []
for rep in range(REPS):
    sc = torch.from_numpy(rng.normal(-450.0, 250.0, L)).to(grp.device)
    params, g = pbt.params(rep + 1, grp.rng_seed), grp.struct()
    e = [ev() for _ in range(5)]
    torch.cuda.synchronize()
    e[0].record()
    _capi.check(LB.shems_pbt_select_dev(C.byref(params), L, ptr(d_pop), ptr(sc), grp._hp_ptr(), ptr(d_parent), ptr(d_rank), grp._stream()))
    e[1].record()
    _capi.check(LB.shems_pbt_copy_dev(ptr(grp.slab), C.byref(g), ranges, len(ranges), ptr(d_parent), grp._stream()))
    e[2].record()
    torch.cuda.synchronize()
    parent = d_parent.cpu().numpy()
    dst = np.flatnonzero(parent != np.arange(L))
    t_dst, t_src = torch.as_tensor(dst, device=grp.device), torch.as_tensor(parent[dst], device=grp.device)
    e[3].record()
    for r in ranges:
        a, b = int(r.offset_floats), int(r.offset_floats + r.floats)
        grp.slab[t_dst, a:b] = grp.slab[t_src, a:b]
    e[4].record()
    torch.cuda.synchronize()
    moved = 4 * floats * len(dst)
    rows.append({"children": int(len(dst)), "select_us": 1e3 * e[0].elapsed_time(e[1]), "copy_us": 1e3 * e[1].elapsed_time(e[2]),
                 "torch_copy_us": 1e3 * e[3].elapsed_time(e[4]), "bytes_read": moved, "bytes_written": moved})
med = lambda k: float(np.median([r[k] for r in rows]))
moved = float(np.median([r["bytes_read"] for r in rows]))
props = torch.cuda.get_device_properties(0)
doc = {"what": "one round of population-based training: shems_pbt_select_dev + shems_pbt_copy_dev, and a torch copy of the same pairs and ranges",
       "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
       "shape": f"{L} learners x {ENVS} households, tiled; {POPS} populations, truncation 0.25; ranges {[(int(r.offset_floats), int(r.floats)) for r in ranges]}",
       "floats_per_child": floats, "method": f"HIP events around each launch after a warm-up round; medians of {REPS}",
       "median": {"select_us": med("select_us"), "copy_us": med("copy_us"), "torch_copy_us": med("torch_copy_us"), "children": med("children"),
                  "bytes_read": moved, "bytes_written": moved,
                  "copy_bytes_per_s": 2.0 * moved / (med("copy_us") * 1e-6), "torch_copy_bytes_per_s": 2.0 * moved / (med("torch_copy_us") * 1e-6)},
       "rounds": rows}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(doc, open(out_path, "w"), indent=1)
print(json.dumps(doc["median"]))
print("written", out_path)

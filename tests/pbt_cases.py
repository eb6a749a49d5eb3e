"""The cases of population-based training shared by the host and the GPU tests (tests/test_pbt_host.py, tests/test_pbt_gpu.py): what
shems_pbt_select_dev and shems_pbt_copy_dev are held to, against tests/pbt_ref.py."""
import numpy as np

import pbt_ref as PR

f32, f64 = np.float32, np.float64
COUNTS = (1, 7, 8, 65)
MASKS = (0, 1, 2, 4, 8, 15)
TIGHT_LO = tuple(float(f32(x)) for x in (3e-4, 1.5e-3, 0.002, 0.08))       # bounds inside the records' spread: they clamp at both ends
TIGHT_HI = tuple(float(f32(x)) for x in (4e-4, 2e-3, 0.004, 0.12))
CHUNK_VECS = 2048                                                           # SHEMS_PBT_CHUNK_VECS


def pops(count):
    """(name, pop, permille): one population; two interleaved ones of unequal size; a population of one beside the rest; populations of
    three, whose quota at permille 250 is 0, beside one that has a quota."""
    l = np.arange(count)
    yield "one", np.zeros(count, np.int32), 250
    yield "two", np.where(l % 3 == 0, 9, 4).astype(np.int32), 500
    yield "single", np.where(l == count // 2, 5, 0).astype(np.int32), 400
    yield "q0p3", np.where(l < 3, 2, np.where(l < 6, 3, 1)).astype(np.int32), 250


def score_patterns(count, pop, seed):
    rng = np.random.default_rng(seed)
    base = -450.0 + 250.0 * rng.standard_normal(count)
    yield "distinct", base.copy()
    yield "ties", np.round(base / 200.0) * 200.0                            # a handful of distinct values: exact ties everywhere
    s = base.copy()                                                         # a NaN and a -inf: the worst of their population, so children
    s[rng.permutation(count)[:2]] = (np.nan, -np.inf)[:min(2, count)]
    yield "nonfinite-children", s
    s = np.full(count, np.nan)                                              # too few finite scores: non-finite learners rank as parents
    s[::5] = base[::5]
    s[1::7] = np.inf
    yield "nonfinite-parents", s


def select_cases():
    """(name, case): case = dict(params, pop, score, hp)."""
    i = 0
    for count in COUNTS:
        for pname, pop, permille in pops(count):
            for sname, score in score_patterns(count, pop, 100 + i):
                tight = i % 3 == 1
                p = PR.params(seed=0x1234567800000000 + 7919 * i, round=i % 5, permille=permille, fields=MASKS[i % len(MASKS)] if i % 4 else 15,
                              down=0.8, up=1.2, lo=TIGHT_LO if tight else PR.DEFAULT_LO, hi=TIGHT_HI if tight else PR.DEFAULT_HI)
                yield f"c{count}-{pname}-{sname}", dict(params=p, pop=pop, score=np.asarray(score, f64), hp=PR.records(count))
                i += 1


def sentinel_slab(count, stride):
    """Every float a distinct bit pattern: learner l's float k holds the bits of the integer l * 2^20 + k + 1 (compared as bytes)."""
    return (np.arange(count, dtype=np.int64)[:, None] * (1 << 20) + np.arange(stride, dtype=np.int64)[None, :] + 1).astype(np.int32).view(f32)


def copy_cases():
    """(name, case): case = dict(count, stride, ranges, parent).  The fake slab of the issue; then single ranges of one vector more and one
    less than a workgroup's chunk (and exactly a chunk), so a full chunk, a one-vector tail and an almost-full tail all run."""
    yield "fake-slab", dict(count=7, stride=1040, ranges=[(0, 516), (520, 12)], parent=np.array([0, 0, 2, 0, 4, 5, 5], np.int32))
    stride = 4 * (CHUNK_VECS + 2)
    for name, vecs, off in (("chunk+1", CHUNK_VECS + 1, 0), ("chunk-1", CHUNK_VECS - 1, 4), ("chunk", CHUNK_VECS, 8)):
        yield name, dict(count=3, stride=stride, ranges=[(off, 4 * vecs)], parent=np.array([2, 1, 2], np.int32))
    yield "multi-chunk", dict(count=4, stride=4 * (3 * CHUNK_VECS + 40), ranges=[(0, 4 * (2 * CHUNK_VECS + 3)), (4 * (2 * CHUNK_VECS + 8), 0),
                                                                                (4 * (2 * CHUNK_VECS + 8), 4 * (CHUNK_VECS + 5))],
                              parent=np.array([3, 3, 2, 3], np.int32))


def bad_copy_args():
    """(ranges, n_ranges or None, word of the message) on the fake slab: misaligned, past the stride, nine ranges."""
    return (([(0, 514)], None, "multiples of 4"), ([(2, 512)], None, "multiples of 4"), ([(528, 516)], None, "runs past stride_bytes"),
            ([(1044, 0)], None, "runs past stride_bytes"), ([(0, 4)] * 9, 9, "n_ranges = 9"), ([(0, 4)], 0, "n_ranges = 0"),
            ([(0, 0), (16, 0)], None, "every range is empty"), ([(-4, 8)], None, "negative"))

"""ADAM + soft target update on arbitrary state: the float64 definition, its plain fp32 twin, and the step metric.

reference(): oracle/ddpg_oracle.py's Adam and soft_update (Flux 0.12.1: Float64 scalars over Float32 arrays, each array statement rounded
to Float32; the soft update in Float32) started from given moments and beta powers -- no second copy of the formulas.
twin(): the same statements with EVERY operation rounded to fp32, in the order csrc/shems_adam.h performs them; it exists to measure
what plain fp32 costs against the definition, which is where the bounds of tests/test_adam_edges_gpu.py come from (4 x its worst).
errors(): the two conditions every element is held to.
  (a) the new value within N ulp of the reference's, the ulp taken at the larger of |old| and |reference new| (the resolution the
      operands of `old +/- step` were held at; with m and g cancelling that is the old moment's, not the tiny result's);
  (b) where the reference's step d = new - old (float64 differences of the fp32 values) exceeds `thresh` ulp of the old value, the
      kernel's step within a relative bound R of it.
An absolute allowance (one fp32 smallest normal for m and v) is taken off both differences first."""
from __future__ import annotations

import numpy as np

import util as U  # noqa: F401  (puts oracle/ on sys.path)
import ddpg_oracle as DO  # noqa: E402

f32, f64 = np.float32, np.float64
F32_MIN_NORMAL = float(np.finfo(f32).tiny)             # 1.17549435e-38
RESOLVED = 2.0 ** 20                                   # (b) again on the elements whose step is at least 2^20 ulp of the old value


def reference(p, m, v, t, g, eta, tau, bp1, bp2):
    """(p, m, v, target) after one update from fp32 arrays and Float64 scalars, by DO.Adam.step and DO.soft_update.  eta and tau may be
    arrays, one value per element (the learners of a group side by side, each with its own record)."""
    opt = DO.Adam(len(p), 0.0)
    eta = np.asarray(eta, f64)
    assert (eta.astype(f32).astype(f64) == eta).all(), "eta must be a Float32 value (the learners hold Float32(eta) as a double)"
    opt.eta = eta if eta.ndim else float(eta)
    opt.m, opt.v, opt.bp = np.array(m, f32), np.array(v, f32), [float(bp1), float(bp2)]
    p1 = opt.step(np.asarray(p, f32), np.asarray(g, f32))
    return p1, opt.m, opt.v, DO.soft_update(np.asarray(t, f32), p1, np.asarray(tau, f32))


def reference_delta(m, v, g, eta, bp1, bp2):
    """The reference's step itself (Float32(delta)): what it takes off a parameter of exactly 0."""
    z = np.zeros(len(g), f32)
    return -reference(z, m, v, z, g, eta, 0.0, bp1, bp2)[0]


def twin(p, m, v, t, g, eta, tau, bp1, bp2, moments="f64"):
    """Every operation in fp32 (NumPy float32 arithmetic does not fuse), in the kernel's order: m1, g^2, v1, s = sqrt(v1 * ic2) + eps,
    y = 1 / s, delta = (m1 * k1) * y, p - delta, (1 - tau) t + tau p.

    moments="fp32" is that, to the letter.  It is no yardstick for the step: b1 m + (1 - b1) g cancels wherever m and g have opposite
    signs, and a plain fp32 m1 is then wrong by up to 10 x (the "cancel" classes) or by 1e-3 (an ordinary g = 1e-3 against m = -1.1e-4),
    which delta inherits; the figures are kept in profiles/adam_edges_errors.txt.  moments="f64", the twin the bounds are taken from,
    restates the two moment statements the way the definition and the kernel have them -- Float64 scalars, ONE rounding to fp32 -- and
    keeps everything that forms delta from them (fp32 factors k1 and ic2, fp32 sqrt, reciprocal and products) in fp32."""
    p, m, v, t, g = (np.asarray(x, f32) for x in (p, m, v, t, g))
    b1, c1, b2, c2, eps = f32(0.9), f32(1.0 - 0.9), f32(0.999), f32(1.0 - 0.999), f32(1e-8)
    k1, ic2, tau = f32(float(eta) / (1.0 - bp1)), f32(1.0 / (1.0 - bp2)), f32(tau)
    with np.errstate(under="ignore"):
        if moments == "fp32":
            m1 = b1 * m + c1 * g
            v1 = b2 * v + c2 * (g * g)
        else:
            m1 = (0.9 * m.astype(f64) + (1.0 - 0.9) * g.astype(f64)).astype(f32)
            v1 = (0.999 * v.astype(f64) + (1.0 - 0.999) * (g * g).astype(f64)).astype(f32)
        y = f32(1) / (np.sqrt(v1 * ic2) + eps)
        pn = p - (m1 * k1) * y
        tn = (f32(1) - tau) * t + tau * pn
    assert all(x.dtype == f32 for x in (m1, v1, pn, tn))
    return pn, m1, v1, tn


def _spacing(x):
    return np.spacing(np.abs(np.asarray(x, f32))).astype(f64)


def errors(old, new, ref, absolute=0.0, thresh=64.0):
    """-> dict(ulp = worst of (a), rel = worst of (b), n_rel = elements (b) looked at) for one array."""
    old, new, ref = (np.asarray(x, f32) for x in (old, new, ref))
    assert np.isfinite(new).all() and np.isfinite(ref).all(), "a non-finite value: the cases hold none, the kernel must produce none"
    o, k, r = old.astype(f64), new.astype(f64), ref.astype(f64)
    diff = np.maximum(np.abs(k - r) - absolute, 0.0)
    ulp = diff / _spacing(np.maximum(np.abs(old), np.abs(ref)))
    d_ref = r - o
    sel = np.abs(d_ref) > thresh * _spacing(old)
    rel = diff[sel] / np.abs(d_ref[sel])
    return dict(ulp=float(ulp.max()), rel=float(rel.max()) if sel.any() else 0.0, n_rel=int(sel.sum()))


NAMES = ("p", "m", "v", "target")
ABSOLUTE = dict(p=0.0, m=F32_MIN_NORMAL, v=F32_MIN_NORMAL, target=0.0)


def all_errors(old, new, ref):
    """old / new / ref: 4-tuples (p, m, v, target).  -> {name: dict(ulp, rel, n_rel, rel_resolved, n_resolved)}; the target's step is
    measured from the old target."""
    out = {}
    for name, o, k, r in zip(NAMES, old, new, ref):
        e = errors(o, k, r, ABSOLUTE[name])
        fine = errors(o, k, r, ABSOLUTE[name], thresh=RESOLVED)
        e["rel_resolved"], e["n_resolved"] = fine["rel"], fine["n_rel"]
        out[name] = e
    return out


def worst(acc, errs):
    """Fold all_errors() results into acc (per name, the maxima)."""
    for name, e in errs.items():
        a = acc.setdefault(name, dict(ulp=0.0, rel=0.0, rel_resolved=0.0, n_rel=0, n_resolved=0))
        for k in ("ulp", "rel", "rel_resolved"):
            a[k] = max(a[k], e[k])
        a["n_rel"] += e["n_rel"]
        a["n_resolved"] += e["n_resolved"]
    return acc


# The bounds: 4 x the worst value of twin() against reference() over every case of tests/adam_cases.py:apply_cases, both networks
# (tests/test_adam_horizon_host.py:test_the_bounds_are_four_times_the_fp32_twin measures them again on every run and holds these figures
# to 4 x .. 4.2 x what it finds).  m and v: the twin's moment statements ARE the definition's, so its error is 0 and the kernels are held
# to the reference's bits, the one-smallest-normal allowance aside.
#                 (a) ulp    (b) relative step       (b) on steps >= 2^20 ulp of the old value
BOUNDS = dict(p=dict(ulp=24.0, rel=1.24e-2, rel_resolved=7.63e-6),
              m=dict(ulp=0.0, rel=0.0, rel_resolved=0.0),
              v=dict(ulp=0.0, rel=0.0, rel_resolved=0.0),
              target=dict(ulp=64.0, rel=1.75e-2, rel_resolved=4.31e-5))


def assert_within_bounds(errs, what, names=NAMES):
    bad = {(n, k): (errs[n][k], BOUNDS[n][k]) for n in names for k in ("ulp", "rel", "rel_resolved") if not errs[n][k] <= BOUNDS[n][k]}
    assert not bad, (what, bad)

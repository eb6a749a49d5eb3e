"""Host-side tests of per-learner hyper-parameters in learner groups: the record's layout, shems_group_hparams_check, the tuned-grid
helper and LearnerGroup's argument errors (all raised before any device work)."""
import ctypes as C
import importlib

import pytest

import util as U


def _g():
    U.pkg()
    return importlib.import_module(U.PKG_NAME + ".group")


def test_record_layout_matches_the_header():
    G = _g()
    H = G.HParams
    assert C.sizeof(H) == 40
    assert [(n, getattr(H, n).offset) for n, _ in H._fields_] == [("eta_act", 0), ("eta_crit", 8), ("gamma", 16), ("tau", 20), ("noise_mu", 24),
                                                                   ("noise_sigma", 28), ("batch", 32), ("reserved", 36)]


def _check(recs):
    G = _g()
    L = G._declare_group()
    arr = (G.HParams * len(recs))(*recs)
    rc = L.shems_group_hparams_check(arr, len(recs))
    return rc, (L.shems_last_error().decode() if rc else "")


def test_check_accepts_the_36_runnable_tuned_points():
    G = _g()
    full, arr = G._hparams_records(36, G.tuned_grid(G.TUNED_RUNNABLE)[0], 0.1, 24000)
    assert len(full) == 36
    assert _check(list(arr)) == (0, "")


@pytest.mark.parametrize("field,value,word", [("batch", 0, "batch"), ("batch", 129, "batch"), ("batch", 150, "batch"), ("eta_act", 0.0, "eta_act"),
                                              ("eta_crit", -1e-3, "eta_crit"), ("tau", 0.0, "tau"), ("tau", 1.5, "tau"), ("tau", float("nan"), "tau"),
                                              ("gamma", 1.01, "gamma"), ("noise_sigma", -0.1, "noise_sigma"), ("eta_act", float("inf"), "eta_act")])
def test_check_rejects_a_bad_field_naming_the_learner(field, value, word):
    G = _g()
    good = dict(eta_act=1e-4, eta_crit=1e-3, gamma=0.99, tau=1e-3, noise_mu=0.0, noise_sigma=0.1, batch=120, reserved=0)
    recs = [G.HParams(**good) for _ in range(4)]
    setattr(recs[2], field, value)
    rc, msg = _check(recs)
    assert rc == -1 and "learner 2" in msg and word in msg, msg


def test_tuned_grid_records_and_skipped_points():
    G = _g()
    recs, points, skipped = G.tuned_grid(["1105", "1141", "1100", "1109", "1154", "1180"], seeds=2, chargers=3)
    # 05 = 0012: BATCH 120, sigma 0.1, (200, 400), (eta_act, eta_crit) = (1e-4, 1e-3); 41 = 1112: BATCH 100, sigma 0.2, (200, 400), (1e-4, 1e-3)
    assert points == ["1105", "1141"]
    assert len(recs) == 2 * 2 * 3
    r0, r1 = recs[0], recs[6]
    assert (r0["batch"], r0["sigma"], r0["hidden"]) == (120, 0.1, (200, 400))
    assert r0["eta_act"] == float(C.c_float(1e-4).value) and r0["eta_crit"] == float(C.c_float(1e-3).value)
    assert (r1["batch"], r1["sigma"], r1["hidden"]) == (100, 0.2, (200, 400))
    assert all(r == r0 for r in recs[:6]) and all(r == r1 for r in recs[6:])
    reasons = dict(skipped)
    assert "(300, 600)" in reasons["1100"] and "150" not in reasons["1100"]           # 00 = 0000: (300, 600)
    assert "(300, 600)" in reasons["1109"]                                            # 09 = 0100: sigma 0.2, (300, 600)
    assert "BATCH_SIZE 150" in reasons["1154"] and "(300, 600)" in reasons["1154"]   # 54 = 2000
    assert "BATCH_SIZE 150" in reasons["1180"] and "(300, 600)" not in reasons["1180"]   # 80 = 2222
    # the whole grid: 36 of 81 points fit, 45 are skipped
    recs, points, skipped = G.tuned_grid(range(81))
    assert len(points) == 36 and len(skipped) == 45 and tuple(p.zfill(2) for p in points) == G.TUNED_RUNNABLE


@pytest.mark.parametrize("kw,word", [(dict(hparams=[{}] * 3), "4 learners"), (dict(hparams=[{"batch": 150}] * 4), "batch 150"),
                                     (dict(hparams=[{}, {}, {"hidden": (300, 600)}, {}]), r"hparams\[2\]: hidden"),
                                     (dict(hparams=[{}, {"noise_type": "ou"}, {}, {}]), "noise_type"),
                                     (dict(hparams=[{}, {}, {}, {"mem_size": 30000}]), "mem_size"),
                                     (dict(hparams=[{}, {"gamma": 1.5}, {}, {}]), "learner 1"),
                                     (dict(hparams=[{}, {}, {"sigmas": 0.1}, {}]), "unknown keys"),
                                     (dict(hparams=[{}] * 4, form="latency"), "latency")])
def test_learner_group_refuses_before_any_device_work(kw, word, monkeypatch):
    G = _g()
    import torch
    monkeypatch.setattr(torch.cuda, "current_device", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    with pytest.raises(ValueError, match=word):
        G.LearnerGroup(4, 64, **kw)

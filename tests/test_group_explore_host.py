"""Host-side tests of per-learner exploration and ring sizes in learner groups: the shems_group_xparams record, its check, the
refusals LearnerGroup raises before any device work, and the input template's grid (RL-SHEMS/input.jl:58-100) as records."""
import ctypes as C
import importlib

import pytest

import util as U


def _g():
    U.pkg()
    return importlib.import_module(U.PKG_NAME + ".group")


def test_record_layout_matches_the_header():
    G = _g()
    X = G.XParams
    assert C.sizeof(X) == 16
    assert [(n, getattr(X, n).offset) for n, _ in X._fields_] == [("ou_theta", 0), ("ou_dt", 4), ("mem_size", 8), ("reserved", 12)]
    assert C.sizeof(G.HParams) == 40 and G.HParams.reserved.offset == 36          # the first record is what it was


def _check(recs, capacity=24000):
    G = _g()
    L = G._declare_group()
    arr = (G.XParams * len(recs))(*recs)
    rc = L.shems_group_xparams_check(arr, len(recs), capacity)
    return rc, (L.shems_last_error().decode() if rc else "")


def test_check_accepts_a_good_array():
    G = _g()
    recs = [G.XParams(0.15, 1e-2, 24000, 0), G.XParams(0.0, 1e-2, 1, 0), G.XParams(0.2, 0.5, 20000, 0), G.XParams(0.15, 1e-2, 96, 0)]
    assert _check(recs) == (0, "")


@pytest.mark.parametrize("field,value,word", [("ou_theta", -0.1, "ou_theta"), ("ou_theta", float("nan"), "ou_theta"), ("ou_dt", 0.0, "ou_dt"),
                                              ("mem_size", 0, "mem_size"), ("mem_size", 24001, "mem_size")])
def test_check_rejects_a_bad_field_naming_the_learner(field, value, word):
    G = _g()
    recs = [G.XParams(0.15, 1e-2, 24000, 0) for _ in range(4)]
    setattr(recs[2], field, value)
    rc, msg = _check(recs)
    assert rc == -1 and "learner 2" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(noise_type="ou", hparams=[{}, {}, {"noise_type": "gn"}, {}]), r"hparams\[2\]: noise_type 'gn'"),
    (dict(form="wide", noise_type="ou", hparams=[{"noise_type": "gn"}, {}, {}, {}]), r"hparams\[0\]: noise_type 'gn'"),
    (dict(hparams=[{}, {}, {}, {"theta": 0.2}]), r"hparams\[3\]: theta"),
    (dict(form="wide", hparams=[{}, {"theta": 0.2}, {}, {}]), r"hparams\[1\]: theta"),
    (dict(form="wide", capacity=720, noise_type="ou", hparams=[{}, {"mem_size": 30000}, {}, {}]), r"hparams\[1\]: mem_size"),
    (dict(noise_type="en"), "noise_type 'en'"), (dict(noise_type="pn"), "noise_type 'pn'"), (dict(noise_type="xx"), "noise_type 'xx'"),
    (dict(form="wide", noise_type="en"), "noise_type 'en'"),
    (dict(noise_type="ou", hparams=[{}, {}, {"theta": -0.1}, {}]), "learner 2: ou_theta"),
    (dict(noise_type="ou", dt=0.0), "learner 0: ou_dt"),
    (dict(form="latency", noise_type="ou"), "latency"),
])
def test_learner_group_refuses_before_any_device_work(kw, word, monkeypatch):
    G = _g()
    import torch
    monkeypatch.setattr(torch.cuda, "current_device", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    with pytest.raises(ValueError, match=word):
        G.LearnerGroup(4, 64, **kw)


# Regression pins, not new behaviour: these refusals existed before per-learner exploration and keep their wording beside it.
@pytest.mark.parametrize("kw,word", [
    (dict(hparams=[{}, {"noise_type": "ou"}, {}, {}]), r"hparams\[1\]: noise_type 'ou'"),
    (dict(capacity=720, hparams=[{}, {}, {"mem_size": 721}, {}]), r"hparams\[2\]: mem_size"),
    (dict(capacity=720, hparams=[{"mem_size": 0}, {}, {}, {}]), r"hparams\[0\]: mem_size"),
    (dict(form="latency", capacity=720, hparams=[{}, {"mem_size": 96}, {}, {}]), "latency"),
])
def test_refusals_that_existed_keep_their_wording(kw, word, monkeypatch):
    G = _g()
    import torch
    monkeypatch.setattr(torch.cuda, "current_device", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    with pytest.raises(ValueError, match=word):
        G.LearnerGroup(4, 64, **kw)


def test_records_carry_theta_mem_size_and_the_groups_noise():
    G = _g()
    recs = [{}, {"theta": 0.2, "mem_size": 96}, {"sigma": 0.3}, {"mem_size": 720}]
    full, arr = G._hparams_records(4, recs, 0.1, 720, noise_type="ou", theta=0.15)
    assert [r["mem_size"] for r in full] == [720, 96, 720, 720] and all(r["noise_type"] == "ou" for r in full)
    assert full[1]["theta"] == float(C.c_float(0.2).value) and full[0]["theta"] == float(C.c_float(0.15).value)
    xp = G._xparams_records(full, 720, 1e-2)
    assert [x.mem_size for x in xp] == [720, 96, 720, 720] and xp[1].ou_theta == C.c_float(0.2).value and xp[3].ou_dt == C.c_float(1e-2).value
    assert all(x.reserved == 0 for x in xp) and all(h.reserved == 0 for h in arr)


def test_input_grid_decodes_the_27_points():
    G = _g()
    recs, points = G.input_grid(range(27))
    assert len(recs) == 27 and points == [str(c) for c in range(27)] and len(G.INPUT_ALL) == 27 and G.INPUT_CAPACITY == 30000
    key = lambda r: (r["mem_size"], r["batch"], r["hidden"], r["gamma"], r["sigma"], r["theta"])
    f = lambda x: float(C.c_float(x).value)
    assert key(recs[0]) == (30000, 200, (150, 300), f(0.99), 0.1, 0.15)
    assert key(recs[14]) == (20000, 50, (300, 600), f(0.99), 0.2, 0.2)
    assert key(recs[26]) == (24000, 120, (300, 600), f(0.99), 0.2, 0.2)
    assert {r["mem_size"] for r in recs} == {30000, 20000, 24000} and {r["batch"] for r in recs} == {200, 50, 120}
    assert {(r["hidden"], r["gamma"], r["sigma"], r["theta"]) for r in recs} == {((150, 300), f(0.99), 0.1, 0.15), ((300, 600), f(0.999), 0.1, 0.15),
                                                                                ((300, 600), f(0.99), 0.2, 0.2)}
    for r in recs:
        assert r["noise_type"] == "ou" and r["mu"] == 0.0 and r["tau"] == f(1e-3) and (r["eta_act"], r["eta_crit"]) == (f(1e-4), f(1e-3))
        assert set(r) <= set(G.HPARAM_KEYS)
    recs4, points4 = G.input_grid(G.INPUT_ALL, seeds=2, chargers=2)
    assert len(recs4) == 108 and recs4[4 * 14 + 3] == recs[14] and points4 == list(G.INPUT_ALL)
    # the records pass the checks of a wide "ou" group carved for the grid's largest ring
    full, arr = G._hparams_records(108, recs4, 0.1, G.INPUT_CAPACITY, width=(300, 600), noise_type="ou")
    assert len(G._xparams_records(full, G.INPUT_CAPACITY, 1e-2)) == 108
    for bad in (27, "27", "1127", 81, "x"):
        with pytest.raises(ValueError, match="27 points"):
            G.input_grid([bad])
    assert G.input_grid(["1114"])[0][0] == recs[14]                           # a JOB_ID: its last two digits

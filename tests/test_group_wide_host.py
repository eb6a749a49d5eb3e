"""Host-side tests of the wide learner-group form (LearnerGroup(form="wide")): shems_group_hparams_check_wide, the pass-width workspace,
tuned_grid(wide=True), the pad / unpad helpers between two hidden sizes and the argument errors (all raised before any device work)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import util as U


def _g():
    U.pkg()
    return importlib.import_module(U.PKG_NAME + ".group")


def _d():
    U.pkg()
    return importlib.import_module(U.PKG_NAME + ".ddpg")


GOOD = dict(eta_act=1e-4, eta_crit=1e-3, gamma=0.99, tau=1e-3, noise_mu=0.0, noise_sigma=0.1, batch=120, reserved=0)


def _check(batches, wide_max=None):
    G = _g()
    L = G._declare_group()
    recs = [G.HParams(**dict(GOOD, batch=b)) for b in batches]
    arr = (G.HParams * len(recs))(*recs)
    rc = L.shems_group_hparams_check(arr, len(recs)) if wide_max is None else L.shems_group_hparams_check_wide(arr, len(recs), wide_max)
    return rc, (L.shems_last_error().decode() if rc else "")


def test_wide_check_takes_batch_1_to_256():
    assert _check([1, 256, 150, 120], 256) == (0, "")


@pytest.mark.parametrize("bad", [0, 257])
def test_wide_check_refuses_batch_outside_1_to_256_naming_the_learner(bad):
    rc, msg = _check([120, 150, bad, 1], 256)
    assert rc == -1 and "learner 2" in msg and "batch" in msg, msg


def test_wide_check_limit_is_max_batch_and_at_most_256():
    rc, msg = _check([120, 150], 128)
    assert rc == -1 and "learner 1" in msg and "batch 150" in msg, msg
    rc, msg = _check([120], 257)
    assert rc == -1 and "max_batch" in msg, msg


def test_existing_check_still_refuses_129():
    rc, msg = _check([120, 129])
    assert rc == -1 and "learner 1" in msg and "batch 129" in msg, msg


def _ws(l1, l2, b=None):
    G = _g()
    L = G._declare_group()
    out = C.c_int64(0)
    rc = L.shems_wide_workspace_floats(l1, l2, C.byref(out)) if b is None else L.shems_wide_group_workspace_floats(l1, l2, b, C.byref(out))
    return rc, out.value


def test_group_workspace_is_the_single_learner_one_up_to_batch_128():
    base = _ws(300, 600)
    assert base[0] == 0 and base[1] > 0
    for b in (1, 50, 120, 128):
        assert _ws(300, 600, b) == base


def test_group_workspace_grows_with_the_pass_width():
    base = _ws(300, 600)[1]
    rc150, w150 = _ws(300, 600, 150)            # P = 160
    rc256, w256 = _ws(300, 600, 256)
    rc160, w160 = _ws(300, 600, 160)
    assert rc150 == rc256 == rc160 == 0
    assert base < w150 == w160 < w256
    # every row-proportional part scales with P: the workspace is linear in the pass width
    assert abs(w150 / base - 160 / 128) < 1e-3 and abs(w256 / base - 2.0) < 1e-3


def test_group_workspace_refuses_257():
    assert _ws(300, 600, 257)[0] == -1
    assert _ws(300, 600, 0)[0] == -1


def test_tuned_grid_wide_holds_all_81_points():
    G = _g()
    recs, points, skipped = G.tuned_grid(range(81), wide=True)
    assert len(points) == 81 and skipped == [] and len(recs) == 81
    assert tuple(p.zfill(2) for p in points) == G.TUNED_ALL
    r = recs[54]                                 # 54 = 2000: BATCH 150, (300, 600)
    assert points[54] == "54" and r["batch"] == 150 and r["hidden"] == (300, 600)
    assert max(x["batch"] for x in recs) == 150 and {x["hidden"] for x in recs} == {(300, 600), (250, 500), (200, 400)}
    recs4, points4, _ = G.tuned_grid(G.TUNED_ALL, seeds=4, wide=True)
    assert len(recs4) == 324 and points4 == list(G.TUNED_ALL)
    # the records pass the wide check of a (300, 600) group
    full, arr = G._hparams_records(len(recs4), recs4, 0.1, 24000, width=(300, 600))
    assert len(full) == 324


def test_tuned_grid_default_unchanged():
    G = _g()
    recs, points, skipped = G.tuned_grid(range(81))
    assert len(points) == 36 and len(skipped) == 45


@pytest.mark.parametrize("hid", [(150, 300), (200, 400), (250, 500)])
def test_pad_to_and_unpad_from_round_trip(hid):
    D = _d()
    rng = np.random.default_rng(7)
    for in_dim, out_dim in ((9, 2), (11, 1)):
        p = rng.standard_normal(D.net_size(in_dim, out_dim, hid)).astype(np.float32)
        q = D.pad_net_to(p, in_dim, out_dim, hid, (300, 600))
        assert q.size == D.net_size(in_dim, out_dim, (300, 600))
        assert np.count_nonzero(q) == np.count_nonzero(p)
        assert (D.unpad_net_from(q, in_dim, out_dim, hid, (300, 600)) == p).all()
        # the padded network computes the same function
        x = rng.standard_normal((5, in_dim)).astype(np.float32)

        def fwd(flat, h):
            W1, b1, W2, b2, W3, b3 = D._blocks(flat, in_dim, out_dim, h)
            return np.maximum(np.maximum(x @ W1 + b1, 0) @ W2 + b2, 0) @ W3 + b3
        assert np.allclose(fwd(p, hid), fwd(q, (300, 600)), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        D.pad_net_to(np.zeros(D.net_size(9, 2, (300, 600)), np.float32), 9, 2, (300, 600), (250, 500))
    with pytest.raises(NotImplementedError):     # pad_net keeps refusing what does not fit (250, 500)
        D.pad_net(np.zeros(D.net_size(9, 2, (300, 600)), np.float32), 9, 2, (300, 600))


@pytest.mark.parametrize("kw,word", [(dict(form="wide", tiled=True), "tiled"),
                                     (dict(form="wide", hidden=(250, 500), hparams=[{}, {"hidden": (300, 600)}, {}, {}]), r"hparams\[1\]: hidden"),
                                     (dict(form="wide", hparams=[{}, {}, {"batch": 257}, {}]), r"hparams\[2\]: batch 257"),
                                     (dict(form="wide", hparams=[{}, {"noise_type": "ou"}, {}, {}]), r"hparams\[1\]: noise_type"),
                                     (dict(form="wide", hparams=[{}, {}, {}, {"mem_size": 30000}]), r"hparams\[3\]: mem_size"),
                                     (dict(hparams=[{}, {}, {"hidden": (300, 600)}, {}]), r"hparams\[2\]: hidden"),
                                     (dict(hparams=[{"batch": 150}] * 4), "batch 150"),
                                     (dict(hidden=(300, 600)), "wide")])
def test_wide_group_refuses_before_any_device_work(kw, word, monkeypatch):
    G = _g()
    import torch
    monkeypatch.setattr(torch.cuda, "current_device", lambda: (_ for _ in ()).throw(AssertionError("device work")))
    with pytest.raises(ValueError, match=word):
        G.LearnerGroup(4, 64, **kw)


def test_wide_group_width_defaults():
    G = _g()
    assert G._wide_width(None, None) == (300, 600)
    assert G._wide_width([{"hidden": (200, 400)}, {"hidden": (150, 300)}], None) == (200, 400)
    assert G._wide_width([{"hidden": (300, 600)}, {}], None) == (300, 600)
    assert G._wide_width([{}], None) == (250, 500)
    assert G._wide_width(None, (250, 500)) == (250, 500)

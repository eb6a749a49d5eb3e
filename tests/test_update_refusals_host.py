"""What the single learner's update forms refuse, row by row, without a device and without the library: bare Agent / TD3Agent objects
(no __init__), bare rings, and a sentinel where the first device-facing call of every form stands (_ddpg_args, _td3_args, the lazy
prototype declarations).  One table holds every message in full.  Per form: one row per (fact, message); one row per adjacent pair of
facts in the form's order, both set, the earlier message asserted; one row per accepted case, where the sentinel must be reached.  The
rows describe the behaviour of the commit before the refusal table (ddpg.REFUSALS) existed, and hold on it unchanged."""
import ctypes as C
import importlib
import types

import pytest

import util as U


class Reached(Exception):
    """The call passed its refusals and arrived at its device-facing half."""


def _reached(*a, **k):
    raise Reached


def _mods():
    return tuple(importlib.import_module(U.PKG_NAME + m) for m in (".ddpg", ".td3", ".replay", "._capi"))


class _Sync:
    native = None

    def __init__(self, world=1):
        self.world = world


class _Ring:
    """A ring nobody reads: struct() hands out nothing, the length is the capacity."""
    capacity = 1000
    s = types.SimpleNamespace(device=None)

    def struct(self):
        return C.c_int64(0)

    def __len__(self):
        return self.capacity


def _per_ring(R):
    ring = object.__new__(R.PrioritizedRing)           # (isinstance(ring, PrioritizedRing) holds)
    ring.capacity, ring.pushed, ring.covered, ring.s = 1000, 1000, 0, _Ring.s
    return ring


# ---- the faults: what one fact looks like on a bare learner (attributes), on the ring, or in the call ----
def _faults(D):
    return {
        "per_ring": dict(ring="per"),
        "exclude": dict(call=dict(exclude=(0, 10))),
        "publish": dict(call=dict(publish=object())),
        "batch": dict(attrs=dict(batch=150)),
        "wide": dict(attrs=dict(wide=True)),
        "hidden": dict(attrs=dict(hidden=(300, 600))),
        "pn": dict(attrs=dict(noise_type="pn")),
        "world": dict(attrs=dict(sync=_Sync(2))),
        "tiled_mode": dict(attrs=dict(tiled_mode=True)),
        "tiled_current": dict(attrs=dict(_tiled_current=True)),
        "grouped": dict(attrs=dict(_before_param_write=lambda: None)),
        "split": dict(attrs=dict(fused=False)),
        "bc": dict(attrs=dict(bc=D.BC())),
    }


def _bare(cls, faults, names, base=()):
    """(bare learner, ring kind, call keywords) with the faults `names` on top of the form's own `base` faults."""
    ag = object.__new__(cls)
    for k, v in dict(batch=120, wide=False, hidden=(250, 500), noise_type="gn", sync=_Sync(1), fused=True, device=None, updates=0, clones=0,
                     evaluations=0, policy_delay=2, rng_seed=1, eta_crit=1e-3, eta_act=1e-4, bp_critic=[0.9, 0.999], bp_actor=[0.9, 0.999],
                     torch=types.SimpleNamespace(int32="i32", float32="f32")).items():
        setattr(ag, k, v)
    ag._ddpg_args = ag._td3_args = _reached
    ring, call = "plain", {}
    for n in tuple(base) + tuple(names):
        f = faults[n]
        for k, v in f.get("attrs", {}).items():
            setattr(ag, k, v)
        ring = f.get("ring", ring)
        call.update(f.get("call", {}))
    return ag, ring, call


GIVEN = "replay_given: one replica on the tuned kernels in Flux order, the one-call form, batch <= 128, no parameter noise"
_IDX = types.SimpleNamespace(dtype="i32", numel=lambda: 128)
_WTS = types.SimpleNamespace(dtype="f32", numel=lambda: 128)

# form -> (class, method, positional arguments behind the ring, the form's own faults, the order: one position per fact, each a list
# of (fault, message) variants of that fact, and the accepted cases: lists of faults that refuse nothing today)
FORMS = {
    "per": ("Agent", "replay", (), ("per_ring",), [
        [("exclude", "prioritized replay: the pipelined forms of replay() (exclude / publish) belong to shems_ddpg_update"),
         ("publish", "prioritized replay: the pipelined forms of replay() (exclude / publish) belong to shems_ddpg_update")],
        [("batch", "prioritized replay: BATCH_SIZE = 150; the sampler draws at most 128 columns")],
        [("wide", "prioritized replay: hidden sizes (250, 500) run layer by layer (shems_wide_*), which has no weighted head"),
         ("hidden", "prioritized replay: hidden sizes (300, 600) run layer by layer (shems_wide_*), which has no weighted head")],
        [("pn", "prioritized replay: parameter noise (noise_type = 'pn') adapts between getData and the updates of replay()")],
        [("world", "prioritized replay: data-parallel replicas do not exchange priorities")],
        [("tiled_mode", "prioritized replay: the tiled working layout (use_tiled)")],
        [("grouped", "prioritized replay: a learner of a learner group keeps its own working layout")],
        [("split", "prioritized replay: the split form of replay() (fused = False)")],
    ], [[], ["tiled_current"]]),
    "given": ("Agent", "replay_given", (_IDX, _WTS), (), [
        [("bc", "replay_given: bc with given slots and weights: the weighted update has no behaviour-regularised head")],
        [("batch", GIVEN)], [("wide", GIVEN), ("hidden", GIVEN)], [("pn", GIVEN)], [("world", GIVEN)], [("tiled_mode", GIVEN)],
        [("grouped", GIVEN)], [("split", GIVEN)],
    ], [[], ["tiled_current"], ["per_ring"]]),
    "clone": ("Agent", "clone", (), (), [
        [("per_ring", "clone: the supervised update draws uniformly; a PrioritizedRing has no cloning form")],
        [("wide", "clone: hidden sizes (250, 500) run layer by layer (shems_wide_*), which has no supervised update"),
         ("hidden", "clone: hidden sizes (300, 600) run layer by layer (shems_wide_*), which has no supervised update")],
        [("batch", "clone: BATCH_SIZE = 150; the supervised update holds at most 128 columns")],
        [("world", "clone: data-parallel replicas do not exchange the supervised gradient")],
        [("grouped", "clone: a learner of a learner group keeps its own working layout")],
    ], [[], ["split"], ["tiled_mode"], ["tiled_current"], ["pn"], ["bc"], ["publish"]]),
    "evaluate": ("Agent", "evaluate", (), (), [
        [("per_ring", "evaluate: the critic-only update draws uniformly; a PrioritizedRing has no critic-only form")],
        [("wide", "evaluate: hidden sizes (250, 500) run layer by layer (shems_wide_*), which has no critic-only update"),
         ("hidden", "evaluate: hidden sizes (300, 600) run layer by layer (shems_wide_*), which has no critic-only update")],
        [("batch", "evaluate: BATCH_SIZE = 150; the critic-only update holds at most 128 columns")],
        [("world", "evaluate: data-parallel replicas do not exchange the critic-only gradient")],
        [("grouped", "evaluate: a learner of a learner group keeps its own working layout")],
    ], [[], ["split"], ["tiled_mode"], ["tiled_current"], ["pn"], ["bc"]]),
    "bc": ("Agent", "replay", (), ("bc",), [
        [("per_ring", "replay: bc with a PrioritizedRing: the weighted update has no behaviour-regularised head")],
        [("batch", "replay: bc with BATCH_SIZE = 150; the behaviour-regularised update holds at most 128 columns")],
        [("wide", "replay: bc with a wide network: hidden sizes beyond (250, 500) run layer by layer (shems_wide_*), which has no "
                  "behaviour-regularised head"),
         ("hidden", "replay: bc with a wide network: hidden sizes beyond (250, 500) run layer by layer (shems_wide_*), which has no "
                    "behaviour-regularised head")],
        [("pn", "replay: bc with parameter noise (noise_type = 'pn'), which adapts between getData and the updates of replay()")],
        [("world", "replay: bc with data-parallel replicas (sync.world = 2): the split form has no behaviour-regularised head")],
        [("tiled_mode", "replay: bc with the tiled working layout (use_tiled): there is no tiled behaviour-regularised gradient launch"),
         ("tiled_current", "replay: bc with the tiled working layout (use_tiled): there is no tiled behaviour-regularised gradient launch")],
        [("grouped", "replay: bc for a learner of a learner group: learner groups have no behaviour-regularised update")],
        [("split", "replay: bc with the split form of replay() (fused = False)")],
    ], [[], ["exclude"], ["publish"]]),
}
_TD3_ORDER = [
    [("per_ring", "TD3: the twin-critic update has no weighted head; a PrioritizedRing belongs to ddpg.Agent")],
    [("exclude", "TD3: the pipelined forms of replay() (exclude / publish) belong to shems_ddpg_update"),
     ("publish", "TD3: the pipelined forms of replay() (exclude / publish) belong to shems_ddpg_update")],
    [("batch", "TD3: BATCH_SIZE = 150; the twin-critic update holds at most 128 columns")],
    [("pn", "TD3: parameter noise (noise_type = 'pn')")],
    [("world", "TD3: data-parallel replicas do not exchange the second critic's gradient")],
    [("tiled_mode", "TD3: the tiled working layout (use_tiled)"), ("tiled_current", "TD3: the tiled working layout (use_tiled)")],
    [("grouped", "TD3: a learner of a learner group keeps its own working layout")],
]
FORMS["td3"] = ("TD3Agent", "replay", (), (), _TD3_ORDER, [[], ["split"], ["wide"], ["hidden"]])
FORMS["td3+bc"] = ("TD3Agent", "replay", (), ("bc",), _TD3_ORDER, [[], ["split"], ["wide"], ["hidden"]])     # (bc_refusals is not consulted)


def _rows():
    rows = []
    for form, (_, _, _, _, order, accepted) in FORMS.items():
        for variants in order:
            rows += [(form, (fault,), msg) for fault, msg in variants]
        for first, second in zip(order, order[1:]):
            rows.append((form, (first[0][0], second[0][0]), first[0][1]))
        rows += [(form, tuple(faults), None) for faults in accepted]
    return rows


ROWS = _rows()


@pytest.fixture
def lazy_declarations_are_sentinels(monkeypatch):
    D, _, _, capi = _mods()
    monkeypatch.setattr(D, "_declare_per", _reached)
    monkeypatch.setattr(capi, "declare_bc", _reached)
    monkeypatch.setattr(capi, "lib", _reached)


@pytest.mark.parametrize("form,faults,message", ROWS, ids=[f"{f}-{'+'.join(n) or 'none'}" for f, n, _ in ROWS])
def test_update_form_refusals(form, faults, message, lazy_declarations_are_sentinels):
    D, T, R, _ = _mods()
    cls, method, args, base, _, _ = FORMS[form]
    ag, ring, call = _bare(getattr(D, cls, None) or getattr(T, cls), _faults(D), faults, base)
    ring = _per_ring(R) if ring == "per" else _Ring()
    if message is None:
        with pytest.raises(Reached):
            getattr(ag, method)(ring, *args, **call)
        return
    with pytest.raises(NotImplementedError) as ei:
        getattr(ag, method)(ring, *args, **call)
    assert str(ei.value) == message
    assert (ag.updates, ag.clones, ag.evaluations) == (0, 0, 0)


def test_row_count():
    """The figure the pull request states: rows of the table above plus the rows of the three tests below."""
    assert len(ROWS) == 129


# ---- Agent.replay's own refusal: it stands behind the argument record (the order of the commit before the table) ----
@pytest.mark.parametrize("faults,message", [(("batch", "pn"), "parameter-noise adaptation with BATCH_SIZE > 128"), (("batch",), None), (("pn",), None),
                                            ((), None)])
def test_replay_parameter_noise_beyond_one_pass(faults, message, lazy_declarations_are_sentinels):
    D, _, _, _ = _mods()
    ag, _, call = _bare(D.Agent, _faults(D), faults)
    ag._ddpg_args = lambda *a, **k: D.DdpgArgs()
    ag._stream = lambda: None
    ag._replay_wide = ag._critic_grad_ex = _reached      # the two routes behind the refusal: sub-batches, the split form ("pn")
    ag.L = types.SimpleNamespace(shems_ddpg_update=_reached)
    with pytest.raises(Reached if message is None else NotImplementedError) as ei:
        ag.replay(_Ring(), **call)
    assert message is None or str(ei.value) == message


# ---- TD3Agent: the constructor and the methods it always refuses ----
TD3_INIT = [
    ("wide", dict(wide=True), NotImplementedError, "TD3: hidden sizes (250, 500) run layer by layer (shems_wide_*), which has no twin-critic update"),
    ("hidden", dict(hidden=(300, 600)), NotImplementedError,
     "TD3: hidden sizes (300, 600) run layer by layer (shems_wide_*), which has no twin-critic update"),
    ("pn", dict(noise_type="pn"), NotImplementedError,
     "TD3: parameter noise (noise_type = 'pn') adapts between getData and the updates of replay(); the TD3 update is one call"),
    ("slab", dict(tensors={}), NotImplementedError,
     "TD3: a learner of a learner group keeps its state in the group's slab; twin critics for a group are td3.TD3LearnerGroup"),
    ("sigma_trg", dict(sigma_trg=-0.5), ValueError, "TD3: sigma_trg = -0.5, clip_trg = 0.5 must be finite and >= 0"),
    ("policy_delay", dict(policy_delay=0), ValueError, "policy_delay = 0: the actor moves every 1 or more updates"),
]
_TD3_INIT_ORDER = ["wide", "pn", "slab", "sigma_trg", "policy_delay"]
TD3_INIT_ROWS = [((n,), exc, msg) for n, _, exc, msg in TD3_INIT] + \
                [((a, b), *next((e, m) for n, _, e, m in TD3_INIT if n == a)) for a, b in zip(_TD3_INIT_ORDER, _TD3_INIT_ORDER[1:])] + \
                [((), Reached, None), (("clip_trg_zero",), Reached, None)]


@pytest.mark.parametrize("faults,exc,message", TD3_INIT_ROWS, ids=["+".join(f) or "none" for f, _, _ in TD3_INIT_ROWS])
def test_td3_constructor_refusals(faults, exc, message, monkeypatch):
    D, T, _, _ = _mods()
    monkeypatch.setattr(D.Agent, "__init__", _reached)
    kw = dict(clip_trg=0.0) if faults == ("clip_trg_zero",) else {}
    for f in faults:
        kw.update(next((k for n, k, _, _ in TD3_INIT if n == f), {}))
    with pytest.raises(exc) as ei:
        T.TD3Agent(**kw)
    assert message is None or str(ei.value) == message


@pytest.mark.parametrize("call,message", [
    (lambda ag: ag.use_tiled(True), "TD3: the tiled working layout (use_tiled) holds the actor's and critic 1's layer-2 state only"),
    (lambda ag: ag.use_tiled(), "TD3: the tiled working layout (use_tiled) holds the actor's and critic 1's layer-2 state only"),
    (lambda ag: ag.evaluate(_Ring()), "TD3: evaluate() is the critic-only update of ONE critic; the twin critics have none"),
    (lambda ag: ag.enable_data_parallel(None), "TD3: data-parallel replicas do not exchange the second critic's gradient"),
    (lambda ag: ag.replay_given(_Ring(), None, None),
     "TD3: replay_given is the single-critic update (shems_ddpg_update_given); the twin critics have none"),
], ids=["use_tiled(True)", "use_tiled()", "evaluate", "enable_data_parallel", "replay_given"])
def test_td3_always_refused(call, message):
    _, T, _, _ = _mods()
    ag = object.__new__(T.TD3Agent)                          # (no attribute at all: nothing is read before the refusal)
    with pytest.raises(NotImplementedError) as ei:
        call(ag)
    assert str(ei.value) == message
    assert ag.use_tiled(False) is ag and ag.tiled_mode is False      # the one accepted call: switching the mode off


def test_bc_refusals_is_the_bc_form_of_the_table():
    """The free function a caller without a learner asks (imitation.offline's checks, tests/test_bc_host.py): the same words as
    Agent.replay with bc set, fact by fact, in the same order."""
    D, _, _, _ = _mods()
    order = FORMS["bc"][4]
    kws = [dict(prioritized=True), dict(batch=150), dict(wide=True), dict(noise_type="pn"), dict(world=2), dict(tiled=True), dict(grouped=True),
           dict(fused=False)]
    assert len(kws) == len(order)
    for i, (kw, variants) in enumerate(zip(kws, order)):
        for extra in ({},) + ((kws[i + 1],) if i + 1 < len(kws) else ()):
            with pytest.raises(NotImplementedError) as ei:
                D.bc_refusals("replay", **kw, **extra)
            assert str(ei.value) == variants[0][1]
    assert D.bc_refusals("replay") is None and D.bc_refusals("replay", batch=128) is None

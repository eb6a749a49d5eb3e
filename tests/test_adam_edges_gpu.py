"""ADAM + the soft target update (csrc/shems_adam.h) on the GPU, held to the float64 definition (tests/adam_ref.py) at the value edges
of the elementwise arithmetic and over a whole training horizon of the beta powers.

1. The apply entry points take a gradient buffer: the tests write p, m, v, target and g of their own choosing (tests/adam_cases.py: every
   gradient class in every moment state in every run of 64 elements), call the entry point once, and compare all four outputs.
2. The grouped throughput kernels fuse ADAM into the gradient launches: the tests write late moments, set the beta powers of updates
   7 000 and 72 072, run one update with store_grad on, and hold params, targets, m and v to the reference from the kernel's own gradient.

The metric is the step, not the parameter (tests/adam_ref.py:errors): (a) the new value within N ulp of the reference's, (b) where the
reference's step exceeds 64 ulp of the old value, the kernel's step within R of it, and (b) again with a far smaller R on the steps that
are at least 2^20 ulp of the old value (a parameter of exactly 0 or 1e-12 resolves its step to the last bit).  N and R are 4 x what a
plain fp32 twin of the formulas costs against float64 (tests/test_adam_horizon_host.py measures that on every run; the figures and the
kernels' own are in profiles/adam_edges_errors.txt).  m and v are held to the reference's bits, one fp32 smallest normal aside: whether
subnormal results are flushed is the device's affair -- the MI355X is observed NOT to flush (every m and v below came back bit for bit,
subnormal ones included)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import adam_cases as K
import adam_ref as AR
import util as U

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENTINEL = -777.25
GUARD = 64
SIDES = dict(critic=("critic", "m_critic", "v_critic", "critic_t", "grad_critic"), actor=("actor", "m_actor", "v_actor", "actor_t", "grad_actor"))


def _mods():
    torch = pytest.importorskip("torch")
    S = U.pkg()
    mod = lambda n: importlib.import_module(U.PKG_NAME + "." + n)
    return torch, S, mod("ddpg"), mod("group"), mod("td3")


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


# =============================================================================================== 1. the apply entry points ==
class Guarded:
    """An Agent whose every device tensor is a view into ONE buffer, 64 sentinel words before and after each: whatever a launch writes
    outside the views it was given shows."""
    def __init__(self, hidden=(250, 500), wide=None, layout=None):
        torch, S, D, G, T = _mods()
        L = D._declare()
        nws = C.c_int64(0)
        is_wide = D.is_wide(hidden) if wide is None else wide
        lay = tuple(layout) if layout is not None else tuple(hidden)
        if is_wide:
            S._capi.check(L.shems_wide_workspace_floats(*lay, C.byref(nws)))
            na, nc = D.net_size(9, 2, lay), D.net_size(11, 1, lay)
        else:
            S._capi.check(L.shems_ddpg_workspace_floats(C.byref(nws)))
            na, nc = D.N_ACTOR, D.N_CRITIC
        sizes = dict(actor=na, critic=nc, actor_t=na, critic_t=nc, m_actor=na, v_actor=na, m_critic=nc, v_critic=nc, grad_actor=na, grad_critic=nc,
                     publish=na, s_min=9, s_max=9, losses=2, ws=nws.value)
        self.off, at = {}, GUARD
        for k, n in sizes.items():
            self.off[k] = (at, n)
            at += -(-n // 64) * 64 + GUARD                     # every view 256-byte aligned
        self.base = torch.full((at,), SENTINEL, dtype=torch.float32, device="cuda")
        view = lambda k: self.base[self.off[k][0]:self.off[k][0] + self.off[k][1]]
        self.publish = view("publish")
        self.ag = D.Agent(seed=3, hidden=hidden, wide=wide, layout=layout, tensors={k: view(k) for k in sizes if k != "publish"})
        self.torch, self.D, self.n = torch, D, dict(actor=na, critic=nc)
        self.lay, self.hidden, self.wide = lay, tuple(hidden), is_wide

    def snapshot(self):
        return self.base.view(self.torch.int32).clone()

    def changed_outside(self, before, names):
        """Words that differ from `before` outside the views `names`."""
        diff = self.base.view(self.torch.int32) != before
        for k in names:
            o, n = self.off[k]
            diff[o:o + n] = False
        return int(diff.sum())


def _embed(g, side, a):
    """A case's vector (own size of the network) in the layout the kernels run at: as is, or zero-padded (ddpg.pad_net_to)."""
    if g.lay == g.hidden:
        return np.ascontiguousarray(a[:g.n[side]], f32)
    i, o = (11, 1) if side == "critic" else (9, 2)
    return g.D.pad_net_to(a[:g.D.net_size(i, o, g.hidden)], i, o, g.hidden, g.lay)


def _apply_all_cases(g, entry, tiled=False):
    torch, ag = g.torch, g.ag
    st = ag._stream()
    up = lambda t, a: t.copy_(torch.from_numpy(np.array(a, f32)))           # (a copy: the cases are shared and read-only)
    for side in ("critic", "actor"):
        critic = side == "critic"
        kp, km, kv, kt, kg = SIDES[side]
        i_d, o_d = (11, 1) if critic else (9, 2)
        own = g.D.net_size(i_d, o_d, g.hidden)
        for name, *_ in K.apply_cases(critic):
            case = K.apply_case(critic, name)
            own_blocks = [(lo, hi) for _, lo, hi in _blocks_of(g.hidden, i_d, o_d)]
            K.assert_not_vacuous(dict(g=case["g"][:own], old=tuple(a[:own] for a in case["old"]), delta=case["delta"][:own]), own_blocks)
            old = tuple(_embed(g, side, a) for a in case["old"])
            grad, ref = _embed(g, side, case["g"]), tuple(_embed(g, side, a) for a in case["ref"])
            for k, a in zip((kp, km, kv, kt, kg), old + (grad,)):
                up(getattr(ag, k), a)                           # (tiled mode: reading the property brings the Flux-order view up to date first)
            if not critic:
                g.publish.fill_(SENTINEL)
            ag.tau = case["tau"]
            if critic:
                ag.eta_crit, ag.bp_critic = case["eta"], list(case["bp"])
            else:
                ag.eta_act, ag.bp_actor = case["eta"], list(case["bp"])
            if tiled:
                assert ag._enter_tiled() and ag._tiled_current  # the regions hold the layer-2 state; the apply entry points speak Flux order
            d = ag._ddpg_args()                                 # (and leaves the tiled regions again)
            region = ag._w2t.view(torch.int32).clone() if tiled else None
            before = g.snapshot()
            if critic:
                ag._critic_apply(d, 1.0, st)
            else:
                ag._actor_apply_pub(d, 1.0, g.publish, st)
            torch.cuda.synchronize()
            written = (kp, km, kv, kt) + (() if critic else ("publish",))
            assert g.changed_outside(before, written) == 0, (entry, side, name, "a word outside p, m, v and the target changed")
            if tiled:                                           # the round trip through the tiled regions keeps every bit, and the apply left them alone
                assert torch.equal(ag._w2t.view(torch.int32), region)
                assert ag._enter_tiled()
                ag.flux_()
                assert g.changed_outside(before, written) == 0
            new = tuple(getattr(ag, k).cpu().numpy() for k in (kp, km, kv, kt))
            errs = AR.all_errors(old, new, ref)
            sub = [(np.abs(r) < AR.F32_MIN_NORMAL) & (r != 0) for r in ref[1:3]]                  # the reference's subnormal m and v
            kept = [int((_bits(k)[s_] == _bits(r)[s_]).sum()) for k, r, s_ in zip(new[1:3], ref[1:3], sub)]
            print(f"{entry} {side} {name}:", {k: (v["ulp"], v["rel"], v["rel_resolved"]) for k, v in errs.items()},
                  f"subnormal m, v in the reference: {[int(s_.sum()) for s_ in sub]}, of which the device returned bit for bit: {kept}")
            AR.assert_within_bounds(errs, (entry, side, name))
            if case["tau"] == 0.0:                              # the TD3 hold relies on it
                assert np.array_equal(_bits(new[3]), _bits(old[3])), (entry, side, name, "tau = 0 must keep the target's bytes")
            if case["tau"] == 1.0:                              # the clone relies on it
                assert np.array_equal(_bits(new[3]), _bits(new[0])), (entry, side, name, "tau = 1 must leave the target on the parameters, bit for bit")
            if not critic:
                assert np.array_equal(_bits(g.publish.cpu().numpy()), _bits(new[0])), (entry, name, "publish")
            if g.lay != g.hidden:                               # the padding: zero bytes before, zero bytes after
                pad = g.D.pad_net_to(np.ones(own, f32), i_d, o_d, g.hidden, g.lay) == 0
                assert pad.sum() == g.n[side] - own
                for a in new:
                    assert not _bits(a)[pad].any(), (entry, side, name, "padding")


def _blocks_of(hidden, i_d, o_d):
    h1, h2 = hidden
    o = np.cumsum([0, i_d * h1, h1, h1 * h2, h2, h2 * o_d, o_d])
    return [(n, int(o[k]), int(o[k + 1])) for k, n in enumerate(("W1", "b1", "W2", "b2", "W3", "b3"))]


def test_apply_entry_points_in_flux_order():
    """shems_ddpg_critic_apply / shems_ddpg_actor_apply_pub: 129 001 and 129 002 parameters (a tail of one and of two elements behind the
    last float4)."""
    g = Guarded()
    assert not g.wide and g.n == dict(actor=129002, critic=129001)
    _apply_all_cases(g, "shems_ddpg_*_apply")


def test_apply_entry_points_with_the_tiled_mode_on():
    """The single learner's tiled working mode: the regions hold the layer-2 state when the call arrives, the entry points bring the
    Flux-order view up to date, and the values -- subnormal, huge, exactly zero -- survive both conversions bit for bit."""
    g = Guarded()
    g.ag.use_tiled(True)
    _apply_all_cases(g, "shems_ddpg_*_apply, tiled mode", tiled=True)


def test_wide_apply_entry_points_at_250_500():
    g = Guarded(wide=True)
    assert g.wide and g.n == dict(actor=129002, critic=129001)
    _apply_all_cases(g, "shems_wide_*_apply (250, 500)")


def test_wide_apply_entry_points_at_a_padded_size():
    """A (280, 560) network zero-padded into the (300, 600) layout: the sweep runs over the padding too, which must stay zero bytes."""
    g = Guarded(hidden=(280, 560), wide=True, layout=(300, 600))
    assert g.n == dict(actor=184802, critic=K.N_MAX)
    _apply_all_cases(g, "shems_wide_*_apply (280, 560) in (300, 600)")


# ============================================================================== 2. the grouped kernels at the late regime ==
FLUX8 = ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic")
CRITIC2 = ("critic2", "critic2_t", "m_critic2", "v_critic2")
NETS = dict(actor=("actor", "m_actor", "v_actor", "actor_t", "grad_actor"), critic=("critic", "m_critic", "v_critic", "critic_t", "grad_critic"),
            critic2=("critic2", "m_critic2", "v_critic2", "critic2_t", "grad_critic2"))
TILE_WORDS = 32 * 4 * 64 * 64          # a network's tiled region: [32 tiles][m | v | p | target][64 x 64]
PAD_WORDS = TILE_WORDS - 4 * 250 * 500  # of which hold no element of the 250 x 500 matrices


def _view(grp, name):
    o, n = grp.layout[name]
    return grp.slab[:, o:o + n]


def _np_all(grp, name):
    return _view(grp, name).cpu().numpy()


@np.errstate(all="ignore")
def _late_rows(name, L, n):
    """[L][n] late moments: one generated vector per array, rolled by 32 l (the states alternate in runs of 16) and scaled per learner."""
    m, v = K.late_moments(sum(map(ord, name)), n)
    src = m if name.startswith("m_") else v
    return np.stack([np.roll(src, 32 * l) * f32(1 + l / 64) if name.startswith("m_") else np.roll(src, 32 * l) for l in range(L)])


class Late:
    """A group with the pad words of its tiled regions located, and the means to put it into the late regime and check one update."""
    def __init__(self, torch, grp, nets):
        self.torch, self.grp, self.nets = torch, grp, nets
        self.hidden = grp.hidden if grp.form == "wide" else (250, 500)       # the layout the kernels run at
        self.regions = [r for r in ("w2t_actor", "w2t_critic", "w2t_critic2") if grp.tiled and r in grp.layout]
        self.pad = {}
        if grp.tiled:                  # the words of a region that hold nothing: those that do not follow the Flux-order blocks
            grp.flux_()
            names = [k for net in nets for k in NETS[net][:4]]
            keep = {k: _view(grp, k).clone() for k in names}
            for k in names:
                _view(grp, k).fill_(1.0)
            grp.flux_changed()
            assert grp._use_tiled()
            for r in self.regions:
                self.pad[r] = _view(grp, r)[0] != 1.0
                assert int(self.pad[r].sum()) == PAD_WORDS, (r, int(self.pad[r].sum()))
            grp.flux_()
            for k in names:
                _view(grp, k).copy_(keep[k])
            grp.flux_changed()

    def update(self, what, run, stepped, steps, taus=None, held=(), own=None):
        """Write late moments, set the beta powers of `steps` = dict(critic=, actor=), run() one update, and hold every network in
        `stepped` to the reference from the stored gradient; the arrays of `held` networks keep their bytes.  own: {network: bool [L][n]},
        the elements that are a learner's own units in a zero-padded layout (None: all) -- the padding holds zero moments, and zero bytes
        in all four arrays after the update."""
        torch, grp = self.torch, self.grp
        L = grp.count
        grp.flux_()
        for net in self.nets:
            for k in NETS[net][1:3]:
                rows = _late_rows(k, L, grp.layout[k][1])
                if own is not None:
                    rows[~own[net]] = 0
                _view(grp, k).copy_(torch.from_numpy(rows))
        grp.flux_changed()
        for ag in grp.learners:
            ag.bp_critic, ag.bp_actor = list(K.powers(steps["critic"])), list(K.powers(steps["actor"]))
        old = {k: _np_all(grp, k) for net in self.nets for k in NETS[net][:4]}
        pads = {}
        if grp.tiled:
            assert grp._use_tiled()
            pads = {r: _view(grp, r)[:, self.pad[r]].view(torch.int32).clone() for r in self.regions}
        run()
        for r, b in pads.items():      # before anything else touches the regions
            assert torch.equal(_view(grp, r)[:, self.pad[r]].view(torch.int32), b), (what, r, "pad words of the tiled region were written")
        grp.flux_()
        torch.cuda.synchronize()
        for net in self.nets:
            kp, km, kv, kt, kg = NETS[net]
            new = tuple(_np_all(grp, k) for k in (kp, km, kv, kt))
            was = tuple(old[k] for k in (kp, km, kv, kt))
            if net not in stepped:
                assert net in held
                for k, a, b in zip((kp, km, kv, kt), was, new):
                    assert np.array_equal(_bits(a), _bits(b)), (what, k, "must keep its bytes")
                continue
            grad = _np_all(grp, kg)
            n = grad.shape[1]
            critic = net != "actor"
            for _, lo, hi in _blocks_of(self.hidden, 11 if critic else 9, 1 if critic else 2):
                assert (np.abs(grad[:, lo:hi]).max(1) > 0).all(), (what, net, "a gradient block of a learner is all zero")
            eta = np.repeat([ag.eta_crit if critic else ag.eta_act for ag in grp.learners], n)
            tau = np.repeat([f32(ag.tau) for ag in grp.learners] if taus is None else np.broadcast_to(f32(taus), L), n).astype(f32)
            bp = K.powers(steps["critic" if critic else "actor"])
            flat = lambda a: np.ascontiguousarray(a).reshape(-1)
            ref = AR.reference(*(flat(a) for a in was), flat(grad), eta, tau, *bp)
            mine = slice(None) if own is None else own[net].reshape(-1)
            assert (ref[1][mine] != 0).all(), "late moments: the reference's step of every element is non-zero"
            if own is not None:
                for a in new:
                    assert not _bits(a)[~own[net]].any(), (what, net, "the padding must stay zero bytes")
            errs = AR.all_errors(tuple(flat(a) for a in was), tuple(flat(a) for a in new), ref)
            print(f"{what} {net}:", {k: (v["ulp"], v["rel"], v["rel_resolved"], v["n_resolved"]) for k, v in errs.items()})
            AR.assert_within_bounds(errs, (what, net))
            if taus == 0.0:
                assert np.array_equal(_bits(new[3]), _bits(was[3])), (what, net, "a held target must keep its bytes")
            if taus == 1.0:
                assert np.array_equal(_bits(new[3]), _bits(new[0])), (what, net, "tau = 1: the target on its network, bit for bit")
        for ag in grp.learners:        # the host's powers moved on, and stayed inside (0, 1)
            assert 0.0 < ag.bp_critic[0] < 1.0 and 0.0 < ag.bp_actor[0] < 1.0


GROUP_PARAMS = [(L, tiled, records) for L in (2, 48) for tiled in (True, False) for records in (False, True)]
GROUP_IDS = [f"L{L}-{'tiled' if t else 'flux'}-{'records' if r else 'shared'}" for L, t, r in GROUP_PARAMS]
S7, S72 = 7000, K.THESIS_UPDATES


def _free(torch):
    import gc
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=GROUP_PARAMS, ids=GROUP_IDS)
def ddpg_group(request):
    import test_group_td3_gpu as GT
    L, tiled, records = request.param
    torch, grp = GT._ddpg_group(L, batch=K.GROUP_BATCH, tiled=tiled, hparams=K.group_records(L) if records else None)
    assert grp.tiled == tiled and grp.form == "throughput" and (grp.envs_per_learner, grp.capacity) == (K.GROUP_E, K.GROUP_CAP)
    yield Late(torch, grp, ("critic", "actor")), request.param
    del grp
    _free(torch)


@pytest.mark.parametrize("family", ["ddpg", "clone", "critic-only"])
def test_grouped_ddpg_families_at_the_late_regime(ddpg_group, family):
    """shems_ddpg_group_update_tp, shems_ddpg_group_clone_update_tp (tau = 1: the targets on their actors) and
    shems_ddpg_group_critic_update_tp: one update each, the critic at one late step and the actor at the other."""
    late, (L, tiled, records) = ddpg_group
    grp = late.grp
    what = f"{family}, {L} learners, tiled={tiled}, records={records}"
    if family == "ddpg":
        late.update(what, lambda: grp.replay(tick=3), ("critic", "actor"), dict(critic=S7, actor=S72))
    elif family == "clone":
        late.update(what, lambda: grp.clone(None, tick=3), ("actor",), dict(critic=S72, actor=S7), taus=1.0, held=("critic",))
    else:
        late.update(what, lambda: grp.evaluate(None, tick=3), ("critic",), dict(critic=S72, actor=S7), held=("actor",))
    if records:
        assert len({ag.eta_crit for ag in grp.learners}) > 1 and len({ag.tau for ag in grp.learners}) > 1


@pytest.fixture(scope="module", params=GROUP_PARAMS, ids=GROUP_IDS)
def x_group(request):
    """The *_x entry point: a group whose records carry a ring size (they are built from the shared values when none are given)."""
    import test_group_td3_gpu as GT
    L, tiled, records = request.param
    sizes = [dict(mem_size=K.GROUP_CAP, batch=K.GROUP_BATCH) for l in range(L)]
    hp = [dict(r, **s) for r, s in zip(K.group_records(L), sizes)] if records else sizes
    torch, grp = GT._ddpg_group(L, batch=K.GROUP_BATCH, tiled=tiled, hparams=hp)
    assert grp._x and grp.tiled == tiled
    yield Late(torch, grp, ("critic", "actor")), request.param
    del grp
    _free(torch)


def test_grouped_x_entry_point_at_the_late_regime(x_group):
    late, (L, tiled, records) = x_group
    late.update(f"ddpg_x, {L} learners, tiled={tiled}, records={records}", lambda: late.grp.replay(tick=3), ("critic", "actor"), dict(critic=S72, actor=S7))


@pytest.fixture(scope="module", params=GROUP_PARAMS, ids=GROUP_IDS)
def td3_group(request):
    import test_group_td3_gpu as GT
    L, tiled, records = request.param
    torch, grp = GT._group(L, batch=K.GROUP_BATCH, tiled=tiled, hparams=K.group_records(L) if records else None)
    assert grp.tiled == tiled
    yield Late(torch, grp, ("critic", "critic2", "actor")), request.param
    del grp
    _free(torch)


@pytest.mark.parametrize("policy", [True, False])
def test_grouped_td3_at_the_late_regime(td3_group, policy):
    """shems_td3_group_update_tp on a policy step, and off one: the critics step with their targets held (tau = 0), the actor, its
    moments and its target keep their bytes."""
    late, (L, tiled, records) = td3_group
    grp = late.grp
    what = f"td3 {'policy' if policy else 'hold'}, {L} learners, tiled={tiled}, records={records}"
    if policy:
        late.update(what, lambda: grp.replay(tick=3, update_policy=True), ("critic", "critic2", "actor"), dict(critic=S7, actor=S72))
    else:
        late.update(what, lambda: grp.replay(tick=3, update_policy=False), ("critic", "critic2"), dict(critic=S72, actor=S7), taus=0.0, held=("actor",))


@pytest.fixture(scope="module", params=GROUP_PARAMS, ids=GROUP_IDS)
def per_group(request):
    import test_group_per_gpu as GP
    L, tiled, records = request.param
    torch, grp = GP._group(L, batch=K.GROUP_BATCH, tiled=tiled, hparams=K.group_records(L) if records else None)
    assert grp.tiled == tiled
    yield Late(torch, grp, ("critic", "actor")), request.param
    del grp
    _free(torch)


def test_grouped_prioritized_update_at_the_late_regime(per_group):
    late, (L, tiled, records) = per_group
    late.update(f"per, {L} learners, tiled={tiled}, records={records}", lambda: late.grp.replay(tick=3), ("critic", "actor"), dict(critic=S72, actor=S7))


@pytest.mark.parametrize("step", [100, K.THESIS_UPDATES])
@pytest.mark.parametrize("L,tiled", [(2, True), (2, False), (48, True), (48, False)])
def test_records_with_the_shared_values_leave_the_shared_bytes_away_from_update_1(L, tiled, step):
    """tests/test_group_hparams_gpu.py:test_uniform_records_equal_the_shared_entry_points_bitwise asserts this from a fresh group (updates
    1 .. 3).  Here with late moments at update 100, where 1 - bp1 is not yet 1 and a quotient formed in another precision shows in the
    bytes, and at update 72 072: the *_hp kernels form eta / (1 - bp1) on the device, the plain ones take the host's quotient."""
    import test_group_td3_gpu as GT
    out = []
    for hp in (None, [dict(batch=K.GROUP_BATCH) for _ in range(L)]):
        torch, grp = GT._ddpg_group(L, batch=K.GROUP_BATCH, tiled=tiled, hparams=hp)
        assert (grp._hp_dev is not None) == (hp is not None)
        for k in ("m_actor", "v_actor", "m_critic", "v_critic"):
            _view(grp, k).copy_(torch.from_numpy(_late_rows(k, L, grp.layout[k][1])))
        grp.flux_changed()
        for ag in grp.learners:
            ag.bp_critic, ag.bp_actor = list(K.powers(step)), list(K.powers(step))
        grp.replay(tick=3)
        out.append(GT._side(grp, GT.DDPG_SIDE))
        del grp
    for k in GT.DDPG_SIDE:
        assert torch.equal(out[0][k], out[1][k]), k
    assert float(out[0]["grad_critic"].abs().max()) > 0
    _free(torch)


def test_latency_form_at_update_72072():
    """shems_ddpg_group_update (ADAM inside the gradient launches K3 / K5, grid z = learner)."""
    import test_group_td3_gpu as GT
    torch, S, D, G, T = _mods()
    grp = G.LearnerGroup(3, K.GROUP_E, seed=GT.K.SEED, rng_seed=GT.K.RNG_SEED, capacity=K.GROUP_CAP, form="latency")
    for l, ag in enumerate(grp.learners):
        d, up = GT._fill(torch, grp, l)
        ag.set_params(actor=d["pa"], critic=d["pc"])
        up(ag.actor_t, d["pa_t"])
        up(ag.critic_t, d["pc_t"])
        ag.batch = K.GROUP_BATCH
    assert grp.form == "latency" and not grp.tiled
    Late(torch, grp, ("critic", "actor")).update("latency form", lambda: grp.replay(tick=3), ("critic", "actor"), dict(critic=S72, actor=S72))


def test_wide_group_form_with_per_learner_hidden_sizes_at_update_72072():
    """shems_wide_group_update: k_adam_soft_hp forms eta_l / (1 - bp1) on the device from learner l's record; the networks are zero-padded
    into (300, 600) and their padding -- zero moments, zero gradient -- stays zero bytes."""
    import test_group_wide_gpu as GW
    torch, S, D, G, T = _mods()
    hid = [(300, 600), (250, 500), (200, 400)]
    recs = [dict(r, hidden=h) for r, h in zip(K.group_records(3), hid)]
    env, grp = GW._group(3, K.GROUP_E, cap=K.GROUP_CAP, hparams=recs)
    rng = np.random.default_rng(3)
    masks = {}
    for l, ag in enumerate(grp.learners):
        GW._boost(ag, rng, hid[l])
        masks[l] = dict(actor=GW._pad_mask(D, hid[l], 9, 2), critic=GW._pad_mask(D, hid[l], 11, 1))
    own = {net: np.stack([~masks[l][net] for l in range(3)]) for net in ("actor", "critic")}
    assert all(own[net][0].all() and not own[net][2].all() for net in own)
    Late(torch, grp, ("critic", "actor")).update("wide group form", lambda: grp.replay(tick=3), ("critic", "actor"), dict(critic=S72, actor=S72), own=own)
    env.close()


# =========================================================== 3. every update entry point accepts the settled beta power ==
def test_single_learner_update_entry_points_accept_the_settled_power():
    """tests/test_errors_gpu.py:81 holds the refusals (0.0, 1.0, 1.5).  The accepted side: 0.9^t sticks at 5 units of the smallest
    subnormal double (tests/test_adam_horizon_host.py), and with it every update entry point of the single learner runs, leaves a finite
    state, moves its parameters, and the host's powers stay where they are."""
    import test_ddpg_gpu as TD
    import test_per_gpu as TP
    torch, S, D, ag, ring, h = TD._setup(seed=11, cap=2048)
    T = importlib.import_module(U.PKG_NAME + ".td3")
    late = [K.SETTLED_BP1, K.powers(K.THESIS_UPDATES)[1]]
    assert late[0] * 0.9 == late[0] and 0.0 < late[0] < 1e-300

    def fresh(make=lambda: D.Agent(seed=11), **attrs):
        a = make()
        a.set_params(actor=h["pa"], critic=h["pc"])
        a.set_norm(h["s_min"], h["s_max"])
        a.bp_actor, a.bp_critic = list(late), list(late)
        for k, v in attrs.items():
            setattr(a, k, v)
        return a

    idx = torch.from_numpy(np.concatenate([np.arange(120), np.full(8, -1)]).astype(np.int32)).cuda()
    ones = torch.ones(128, dtype=torch.float32, device="cuda")
    per = TP._per_ring(D, torch, ring, np.linspace(0.1, 2.0, ring.capacity))
    runs = (("shems_ddpg_update", fresh(), lambda a: a.replay(ring, tick=1), "ca"),
            ("the split calls", fresh(fused=False), lambda a: a.replay(ring, tick=1), "ca"),
            ("shems_ddpg_update on the tiled layout", fresh().use_tiled(True), lambda a: a.replay(ring, tick=1), "ca"),
            ("shems_ddpg_update_per", fresh(), lambda a: a.replay(per, tick=1), "ca"),
            ("shems_ddpg_update_given", fresh(), lambda a: a.replay_given(ring, idx, ones), "ca"),
            ("shems_ddpg_clone_update", fresh(), lambda a: a.clone(ring, tick=1), "a"),
            ("shems_ddpg_critic_update", fresh(), lambda a: a.evaluate(ring, tick=1), "c"),
            ("shems_td3_update", fresh(lambda: T.TD3Agent(seed=11, policy_delay=1)), lambda a: a.replay(ring, tick=1), "ca"),
            ("shems_wide_*", fresh(lambda: D.Agent(seed=11, wide=True)), lambda a: a.replay(ring, tick=1), "ca"))
    for what, a, run, moves in runs:
        before = {k: getattr(a, k).clone() for k in ("actor", "critic")}
        run(a)
        torch.cuda.synchronize()
        for k in ("actor", "critic", "actor_t", "critic_t", "m_actor", "v_actor", "m_critic", "v_critic"):
            assert bool(torch.isfinite(getattr(a, k)).all()), (what, k)
        assert (not torch.equal(a.actor, before["actor"])) == ("a" in moves) and (not torch.equal(a.critic, before["critic"])) == ("c" in moves), what
        assert a.bp_actor[0] == a.bp_critic[0] == K.SETTLED_BP1 and 0.0 < a.bp_actor[1] <= late[1] and 0.0 < a.bp_critic[1] <= late[1], what
    # the native loop's record (shems_train_steps, csrc/shems_train.hip:123) takes the same check and advances the powers as C doubles
    wl = D.TrainWorkload(S, torch, 1024, seed=5, updates=1, loop="native")
    wl.agent.bp_actor, wl.agent.bp_critic = list(late), list(late)
    wl.steps(3)
    wl.finish()
    torch.cuda.synchronize()
    assert wl.agent.updates == 3 and bool(torch.isfinite(wl.agent.actor).all()) and bool(torch.isfinite(wl.agent.critic).all())
    assert wl.agent.bp_actor == wl.agent.bp_critic == [K.SETTLED_BP1, late[1] * 0.999 * 0.999 * 0.999]

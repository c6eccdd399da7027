"""GPU: the visibility-gated Adam step (csrc/optim.hip ``adam_visible_kernel`` behind ``sgn_adam_step_visible``,
``FusedAdam.step(visible=...)`` / ``optim.step_many(..., visible=...)``).

The contract: a visible row gets the dense step's ``param`` / ``exp_avg`` / ``exp_avg_sq`` bit for bit, an invisible row
keeps its bits and its gradient is never used, ``state['step']`` advances either way.  The yardstick is the dense
``FusedAdam`` itself (bits) and, on the visible rows, the float64 definition of tests/adam_fp64.py under the rule and the
caps of tests/test_gpu_adam_fp64.py.  R = 1031 rows (odd, no multiple of 4; R x 45 = 46395 elements span twelve
4096-element workgroup chunks), row widths 1, 3, 4 and 45 — a float4 then lies in one row, straddles two, or covers
four — in the six parameter shapes of a Gaussian model.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import adam_fp64 as AF

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 1031
SHAPES = [(R,), (R, 1), (R, 3), (R, 4), (R, 1, 3), (R, 15, 3)]
COMBOS = [(1, AF.HYPERS[0]), (30000, AF.HYPERS[0]), (25, AF.HYPERS[2]), (1000, AF.HYPERS[1])]   # t = 1 and 30000 at eps 1e-15
PATTERNS = ["all", "none", "first", "last", "alternating", "random30", "runs64"]
KINDS = ["bool", "uint8", "int32"]
NAN_BITS = 0x7FC0DEAD                        # a quiet NaN with a payload: "kept its bits" includes the payload
_CACHE = {}


def _shape_id(shape):
    return "x".join(str(s) for s in shape)


def _mask(pattern, rows=R):
    m = torch.zeros(rows, dtype=torch.bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[rows - 1] = True
    elif pattern == "alternating":
        m[0::2] = True
    elif pattern == "random30":
        m = torch.rand(rows, generator=torch.Generator().manual_seed(30)) < 0.3
    elif pattern == "runs64":
        m = (torch.arange(rows) // 64) % 2 == 0
    else:
        assert pattern == "none"
    return m


def _encode(mask, kind):
    """The mask as the visibility tensor of ``kind`` on the device: uint8 visible values are not only 1, int32 are radii
    (visible > 0; invisible rows hold 0 and negative values)."""
    j = torch.arange(mask.numel())
    if kind == "bool":
        vis = mask.clone()
    elif kind == "uint8":
        vis = torch.where(mask, torch.tensor([1, 255, 2, 128], dtype=torch.uint8)[j % 4], torch.zeros((), dtype=torch.uint8))
    else:
        vis = torch.where(mask, (1 + j % 97).int(), torch.tensor([0, -1, 0, -7], dtype=torch.int32)[j % 4])
    assert torch.equal(vis > 0 if kind == "int32" else vis != 0, mask)
    return vis.to(DEV)


def _inputs(shape, seed=0):
    """``adam_fp64.make_case`` in the shape of a parameter: p, g, m, v (CPU), made once and left unchanged."""
    key = ("in", shape, seed)
    if key not in _CACHE:
        c = AF.make_case(math.prod(shape), seed)
        _CACHE[key] = SimpleNamespace(p=c.p.view(shape), g=c.g.view(shape), m=c.m.view(shape), v=c.v.view(shape))
    return _CACHE[key]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _step(x, combo, **step_kw):
    """One ``FusedAdam.step(**step_kw)`` on device copies of ``x.p / g / m / v`` from the state of step t - 1."""
    from sgn_rast.optim import FusedAdam
    t, (lr, b1, b2, eps) = combo
    prm = torch.nn.Parameter(x.p.to(DEV).clone())
    prm.grad = x.g.to(DEV).clone()
    opt = FusedAdam([prm], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[prm] = {"step": torch.tensor(float(t - 1)), "exp_avg": x.m.to(DEV).clone(), "exp_avg_sq": x.v.to(DEV).clone()}
    opt.step(**step_kw)
    st = opt.state[prm]
    return SimpleNamespace(param=prm.detach().cpu(), exp_avg=st["exp_avg"].cpu(), exp_avg_sq=st["exp_avg_sq"].cpu(),
                           grad=prm.grad.cpu(), step=float(st["step"]))


def _dense(shape, combo):
    key = ("dense", shape, combo)
    if key not in _CACHE:
        _CACHE[key] = _step(_inputs(shape), combo)
    return _CACHE[key]


def _expected_bits(dense, x, mask):
    """Per output: the dense result's bits on the rows of ``mask``, the input's bits elsewhere."""
    rows = mask.view(-1, *([1] * (x.p.dim() - 1)))
    return {name: torch.where(rows, _bits(getattr(dense, name)), _bits(before))
            for name, before in zip(AF.NAMES, (x.p, x.m, x.v))}


def _assert_bits(got, want, label):
    for name in AF.NAMES:
        a = _bits(getattr(got, name))
        assert torch.equal(a, want[name]), (label, name, int((a != want[name]).sum()), "elements differ")


# ------------------------------------------------------------------------------------------- 1. bits against dense
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_visible_rows_get_the_dense_step_and_invisible_rows_keep_their_bits(pattern, kind):
    mask = _mask(pattern)
    vis = _encode(mask, kind)
    for shape in SHAPES:
        x = _inputs(shape)
        for combo in COMBOS:
            dense = _dense(shape, combo)
            got = _step(x, combo, visible=vis)
            label = (_shape_id(shape), pattern, kind, AF.combo_id(combo))
            _assert_bits(got, _expected_bits(dense, x, mask), label)
            assert got.step == dense.step == combo[0], label
            assert torch.equal(_bits(got.grad), _bits(x.g)), (label, "the gradient was written")


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_no_visibility_and_all_visible_are_the_dense_step(shape):
    x = _inputs(shape)
    for combo in COMBOS:
        dense = _dense(shape, combo)
        want = {name: _bits(getattr(dense, name)) for name in AF.NAMES}
        _assert_bits(_step(x, combo, visible=None), want, "visible=None")
        for kind in KINDS:
            _assert_bits(_step(x, combo, visible=_encode(_mask("all"), kind)), want, kind)
        prm = torch.nn.Parameter(torch.zeros(1, device=DEV))              # the mapping form with nothing in it
        _assert_bits(_step(x, combo, visible={prm: torch.ones(1, dtype=torch.bool, device=DEV)}), want, "absent")


# ------------------------------------------------------------------------------------------- 2. poison
@pytest.mark.parametrize("where", ["gradient", "moments"])
@pytest.mark.parametrize("pattern", ["alternating", "random30", "runs64", "first", "none"])
def test_poison_in_invisible_rows_has_no_effect(pattern, where):
    mask = _mask(pattern)
    vis = _encode(mask, "int32")
    poison = torch.tensor([math.nan, math.inf, -math.inf])[torch.arange(R) % 3]
    for shape in SHAPES:
        x = _inputs(shape)
        rows = mask.view(-1, *([1] * (len(shape) - 1)))
        bad = poison.view(rows.shape).expand(shape)
        y = SimpleNamespace(p=x.p, g=x.g, m=x.m, v=x.v)
        if where == "gradient":
            y.g = torch.where(rows, x.g, bad)
        else:
            y.m = torch.where(rows, x.m, bad)
            y.v = torch.where(rows, x.v, torch.full((), NAN_BITS, dtype=torch.int32).view(torch.float32))
            assert int((_bits(y.v) == NAN_BITS).sum()) == int((~mask).sum()) * (math.prod(shape) // R)
        for combo in COMBOS[:2]:
            got = _step(y, combo, visible=vis)
            label = (_shape_id(shape), pattern, where, AF.combo_id(combo))
            _assert_bits(got, _expected_bits(_dense(shape, combo), y, mask), label)     # dense: on the CLEAN inputs
            for name in AF.NAMES:
                assert bool(torch.isfinite(getattr(got, name)[mask]).all()), (label, name)
            assert torch.equal(_bits(got.grad), _bits(y.g)), label


# ------------------------------------------------------------------------------------------- 3. the fp64 definition
@pytest.mark.parametrize("combo", COMBOS, ids=AF.combo_id)
def test_visible_rows_are_held_to_the_fp64_definition(combo):
    t, hyper = combo
    mask = _mask("random30")
    vis = _encode(mask, "int32")
    fails = []
    for shape in [(R,), (R, 3), (R, 15, 3)]:
        x = _inputs(shape)
        flat = [a.reshape(-1) for a in (x.p, x.g, x.m, x.v)]
        key = ("fp64", shape, combo)
        if key not in _CACHE:
            ref = AF.definition(*flat, hyper, t)
            _CACHE[key] = (ref, AF.yardstick(*flat, hyper, t), AF.scales(*flat, hyper, t, ref))
        ref, r32, S = _CACHE[key]
        got = _step(x, combo, visible=vis)
        got = SimpleNamespace(**{name: getattr(got, name).reshape(-1) for name in AF.NAMES})
        elements = mask.repeat_interleave(math.prod(shape) // R)
        fails += AF.compare(got, r32, ref, S, elements, f"{_shape_id(shape)} {AF.combo_id(combo)} visible rows")[0]
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------- 4. layout edges
@pytest.mark.parametrize("shape", [(R, 3), (R, 15, 3), (R,)], ids=_shape_id)
def test_a_misaligned_parameter_takes_the_scalar_path_to_the_same_bits(shape):
    """The parameter starts one element into a 16-byte aligned buffer (the scalar path for the whole tensor) and the
    radii one entry into theirs."""
    from sgn_rast.optim import FusedAdam
    x, n = _inputs(shape), math.prod(shape)
    for pattern in ("alternating", "random30", "last"):
        mask = _mask(pattern)
        radii = torch.cat((torch.ones(1, dtype=torch.int32, device=DEV), _encode(mask, "int32")))[1:]
        for combo in COMBOS[:2]:
            t, (lr, b1, b2, eps) = combo
            buf = torch.full((n + 2,), NAN_BITS, dtype=torch.int32).view(torch.float32)
            buf[1: n + 1] = x.p.reshape(-1)
            buf = buf.to(DEV)
            prm = torch.nn.Parameter(buf[1: n + 1].view(shape))
            assert prm.data_ptr() % 16 == 4 and prm.is_contiguous() and radii.data_ptr() % 16 == 4
            prm.grad = x.g.to(DEV).clone()
            opt = FusedAdam([prm], lr=lr, betas=(b1, b2), eps=eps)
            opt.state[prm] = {"step": torch.tensor(float(t - 1)), "exp_avg": x.m.to(DEV).clone(),
                              "exp_avg_sq": x.v.to(DEV).clone()}
            opt.step(visible=radii)
            st = opt.state[prm]
            got = SimpleNamespace(param=prm.detach().cpu(), exp_avg=st["exp_avg"].cpu(), exp_avg_sq=st["exp_avg_sq"].cpu())
            _assert_bits(got, _expected_bits(_dense(shape, combo), x, mask), (_shape_id(shape), pattern, AF.combo_id(combo)))
            assert _bits(buf)[[0, n + 1]].tolist() == [NAN_BITS, NAN_BITS], "the words around the parameter were written"


@pytest.mark.parametrize("visible_row", [True, False])
def test_one_row_and_no_rows(visible_row):
    """R = 1 at widths 1, 45 and 4099 (a row wider than a workgroup's chunk) and an R = 0 tensor, in one call."""
    from sgn_rast import optim
    combo = COMBOS[0]
    t, (lr, b1, b2, eps) = combo
    shapes = [(1,), (1, 15, 3), (0, 3), (1, 4099)]
    xs = [_inputs(s, seed=2) if math.prod(s) else None for s in shapes]
    prms, vis = [], {}
    for s, x in zip(shapes, xs):
        prm = torch.nn.Parameter(torch.zeros(s, device=DEV) if x is None else x.p.to(DEV).clone())
        prm.grad = torch.zeros(s, device=DEV) if x is None else x.g.to(DEV).clone()
        prms.append(prm)
        vis[prm] = torch.full((s[0],), 3 if visible_row else -3, dtype=torch.int32, device=DEV)
    opt = optim.FusedAdam(prms, lr=lr, betas=(b1, b2), eps=eps)
    for prm, x in zip(prms, xs):
        z = lambda a: torch.zeros_like(prm) if x is None else a.to(DEV).clone()
        opt.state[prm] = {"step": torch.tensor(float(t - 1)), "exp_avg": z(x and x.m), "exp_avg_sq": z(x and x.v)}
    optim.step_many([opt], visible=vis)
    for s, prm, x in zip(shapes, prms, xs):
        st = opt.state[prm]
        assert float(st["step"]) == t, s
        if x is None:
            continue
        got = SimpleNamespace(param=prm.detach(), exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"])
        dense = _step(x, combo)
        _assert_bits(got, _expected_bits(dense, x, torch.tensor([visible_row])), (s, visible_row))


# ------------------------------------------------------------------------------------------- 5. more than one table
def _many_plan():
    """30 parameters, each with its own R, width and mask; parameter 11 has no entry in the mapping (dense), parameter 17
    is empty.  More than 24 are not empty: two launches."""
    widths = [(), (1,), (3,), (4,), (1, 3), (15, 3)]
    plan = []
    for i in range(30):
        rows = 0 if i == 17 else 40 + 37 * i
        plan.append(SimpleNamespace(shape=(rows,) + widths[i % 6], pattern=PATTERNS[2 + i % 5], kind=KINDS[i % 3],
                                    mapped=i != 11, combo=(AF.STEPS[i % 5], AF.HYPERS[(i // 6) % 3])))
    return plan


def test_thirty_parameters_in_one_call_step_exactly_once():
    from sgn_rast import optim
    plan = _many_plan()
    assert sum(1 for q in plan if q.shape[0]) > 24
    opts, prms, vis, single = [], [], {}, []
    for g in range(5):                                           # five optimizers of six parameters, one hyper set each
        group = []
        for i in range(6 * g, 6 * g + 6):
            q = plan[i]
            empty = q.shape[0] == 0
            x = None if empty else _inputs(q.shape, seed=i)
            prm = torch.nn.Parameter(torch.zeros(q.shape, device=DEV) if empty else x.p.to(DEV).clone())
            prm.grad = torch.zeros(q.shape, device=DEV) if empty else x.g.to(DEV).clone()
            mask = _mask(q.pattern, q.shape[0])
            if q.mapped:
                vis[prm] = _encode(mask, q.kind)
            group.append(prm)
            if not empty:                                        # the same parameter in a call of its own
                single.append(_step(x, q.combo, visible=vis.get(prm)))
            else:
                single.append(None)
        lr, b1, b2, eps = plan[6 * g].combo[1]
        opt = optim.FusedAdam(group, lr=lr, betas=(b1, b2), eps=eps)
        for i, prm in zip(range(6 * g, 6 * g + 6), group):
            q = plan[i]
            x = None if q.shape[0] == 0 else _inputs(q.shape, seed=i)
            z = lambda a: torch.zeros_like(prm) if x is None else a.to(DEV).clone()
            opt.state[prm] = {"step": torch.tensor(float(q.combo[0] - 1)), "exp_avg": z(x and x.m),
                              "exp_avg_sq": z(x and x.v)}
        opts.append(opt)
        prms += group
    optim.step_many(opts, visible=vis)
    for i, (q, prm, one) in enumerate(zip(plan, prms, single)):
        st = opts[i // 6].state[prm]
        assert float(st["step"]) == q.combo[0], i
        if one is None:
            continue
        got = SimpleNamespace(param=prm.detach(), exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"])
        _assert_bits(got, {name: _bits(getattr(one, name)) for name in AF.NAMES}, (i, q.shape, q.pattern, q.kind))
        if not q.mapped:                                         # absent from the mapping: the dense step
            _assert_bits(got, {name: _bits(getattr(_step(_inputs(q.shape, seed=i), q.combo), name)) for name in AF.NAMES}, i)


# ------------------------------------------------------------------------------------------- 6. host errors
def test_a_bad_visibility_raises_before_anything_is_stepped():
    from sgn_rast import optim
    ps = [torch.nn.Parameter(torch.randn(R, 3, device=DEV)), torch.nn.Parameter(torch.randn(R, 1, device=DEV))]
    odd = torch.nn.Parameter(torch.randn(R - 1, 3, device=DEV))
    for p in ps + [odd]:
        p.grad = torch.ones_like(p)
    opts = [optim.FusedAdam([ps[0]], lr=0.01), optim.FusedAdam([ps[1], odd], lr=0.01)]
    optim.step_many(opts)                                        # a first step, so that there is a state to watch
    torch.cuda.synchronize()
    state = lambda: [(float(o.state[p]["step"]), _bits(p), _bits(o.state[p]["exp_avg"]), _bits(o.state[p]["exp_avg_sq"]))
                     for o in opts for g in o.param_groups for p in g["params"]]
    before = state()
    ok = torch.ones(R, dtype=torch.bool, device=DEV)
    cases = [
        (opts[:1], torch.ones(R + 1, dtype=torch.bool, device=DEV), ValueError),          # wrong length
        (opts[:1], torch.ones(R, device=DEV), TypeError),                                 # float32
        (opts[:1], torch.ones(R, dtype=torch.int64, device=DEV), TypeError),              # int64
        (opts[:1], torch.ones(R, dtype=torch.bool), ValueError),                          # on the CPU
        (opts[:1], torch.ones(2 * R, dtype=torch.int32, device=DEV)[::2], ValueError),    # not contiguous
        (opts, ok, ValueError),                                                           # one tensor, two row counts
        (opts, {ps[0]: ok, odd: ok}, ValueError),                                         # the last parameter's is wrong
    ]
    for which, bad, error in cases:
        with pytest.raises(error):
            optim.step_many(which, visible=bad)
        with pytest.raises(error):
            which[-1].step(visible=bad)
    torch.cuda.synchronize()
    for a, b in zip(before, state()):
        assert a[0] == b[0] == 1.0 and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


# ------------------------------------------------------------------------------------------- 7. version counters
@pytest.mark.parametrize("many", [False, True], ids=["step", "step_many"])
def test_a_visible_step_raises_the_version_counters(many):
    from sgn_rast import optim
    ps = [torch.nn.Parameter(torch.randn(n, 3, device=DEV)) for n in (10, 1400)]
    opts = [optim.FusedAdam([p], lr=0.01, eps=1e-15) for p in ps]
    vis = {p: (torch.arange(p.shape[0], device=DEV) % 2).int() for p in ps}
    for _ in range(2):                           # the first step creates the state, the second steps an existing one
        for p in ps:
            p.grad = torch.ones_like(p)
        before = [(p._version, o.state[p]["exp_avg"]._version, o.state[p]["exp_avg_sq"]._version) if o.state[p] else None
                  for p, o in zip(ps, opts)]
        if many:
            optim.step_many(opts, visible=vis)
        else:
            for o in opts:
                o.step(visible=vis)
        for p, o, b in zip(ps, opts, before):
            after = (p._version, o.state[p]["exp_avg"]._version, o.state[p]["exp_avg_sq"]._version)
            assert all(x > y for x, y in zip(after, b or (0, 0, 0))), (after, b)
    p = ps[0]                                    # autograd's own check sees the write, as after a dense step
    loss = (p * p).sum()
    p.grad = torch.ones_like(p)
    opts[0].step(visible=vis[p])
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


# ------------------------------------------------------------------------------------------- 8. in the loop
LR, G_MIN = 5e-3, 1e-6


def _preset_state(opt, params, seed):
    """Small non-zero moments (a step of 5e-3 x 1e-5 at most: far below the gradient's), so that "kept its bits" says
    something about ``exp_avg`` and ``exp_avg_sq`` too: zeros would survive a decay."""
    gen = torch.Generator().manual_seed(seed)
    for p in params:
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": (1e-12 * torch.randn(p.shape, generator=gen)).to(DEV),
                        "exp_avg_sq": ((1e-7 * torch.randn(p.shape, generator=gen)) ** 2).to(DEV)}


class _Watch:
    """Per parameter: which rows were ever visible, and which were ever DRIVEN: visible with a gradient element above
    G_MIN.  A driven row must move.  When such an element is first driven (t <= 10, exp_avg ~ 0, exp_avg_sq v <= 2e-13 from
    the preset) its update is at least LR x 0.1 |g| / sqrt((v + 1e-3 g^2) / (1 - 0.999^t)) >= LR x 0.1 |g| / sqrt(2e-10 + g^2)
    = 3.5e-5 at |g| = 1e-6, 70 ulp of the largest parameter here (|means| < 8).  A row that is visible but hidden behind
    others (the walk stops at T < 1e-4) gets a zero gradient and has every right to stay, so "seen" alone is not "moved"."""

    def __init__(self, params, opt_of):
        self.params, self.opt_of = params, opt_of
        self.start = {p: (_bits(p), _bits(opt_of[p].state[p]["exp_avg"]), _bits(opt_of[p].state[p]["exp_avg_sq"]))
                      for p in params}
        self.seen = {p: torch.zeros(p.shape[0], dtype=torch.bool) for p in params}
        self.driven = {p: torch.zeros(p.shape[0], dtype=torch.bool) for p in params}

    def record(self, p, radii):
        vis = (radii > 0).cpu()
        self.seen[p] |= vis
        if p.grad is not None:
            self.driven[p] |= vis & (p.grad.detach().abs().reshape(p.shape[0], -1).amax(dim=1) > G_MIN).cpu()

    def check(self, label):
        total_unseen = total_driven = 0
        for p in self.params:
            st = self.opt_of[p].state[p]
            now = (_bits(p), _bits(st["exp_avg"]), _bits(st["exp_avg_sq"]))
            unseen = ~self.seen[p]
            for name, a, b in zip(AF.NAMES, self.start[p], now):
                assert torch.equal(a[unseen], b[unseen]), (label, tuple(p.shape), name, "an unseen row changed")
            moved = (self.start[p][0] != now[0]).reshape(p.shape[0], -1).any(dim=1)
            assert bool(moved[self.driven[p]].all()), (label, tuple(p.shape), "a driven row did not move")
            total_unseen += int(unseen.sum())
            total_driven += int(self.driven[p].sum())
        print(f"[selective adam] {label}: rows x parameters never seen {total_unseen}, driven {total_driven}")
        return total_unseen, total_driven


def test_training_steps_leave_unseen_rows_alone():
    """Ten fused train steps over two cameras yawed apart, each followed by ``step_many(adam, visible=out.radii)``."""
    from sgn_rast import optim, scenes, step
    cams = []
    for yaw in (0.3, -0.3):
        cam, raw = scenes.make_scene("c1", seed=4, yaw=yaw, device=DEV, n_override=3000)
        cams.append(cam)
    P = step.leaf_params(raw)
    params = list(P.values())
    adam = [optim.FusedAdam([p], lr=LR, eps=1e-15) for p in params]
    opt_of = dict(zip(params, adam))
    for k, (p, o) in enumerate(zip(params, adam)):
        _preset_state(o, [p], seed=k)
    watch = _Watch(params, opt_of)
    w_img, w_a = step.loss_weights(cams[0], seed=7, device=DEV)
    losses = [[], []]
    for it in range(10):
        out = step.train_step(P, cams[it % 2], w_img, w_a, fused=True)
        assert out.radii.dtype == torch.int32
        for p in params:
            watch.record(p, out.radii)
        optim.step_many(adam, visible=out.radii)
        losses[it % 2].append(float(out.loss))
    unseen, driven = watch.check("one model")
    assert unseen > 0 and driven > 0
    assert all(float(o.state[p]["step"]) == 10.0 for p, o in opt_of.items())
    for per_cam in losses:
        assert per_cam[-1] < per_cam[0], losses


def test_scene_graph_steps_leave_each_sub_models_unseen_rows_alone():
    """The scene-graph replay (background + 3 objects): ``optim.visibility(models, out.radii_parts)`` hands each
    sub-model its slice of the projection's radii."""
    from sgn_rast import optim, scenes, step
    cam = scenes.make_camera(160, 96, 140.0)
    models, poses, idft = scenes.make_scene_graph(4000, cam, n_objects=3, object_frac=0.25, z_range=(2.0, 8.0))
    poses[1:, 11] = torch.tensor([4.0, 5.0, 6.0])               # the objects in front of the camera, one partly outside
    poses[1:, 9] = torch.tensor([-1.0, 0.2, 3.2]); poses[1:, 10] = 0.0
    cam.viewmat, cam.cam_pos = cam.viewmat.to(DEV), cam.cam_pos.to(DEV)
    poses, idft = poses.to(DEV), idft.to(DEV)
    w_img, w_a = step.loss_weights(cam, seed=7, device=DEV)
    leaves = [step.leaf_params({k: v.to(DEV) for k, v in m.items()}) for m in models]
    counts = [m["means"].shape[0] for m in leaves]
    adam = [optim.FusedAdam(list(m.values()), lr=LR, eps=1e-15) for m in leaves]
    opt_of = {p: o for m, o in zip(leaves, adam) for p in m.values()}
    for k, (m, o) in enumerate(zip(leaves, adam)):
        _preset_state(o, list(m.values()), seed=k)
    watches = [_Watch(list(m.values()), opt_of) for m in leaves]
    losses = []
    for it in range(6):
        for m in leaves:
            for p in m.values():
                p.grad = None
        out = step.render_scene_graph(leaves, poses, idft, cam)
        loss = ((out.rgb * w_img).sum() + (out.alpha * w_a).sum() + (out.object_acc * w_a).sum()) / (cam.height * cam.width)
        loss.backward()
        parts = out.radii_parts
        vis = optim.visibility(leaves, parts)
        store = parts[0].untyped_storage().data_ptr()           # slices of ONE tensor, in order, not copies
        for i, (part, m) in enumerate(zip(parts, leaves)):
            assert part.untyped_storage().data_ptr() == store and part.storage_offset() == sum(counts[:i])
            assert part.dtype == torch.int32 and part.is_contiguous()
            for p in m.values():
                assert vis[p] is part
                watches[i].record(p, part)
        optim.step_many(adam, visible=vis)
        losses.append(float(loss.detach()))
    figures = [w.check(f"sub-model {i}") for i, w in enumerate(watches)]
    assert figures[0][0] > 0 and all(d > 0 for _u, d in figures)
    assert sum(u for u, _d in figures[1:]) > 0, "no object row was out of view: the objects' half of the test is idle"
    assert losses[-1] < losses[0], losses

"""GPU: ``FusedAdam`` (csrc/optim.hip ``adam_kernel`` behind ``sgn_adam_step``) per element against one float64 step of
``torch.optim.Adam`` (tests/adam_fp64.py), and what the rest of the package needs from an optimizer step.

Floating point, per output (param, exp_avg, exp_avg_sq): ``k`` the kernel's scaled error, ``r`` that of torch's own
float32 step on the CPU from the same state, computed at run time; max k <= 4 max r + 2^-22, median and 0.99 quantile of
k <= 2 x the same quantile of r + 2^-24 (the rule of tests/test_gpu_sh_fp64.py); the same on the ``p = 0`` rows alone,
where the update itself is the output.  Steps 1 to 30000, three sets of hyper-parameters; one table of thirty tensors,
every row with its own hyper-parameters and step, carved out of arenas at every alignment, with sentinels between them;
overflowing, infinite and NaN gradients against torch's float32 step; the version counters autograd and this package's
caches rely on; and the render after a step, which must not be served the binning of the opacities before it.
Measured values: profiles/adam_fp64.md.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import adam_fp64 as AF
from helpers import small_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CASE = {}


def _case(n=AF.N, seed=0):
    if (n, seed) not in _CASE:
        _CASE[(n, seed)] = AF.make_case(n, seed)
    return _CASE[(n, seed)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------- 1. per element
@pytest.mark.parametrize("combo", AF.COMBOS, ids=AF.combo_id)
def test_one_step_per_element_against_fp64(combo):
    from sgn_rast.optim import FusedAdam
    t, hyper = combo
    c = _case()
    ref, r32 = AF.definition(c.p, c.g, c.m, c.v, hyper, t), AF.yardstick(c.p, c.g, c.m, c.v, hyper, t)
    got = AF.step_once(FusedAdam, c.p, c.g, c.m, c.v, hyper, t, device=DEV)
    S = AF.scales(c.p, c.g, c.m, c.v, hyper, t, ref)
    label = AF.combo_id(combo)
    fails, _ = AF.compare(got, r32, ref, S, None, label)
    fails += AF.compare(got, r32, ref, S, c.p0, label + " p=0 rows")[0]
    assert not fails, "\n".join(fails)
    for name, x in zip(AF.NAMES, (c.p, c.m, c.v)):
        assert torch.equal(_bits(getattr(got, name))[c.zero], _bits(x)[c.zero]), (name, "a g = m = v = 0 row moved")
    assert got.step == ref.step == t
    assert torch.equal(_bits(got.grad), _bits(c.g)), "the gradient was written"


# ------------------------------------------------------------------------------------------- 2. one table
SENTINEL = 0x7FC0DEAD                    # a quiet NaN: read as an input it poisons the row that read it
# (size, float offsets mod 4 of param / grad / exp_avg / exp_avg_sq): every size with all four 16-byte aligned, then
# only the gradient off, only the parameter off, all four off (three residues exist: two tensors share one)
_ALIGNED = [(s, (0, 0, 0, 0)) for s in (1, 3, 4, 5, 4095, 4096, 4097, 8192, 8193, 12289)]
_GRAD_OFF = [(s, (0, 1, 0, 0)) for s in (3, 5, 4095, 4096, 8193, 12289)]
_PARAM_OFF = [(s, (2, 0, 0, 0)) for s in (1, 4, 4096, 4097, 8192, 12289)]
_ALL_OFF = [(s, r) for s, r in zip((3, 4, 4095, 4097, 8192, 8193), ((1, 2, 3, 1), (3, 1, 2, 2)) * 3)]
EMPTY_AT = (7, 20)


def _table_plan():
    rows = _ALIGNED + _GRAD_OFF + _PARAM_OFF + _ALL_OFF
    order = torch.randperm(len(rows), generator=torch.Generator().manual_seed(5)).tolist()
    plan = [rows[j] for j in order]
    for at in EMPTY_AT:
        plan.insert(at, (0, (0, 0, 0, 0)))
    return plan


def _row_hyper(i):
    lr, b1, b2, eps = AF.HYPERS[i % 3]
    return (lr * (1.0 + 0.1 * i), b1 - 0.002 * i, b2 - 0.0001 * i, eps * (1.0 + i)), AF.STEPS[i % 5]


def test_one_table_of_thirty_tensors_every_row_different():
    from sgn_rast import optim
    plan = _table_plan()
    assert len(plan) == 30 and sum(1 for s, _ in plan if s) > 24          # two launches
    first_launch = [_row_hyper(i)[1] for i, (s, _) in enumerate(plan) if s][:24]
    assert 1 in first_launch and 30000 in first_launch
    # lay the tensors out: at least two sentinel words before each, then up to the wanted residue
    offs, cursor = [], [0, 0, 0, 0]
    for size, res in plan:
        o = []
        for a in range(4):
            at = cursor[a] + 2
            at += (res[a] - at) % 4
            o.append(at)
            cursor[a] = at + size
        offs.append(o)
    words = max(cursor) + 2
    cases = [_case(size, seed=i) if size else None for i, (size, _) in enumerate(plan)]
    arenas = [torch.full((words,), SENTINEL, dtype=torch.int32).view(torch.float32) for _ in range(4)]
    inside = [torch.zeros(words, dtype=torch.bool) for _ in range(4)]
    for (size, _), o, c in zip(plan, offs, cases):
        if size:
            for a, x in enumerate((c.p, c.g, c.m, c.v)):
                arenas[a][o[a]: o[a] + size] = x
                inside[a][o[a]: o[a] + size] = True
    dev = [a.to(DEV) for a in arenas]
    assert all(a.data_ptr() % 16 == 0 for a in dev)
    view = lambda a, i: dev[a][offs[i][a]: offs[i][a] + plan[i][0]]
    opts, params = [], []
    for i, (size, res) in enumerate(plan):
        (lr, b1, b2, eps), t = _row_hyper(i)
        p = torch.nn.Parameter(view(0, i))
        p.grad = view(1, i)
        assert [x.data_ptr() % 16 // 4 for x in (p, p.grad, view(2, i), view(3, i))] == list(res) or size == 0
        o = optim.FusedAdam([p], lr=lr, betas=(b1, b2), eps=eps)
        o.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": view(2, i), "exp_avg_sq": view(3, i)}
        opts.append(o)
        params.append(p)
    optim.step_many(opts)
    torch.cuda.synchronize()
    after = [a.cpu() for a in dev]
    for a in range(4):                               # every word that belongs to no tensor still holds the sentinel
        assert bool((after[a].view(torch.int32)[~inside[a]] == SENTINEL).all()), ("param", "grad", "exp_avg", "exp_avg_sq")[a]
    assert torch.equal(after[1].view(torch.int32), arenas[1].view(torch.int32)), "the gradient arena was written"
    fails = []
    for i, ((size, res), o, c) in enumerate(zip(plan, offs, cases)):
        hyper, t = _row_hyper(i)
        step = float(opts[i].state[params[i]]["step"])
        if size == 0:
            e = torch.zeros(0)
            assert step == AF.yardstick(e, e, e, e, hyper, t).step == t
            continue
        assert step == t
        ref, r32 = AF.definition(c.p, c.g, c.m, c.v, hyper, t), AF.yardstick(c.p, c.g, c.m, c.v, hyper, t)
        got = SimpleNamespace(
            param=after[0][o[0]: o[0] + size], exp_avg=after[2][o[2]: o[2] + size], exp_avg_sq=after[3][o[3]: o[3] + size])
        S = AF.scales(c.p, c.g, c.m, c.v, hyper, t, ref)
        label = f"row {i} n={size} offsets%4={res} t={t}"
        fails += AF.compare(got, r32, ref, S, None, label)[0]
        fails += AF.compare(got, r32, ref, S, c.p0, label + " p=0 rows")[0]
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------- 3. non-finite
def test_overflowing_infinite_and_nan_gradients_follow_torch_and_stay_in_their_rows():
    """Against torch's float32 step (float64 is the wrong judge of an overflow).  ``(1 - beta2) g`` times ``g``: at
    |g| = 1e20 that is 1e37, still finite, in torch as in the kernel; at 1e30 it is infinite, ``exp_avg / inf = 0`` and the
    parameter stays bit-identical.  n = 4099: the last three rows take the scalar tail of a 16-byte aligned tensor."""
    from sgn_rast.optim import FusedAdam
    n, hyper, t = 4099, AF.HYPERS[0], 25
    c = _case(n, seed=1)
    g = c.g.clone()
    values = (1e20, -1e20, 1e30, -1e30, math.inf, -math.inf, math.nan)
    rows = torch.tensor([9, 130, 1027, 2049, 3000, 4094, 4096, 4097, 4098, 5, 6, 260, 515, 777])   # 5, 6: one float4
    assert len(set(rows.tolist()) | set(torch.cat((c.zero, c.reset, c.tiny)).tolist())) == rows.numel() + 3 * AF.SPECIAL
    g[rows] = torch.tensor(values * 2)
    r32 = AF.yardstick(c.p, g, c.m, c.v, hyper, t)
    got = AF.step_once(FusedAdam, c.p, g, c.m, c.v, hyper, t, device=DEV)
    for name in AF.NAMES:
        a, b = getattr(got, name), getattr(r32, name)
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), name
    assert torch.equal(_bits(got.grad), _bits(g))
    overflow = torch.isinf(r32.exp_avg_sq) & torch.isfinite(g)
    assert overflow.nonzero()[:, 0].tolist() == sorted(rows[[2, 3, 9, 10]].tolist())               # the |g| = 1e30 rows
    assert torch.equal(_bits(got.param)[overflow], _bits(c.p)[overflow])
    assert bool(torch.isfinite(got.exp_avg[overflow]).all()) and bool(torch.isinf(got.exp_avg_sq[overflow]).all())
    assert bool(torch.isnan(got.param[rows[[4, 5, 6, 11, 12, 13]]]).all())                        # inf / inf, NaN
    ordinary = torch.isfinite(r32.exp_avg_sq) & torch.isfinite(g)                                 # the 1e20 rows included
    assert int(ordinary.sum()) == n - 10
    ref = AF.definition(c.p, g, c.m, c.v, hyper, t)
    fails, _ = AF.compare(got, r32, ref, AF.scales(c.p, g, c.m, c.v, hyper, t, ref), ordinary, "beside non-finite rows")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------- 4. version counters
def _versions(opt, p):
    st = opt.state[p]
    return p._version, st["exp_avg"]._version, st["exp_avg_sq"]._version


@pytest.mark.parametrize("many", [False, True], ids=["step", "step_many"])
def test_a_step_raises_the_version_counters_like_torch(many):
    from sgn_rast import optim
    cpu = torch.nn.Parameter(torch.randn(10))
    o_cpu = torch.optim.Adam([cpu], lr=0.01, eps=1e-15)
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (10, 4097)]
    idle = torch.nn.Parameter(torch.randn(10, device=DEV))                  # never gets a gradient
    opts = [optim.FusedAdam([ps[0], idle], lr=0.01, eps=1e-15), optim.FusedAdam([ps[1]], lr=0.01, eps=1e-15)]
    owner = {ps[0]: opts[0], ps[1]: opts[1]}
    idle_before, idle_version = idle.detach().clone(), idle._version
    for _ in range(2):                           # the first step creates the state, the second steps an existing one
        for p in [cpu] + ps:
            p.grad = torch.ones_like(p)
        torch_before = _versions(o_cpu, cpu) if o_cpu.state else None
        before = {p: (_versions(o, p) if o.state[p] else None) for p, o in owner.items()}
        data_ptrs = {p: p.data_ptr() for p in ps}
        o_cpu.step()
        if many:
            optim.step_many(opts)
        else:
            for o in opts:
                o.step()
        torch_delta = None if torch_before is None else [a - b for a, b in zip(_versions(o_cpu, cpu), torch_before)]
        for p, o in owner.items():
            assert p.data_ptr() == data_ptrs[p]
            if before[p] is None:
                continue
            delta = [a - b for a, b in zip(_versions(o, p), before[p])]
            assert all(d > 0 for d in delta), delta
            assert delta[0] == torch_delta[0], (delta, torch_delta)
    assert all(p._version > 0 for p in ps)                                  # the first step counted too
    assert idle.grad is None and idle not in opts[0].state and idle._version == idle_version
    assert torch.equal(idle.detach(), idle_before)
    # autograd's own check sees the write: a graph that saved the parameter before the step refuses to run after it
    p = ps[0]
    loss = (p * p).sum()
    p.grad = torch.ones_like(p)
    opts[0].step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


# ------------------------------------------------------------------------------------------- 5. the stale list
_SCENE = {}


def _scene():
    """1500 Gaussians projected onto 96 x 80 once (the "grad" scene of tests/test_gpu_features.py), left unchanged."""
    if not _SCENE:
        from sgn_rast import ops
        n, W, H = 1500, 96, 80
        cam, P = small_scene(n=n, w=W, h=H, focal=float(W), z_range=(1.0, 5.0))
        P = {k: v.to(DEV) for k, v in P.items()}
        with torch.no_grad():
            quats = P["quats"] / P["quats"].norm(dim=-1, keepdim=True)
            xys, depths, radii, conics, _c, nth, _cov = ops.project_gaussians(
                P["means"], P["log_scales"].exp(), 1.0, quats, cam.viewmat.to(DEV), cam.fx, cam.fy, cam.cx, cam.cy, H, W, 16)
        _SCENE.update(geo=(xys, depths, radii, conics, nth), H=H, W=W, n=n, logit_shape=P["opacity_logits"].shape,
                      rgb=torch.rand(n, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(3)))
    return _SCENE


@pytest.mark.usefixtures("library_defaults")
@pytest.mark.parametrize("surface", ["fused", "features"])
@pytest.mark.parametrize("optimizer", ["FusedAdam", "torch.optim.Adam"])
def test_the_render_after_a_step_bins_for_the_new_opacities(optimizer, surface):
    """Fixed geometry, tile culling on: the culled list depends on the opacities, and the binning cache tells "same
    opacities" by data_ptr and version counter.  Half of the Gaussians start below 1/255 and one step makes them opaque."""
    from sgn_rast import config, features, fused, ops
    from sgn_rast.optim import FusedAdam
    S = _scene()

    def render(logits):
        with torch.no_grad():
            if surface == "fused":
                return fused.rasterize_gaussians_fused(*S["geo"], S["rgb"], logits, S["H"], S["W"], 16)
            return features.rasterize_features(*S["geo"], S["rgb"], logits, S["H"], S["W"], opacity_is_logit=True)

    start = torch.full(S["logit_shape"], 2.0, device=DEV)
    start[0::2] = -7.0                                           # sigmoid(-7) = 0.0009 < 1/255: culled
    logits = torch.nn.Parameter(start.clone())
    with config.override(tile_culling=True):
        ops.clear_binning_cache()
        try:
            first = render(logits)
            logits.grad = torch.full_like(logits, -1.0)
            opt = (FusedAdam if optimizer == "FusedAdam" else torch.optim.Adam)([logits], lr=12.0, eps=1e-15)
            opt.step()                                           # a first Adam step moves every element by lr
            assert torch.allclose(logits.detach(), start + 12.0, rtol=1e-6)
            binnings = ops.binning_stats["binnings"]
            second = render(logits)
            rebinned = ops.binning_stats["binnings"] - binnings
            ops.clear_binning_cache()
            third = render(logits)
        finally:
            ops.clear_binning_cache()
    assert float((third - first).abs().max()) > 0.1              # the step is visible at all
    assert torch.equal(second, third), float((second - third).abs().max())
    assert float((second - first).abs().max()) > 0.1
    assert rebinned >= 1

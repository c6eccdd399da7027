"""GPU: the fused projection front end per Gaussian against the fp64 definition of tests/project_fp64.py —
``fused.project_gaussians_fused`` (sgn_project_fwd_fused / sgn_project_bwd_fused, with and without the pose table and
its POSE instantiation), ``ops.project_gaussians`` over proven activations (sgn_project_bwd_act, MODE 2) and
``views._ProjectViews`` (sgn_project_views_fwd / _bwd), called directly with random upstream gradients: no SH, no
rasteriser and no loss take part.

Exact: rows the reference culls are zeros in every output and gradient (a culled row whose conic or 3D covariance the
reference still writes is compared like a visible one for that tensor, and is zero everywhere else); radii and
num_tiles_hit equal the fp64 reference outside ``threshold_adjacent`` rows, whose share (of all rows, <= 2 %) is
asserted from the reference; copies give copies; two runs are bit-identical.

Floating point, per tensor and per row: ``r`` the error of a fp32 CPU restatement of the definition against fp64,
``k`` the kernel's.  (a) on well-conditioned rows (r <= 1e-5 in the restatement of the inputs as given)
``k <= 4 max_wellcond(r) + 2^-20`` — a factor 2 because two independent fp32 roundings of one chain differ by up to the
sum of their errors, another 2 for the kernel's own operation order, device expf and the 1/sqrtf normalisation; the
16 ulp floor covers the ~300-operation chain where the restatement rounds luckily; (b) on all compared rows the median
and the 0.99 quantile of k are <= 2 x the same quantile of r + 2^-22, and max k <= 4 max r.  The tolerance is taken from
the reference at run time, and every statistic of r is the largest over five restatements (``PF.restatements``): one
evaluation is one sample of a row's rounding error, and against a single one a second CPU evaluation of the same
definition already leaves (a) on a few rows (test_project_fp64.py; the kernels did too, on 1-3 rows of ``stress`` and
MODE 2, by at most 1.66x — profiles/project_fused_fp64.md).  The share of
ill-conditioned rows (of all rows) is capped as in test_project_fp64.py.

All gradient comparisons that include rows past 1.3 tan(fov/2) run under ``ops.upstream_variant(ewa_vjp_clamped=True)``
(autograd through the oracle IS the clamped vjp); the default semantics are compared on the rows inside the limits.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import project_fp64 as PF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ILL_CAP = {"regular": 0.03, "stress": 0.08, "views": 0.08}
INT_OUTPUTS = ("radii", "num_tiles_hit")


# At 4000 rows, and for the single row of n = 1 (visible and well-conditioned there), the families' own seed.  The
# other small sizes hold a few dozen visible rows, where one ill-conditioned or threshold-adjacent row more is already
# over a cap of 2 or 3 %: their seed is the first one for which the reference alone keeps the caps at every such size
# (the single row of that seed is a culled one, which is why n = 1 does not use it).
SEED, SMALL_SEED = 4, 11


@functools.lru_cache(maxsize=None)
def _family(name, n, ls_shift=0.0):
    f = getattr(PF, name)(n, seed=SEED if n >= 2000 or n == 1 else SMALL_SEED)
    f.raw["log_scales"] = f.raw["log_scales"] + ls_shift
    return f


def _world(f):
    """The family without its pose table: world-frame means and rotated quaternions (fp32, as a caller would hand them)."""
    import pose_oracle as PO
    mw, qw = PO.world_from_table(f.raw["means"], f.raw["quats"], f.ids, f.table)
    return SimpleNamespace(raw=dict(means=mw, log_scales=f.raw["log_scales"], quats=qw), ids=None, table=None,
                           cam=f.cam, dup=f.dup, n=f.n)


@functools.lru_cache(maxsize=None)
def _references(name, n, world, glob_scale, clip, block, present, ls_shift=0.0):
    """(family, upstream gradients, [(fp32 restatement, its fp64 reference)]) of one case — computed once, never
    modified.  The first pair is the inputs as given: its fp64 half is THE reference."""
    f = _family(name, n, ls_shift)
    f = _world(f) if world else f
    ups = PF.upstream(n, 11, dup=f.dup)
    ups = tuple(u if p else None for u, p in zip(ups, present))
    kw = dict(glob_scale=glob_scale, clip=clip, block=block, ups=ups)
    return f, ups, PF.restatements(f.raw, f.ids, f.table, f.cam, **kw)


def _loss(outs, ups, zeros_for_absent=False):
    loss = None
    for o, u in zip(outs, ups):
        if u is None and not zeros_for_absent:
            continue
        u = torch.zeros_like(o) if u is None else u.to(DEV)
        loss = (o * u).sum() if loss is None else loss + (o * u).sum()
    return loss


def _cpu(**kw):
    return SimpleNamespace(**{k: v.detach().cpu() for k, v in kw.items()})


def _run_fused(f, ups, glob_scale=1.0, clip=0.01, block=16, clamped=True, pose_grad=False, zeros_for_absent=False):
    from sgn_rast import fused, ops
    cam = f.cam
    leaves = [f.raw[k].to(DEV).requires_grad_(True) for k in ("means", "log_scales", "quats")]
    ids = None if f.ids is None else f.ids.to(DEV)
    table = None if f.table is None else f.table.to(DEV).requires_grad_(pose_grad)
    with ops.upstream_variant(ewa_vjp_clamped=clamped):
        xys, depths, radii, conics, comp, nth, cov3d = fused.project_gaussians_fused(
            *leaves, cam.viewmat[:3, :].to(DEV), cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, block,
            object_ids=ids, poses=table, clip_thresh=clip, glob_scale=glob_scale)
        g = torch.autograd.grad(_loss((xys, depths, conics, comp), ups, zeros_for_absent),
                                leaves + ([table] if pose_grad else []))
    torch.cuda.synchronize()
    out = _cpu(xys=xys, depths=depths, radii=radii, conics=conics, comp=comp, num_tiles_hit=nth, cov3d=cov3d,
               v_means=g[0], v_log_scales=g[1], v_quats=g[2])
    if pose_grad:
        out.v_poses = g[3].detach().cpu()
    return out


def _run_act(f, ups, split=None):
    """MODE 2: the drop-in call over exp(log-scale leaves) and x / |x|, with the graph proofs on."""
    from sgn_rast import ops
    cam = f.cam
    old = ops.activation_proofs
    ops.activation_proofs = True
    try:
        means = f.raw["means"].to(DEV).requires_grad_(True)
        x = f.raw["quats"].to(DEV).requires_grad_(True)
        ls = f.raw["log_scales"].to(DEV)
        parts = [ls.clone().requires_grad_(True)] if split is None else \
            [ls[:split].clone().requires_grad_(True), ls[split:].clone().requires_grad_(True)]
        scales = torch.exp(parts[0] if split is None else torch.cat(parts))
        before = ops.activation_proof_stats["project"]
        with ops.upstream_variant(ewa_vjp_clamped=True):
            xys, depths, radii, conics, comp, nth, cov3d = ops.project_gaussians(
                means, scales, 1.0, x / x.norm(dim=-1, keepdim=True), cam.viewmat[:3, :].to(DEV), cam.fx, cam.fy, cam.cx,
                cam.cy, cam.height, cam.width, 16)
            moved = ops.activation_proof_stats["project"] - before
            g = torch.autograd.grad(_loss((xys, depths, conics, comp), ups), [means, x] + parts)
        torch.cuda.synchronize()
    finally:
        ops.activation_proofs = old
    return _cpu(xys=xys, depths=depths, radii=radii, conics=conics, comp=comp, num_tiles_hit=nth, cov3d=cov3d,
                v_means=g[0], v_quats=g[1], v_log_scales=torch.cat(g[2:])), moved


def _run_views(f, ups):
    from sgn_rast import ops, views
    B, n = len(f.cams), f.n
    leaves = [f.raw[k].to(DEV).requires_grad_(True) for k in ("means", "log_scales", "quats")]
    with ops.upstream_variant(ewa_vjp_clamped=True):
        xys, depths, radii, conics, nth = views._ProjectViews.apply(*leaves, views.cam_table(f.cams), B, PF.H, PF.W)
        g = torch.autograd.grad(_loss((xys, depths, conics), ups[:3]), leaves)
    torch.cuda.synchronize()
    return _cpu(xys=xys, depths=depths, radii=radii, conics=conics, num_tiles_hit=nth, v_means=g[0], v_log_scales=g[1],
                v_quats=g[2])


# ------------------------------------------------------------------------------------------------- the checks
def _check_view(label, got, pairs, inter, outputs, fails, ill):
    """One camera's outputs.  Returns (rows to compare gradients on, rows whose gradient must be zero, adjacent)."""
    r64 = pairs[0][1]
    n = r64.radii.shape[0]
    adj = PF.threshold_adjacent(inter)
    assert int(adj.sum()) <= 0.02 * n, (label, "threshold-adjacent rows", int(adj.sum()), n)
    vis64 = r64.radii > 0
    for k in INT_OUTPUTS:
        diff = getattr(got, k) != getattr(r64, k)
        if bool((diff & ~adj).any()):
            fails.append(f"{label} {k}: differs from fp64 on non-adjacent rows {torch.nonzero(diff & ~adj)[:8, 0].tolist()}")
    both = vis64 & (got.radii > 0)
    for p32, p64 in pairs:
        both = both & (p32.radii > 0) & (p64.radii > 0)
    for t in outputs:
        ref, x = getattr(r64, t), getattr(got, t)
        written = ref.reshape(n, -1).abs().sum(-1) > 0
        # culled rows: zero wherever the reference is zero; a conic / 3D covariance it still writes is compared below
        must_be_zero = ~written & ~adj
        if bool((x.reshape(n, -1)[must_be_zero] != 0).any()):
            fails.append(f"{label} {t}: not zero on a row the reference culls")
        rows = written & ~vis64 & ~adj
        for p32, p64 in pairs:
            rows = rows & (getattr(p32, t).reshape(n, -1).abs().sum(-1) > 0) & (getattr(p64, t).reshape(n, -1).abs().sum(-1) > 0)
        rows = both | rows
        fl, share = PF.compare_float(t, x, [(getattr(p32, t), getattr(p64, t)) for p32, p64 in pairs], rows, label)
        fails += [f"{label} {m}" for m in fl]
        ill[t] = ill.get(t, 0) + share * int(rows.sum())
    return both, ~vis64 & ~adj, adj


def _check_grads(label, got, pairs, rows, zero_rows, fails, ill):
    for t in PF.GRADS:
        x = getattr(got, t)
        if bool((x[zero_rows] != 0).any()):
            fails.append(f"{label} {t}: not zero on a row the reference culls")
        fl, share = PF.compare_float(t, x, [(getattr(p32, t), getattr(p64, t)) for p32, p64 in pairs], rows, label)
        fails += [f"{label} {m}" for m in fl]
        ill[t] = share * int(rows.sum())


def _check_single(label, family, got, pairs, grad_rows=None, outputs=PF.OUTPUTS):
    fails, ill = [], {}
    r64 = pairs[0][1]
    n = r64.radii.shape[0]
    both, culled, _adj = _check_view(label, got, pairs, r64.inter, outputs, fails, ill)
    rows = both if grad_rows is None else both & grad_rows
    _check_grads(label, got, pairs, rows, culled, fails, ill)
    for t, cnt in ill.items():
        assert cnt <= ILL_CAP[family] * n, (label, t, "ill-conditioned rows", cnt, n)
    return fails


def _assert_same(a, b, names, what):
    for t in names:
        assert torch.equal(getattr(a, t), getattr(b, t)), (what, t)


ALL = PF.OUTPUTS + PF.GRADS + INT_OUTPUTS

# name: (family, n, keyword deviations).  The defaults plus each deviation alone.
CASES = {f"n{n}": ("regular", n, {}) for n in (1, 63, 64, 65, 255, 256, 257, 4000)}
CASES.update({
    "stress": ("stress", 4000, {}),
    "glob_scale_0.37": ("regular", 4000, dict(glob_scale=0.37)),
    # (log-scales shifted by -log 2.5: the splats, and with them the conditioning, stay the family's — 2.5 times larger
    # ones are round and large on a tenth of the rows, where every fp32 evaluation of the compensation gradient cancels)
    "glob_scale_2.5": ("regular", 4000, dict(glob_scale=2.5, ls_shift=-math.log(2.5))),
    "clip_1.0": ("regular", 4000, dict(clip=1.0)),
    "block_5": ("regular", 4000, dict(block=5)),
    "no_table": ("regular", 4000, dict(world=True)),
    "no_v_depths": ("regular", 4000, dict(present=(True, False, True, True))),
    "no_v_comp": ("regular", 4000, dict(present=(True, True, True, False))),
    "v_conics_only": ("regular", 4000, dict(present=(False, False, True, False))),
})


@pytest.mark.parametrize("case", list(CASES))
def test_fused_projection_per_row_against_fp64(case):
    family, n, dev = CASES[case]
    dev = dict(dev)
    world, present, ls_shift = dev.pop("world", False), dev.pop("present", (True,) * 4), dev.pop("ls_shift", 0.0)
    key = (dev.get("glob_scale", 1.0), dev.get("clip", 0.01), dev.get("block", 16))
    f, ups, pairs = _references(family, n, world, *key, present, ls_shift)
    got = _run_fused(f, ups, **dev)
    fails = _check_single(case, family, got, pairs)
    if f.dup.numel() and n == 4000:
        for t in ALL:
            assert torch.equal(getattr(got, t)[f.dup[:, 0]], getattr(got, t)[f.dup[:, 1]]), (case, t, "copies")
    if not all(present):
        # an absent upstream gradient is the call with explicit zeros, bit for bit
        _assert_same(got, _run_fused(f, ups, zeros_for_absent=True, **dev), ALL, case + ": absent vs zeros")
    if case in ("n4000", "n65"):
        _assert_same(got, _run_fused(f, ups, **dev), ALL, case + ": two runs")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", [65, 257, 4000])
def test_pose_instantiation_returns_the_same_per_gaussian_gradients(n):
    f, ups, pairs = _references("regular", n, False, 1.0, 0.01, 16, (True,) * 4)
    plain = _run_fused(f, ups)
    posed = _run_fused(f, ups, pose_grad=True)
    _assert_same(plain, posed, ALL, "POSE")
    assert posed.v_poses.shape == (f.table.shape[0], 16) and bool(torch.isfinite(posed.v_poses).all())
    assert torch.equal(posed.v_poses[2], torch.zeros(16))                  # the table row that owns no Gaussian
    fails = _check_single(f"pose_grad n{n}", "regular", posed, pairs)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", ["regular", "stress"])
def test_default_semantics_on_the_rows_inside_the_limits(family):
    f, ups, pairs = _references(family, 4000, False, 1.0, 0.01, 16, (True,) * 4)
    r64 = pairs[0][1]
    got = _run_fused(f, ups, clamped=False)
    inside = PF.inside_limits(r64.inter)
    assert int((~inside & (r64.radii > 0)).sum()) >= 100                   # there ARE visible rows past the limits
    fails = _check_single(f"default semantics {family}", family, got, pairs, grad_rows=inside)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("split", [None, 65], ids=["one model", "two sub-models split at row 65"])
def test_mode2_proven_activations_against_fp64(split):
    f, ups, pairs = _references("regular", 4000, True, 1.0, 0.01, 16, (True,) * 4)
    got, moved = _run_act(f, ups, split=split)
    assert moved == 1, "the graph proof did not take the call"
    fails = _check_single(f"MODE 2 split={split}", "regular", got, pairs)
    assert not fails, "\n".join(fails)


@functools.lru_cache(maxsize=None)
def _views_references(n, B):
    f = PF.views(n, B)
    ups = PF.upstream(n, 13, B=B)[:3] + (None,)
    return f, ups, PF.restatements(f.raw, None, None, f.cams, ups=ups)


def _view_of(r, b, n):
    return SimpleNamespace(**{k: getattr(r, k).reshape(-1, n, *getattr(r, k).shape[2:])[b]
                              for k in ("xys", "depths", "conics", "radii", "num_tiles_hit") if hasattr(r, k)})


@pytest.mark.parametrize("n", [65, 2000])
@pytest.mark.parametrize("B", [1, 2, 16])
def test_views_per_row_against_fp64(B, n):
    f, ups, pairs = _views_references(n, B)
    r64 = pairs[0][1]
    got = _run_views(f, ups)
    label = f"views B={B} n={n}"
    fails, ill = [], {}
    rows, adj_any, seen64 = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    agree = torch.ones(n, dtype=torch.bool)
    for b in range(B):
        g_b, pairs_b = _view_of(got, b, n), [(_view_of(p32, b, n), _view_of(p64, b, n)) for p32, p64 in pairs]
        both, _culled, adj = _check_view(f"{label} view {b}", g_b, pairs_b, r64.inter[b], ("xys", "depths", "conics"),
                                         fails, ill)
        v64 = pairs_b[0][1].radii > 0
        agree &= (g_b.radii > 0) == v64
        for p32_b, p64_b in pairs_b:
            agree &= ((p32_b.radii > 0) == v64) & ((p64_b.radii > 0) == v64)
        rows |= both
        seen64 |= v64
        adj_any |= adj
    # a gradient is a sum over the views: compared where kernel, restatements and reference agree on WHICH views see the row
    _check_grads(label, got, pairs, rows & agree, ~seen64 & ~adj_any, fails, ill)
    assert not bool((~agree & ~adj_any).any()), label
    for t, cnt in ill.items():
        assert cnt <= ILL_CAP["views"] * n * (B if t in PF.OUTPUTS else 1), (label, t, "ill-conditioned rows", cnt)
    if B == 1:
        # one view IS the single-view fused call: forward and backward bit for bit, on the same upstream gradients
        single = SimpleNamespace(raw=f.raw, ids=None, table=None, cam=f.cams[0], n=n)
        one = _run_fused(single, tuple(None if u is None else u[0] for u in ups))
        names = ("xys", "depths", "conics", "radii", "num_tiles_hit")
        _assert_same(_view_of(got, 0, n), one, names, "B = 1 forward vs project_gaussians_fused")
        _assert_same(got, one, PF.GRADS, "B = 1 backward vs project_gaussians_fused")
        print(f"[project fp64] {label}: bit-equal to project_gaussians_fused, forward and backward")
    if B == 16:
        from sgn_rast import _lib
        assert B == _lib.VIEWS_MAX
    assert not fails, "\n".join(fails)

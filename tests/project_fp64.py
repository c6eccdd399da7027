"""The fused projection front end written out as a definition, and the per-row statistics its tests use (CPU, torch).

``reference``: world means / quaternions from the pose table (``pose_oracle.world_from_table``), ``qn = qw / |qw|``,
``scales = exp(log_scales)``, then ``oracle.torch_oracle.project_gaussians`` — all in the requested dtype — and the
gradients of ``L = sum_vis (v_xys.xys + v_depths depths + v_conics.conics + v_comp comp)`` by autograd, ``vis`` the rows
whose reference radius is > 0 (the convention of ``pose_oracle.table_vjp``).  fp64 is the definition; the same function
in fp32 is the "CPU restatement" whose own distance to fp64 sets the tolerances of the GPU test at run time.

Two semantics.  Autograd through the oracle differentiates through the forward's +-1.3 tan(fov/2) clamp: it IS the
*clamped* EWA vjp (``ops.upstream_variant(ewa_vjp_clamped=True)``).  Under the default semantics (upstream CUDA's vjp
of the un-clamped point) only rows inside the limits may be compared — ``inside_limits``.  The clamped rows of the
default vjp are held per row on the plain kernel by ``test_gpu_adversarial_geometry.py``; the fused chain rules (exp,
normalisation, Hamilton product, rigid transform) are row-local and do not read the semantics bit, so the un-clamped
analytic vjp is not restated here.

The compensation gradient: upstream's vjp (restated by the kernel) divides by ``comp + 1e-6`` where the true derivative
of ``sqrt`` divides by ``comp``.  ``compensation`` puts that into the definition instead of into a tolerance.
"""
import math
from types import SimpleNamespace

import torch

import pose_oracle as PO
from oracle import torch_oracle as TO
from sgn_rast import scenes

W, H, FOCAL = 160, 96, 140.0
OUTPUTS = ("xys", "depths", "conics", "comp", "cov3d")
GRADS = ("v_means", "v_log_scales", "v_quats")


# ---------------------------------------------------------------------------------------------- the definition
class _CompVjp(torch.autograd.Function):
    """Identity on ``comp``; the backward multiplies by ``comp / (comp + 1e-6)``."""
    @staticmethod
    def forward(ctx, comp):
        ctx.save_for_backward(comp)
        return comp.clone()

    @staticmethod
    def backward(ctx, g):
        comp, = ctx.saved_tensors
        return g * comp / (comp + 1e-6)


def compensation(det0, det):
    """``sqrt(clamp(det0 / det, 0))`` whose backward is the true derivative times ``comp / (comp + 1e-6)``: upstream's
    ``v_sqr_comp = v_comp * 0.5 / (comp + 1e-6)``."""
    return _CompVjp.apply(torch.sqrt(torch.clamp(det0 / det, min=0.0)))


def _cam_list(cams):
    single = not isinstance(cams, (list, tuple))
    return ([cams] if single else list(cams)), single


def reference(raw, ids, table, cams, glob_scale=1.0, clip=0.01, block=16, ups=None, dtype=torch.float64):
    """The seven outputs, the three leaf gradients (when ``ups`` is given) and the fp64 intermediates that
    ``threshold_adjacent`` reads.  ``raw``: dict with ``means`` (local), ``log_scales``, ``quats`` (raw); ``ids`` /
    ``table``: the pose table or None; ``cams``: one camera, or a list (outputs stacked [B, n, ...], L summed over the
    views); ``ups``: (v_xys, v_depths, v_conics, v_comp), each a tensor shaped like its output or None."""
    cam_l, single = _cam_list(cams)
    m, ls, q = (raw[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in ("means", "log_scales", "quats"))
    if ids is None:
        mw, qw = m, q
    else:
        mw, qw = PO.world_from_table(m, q, ids.cpu(), table.detach().cpu().to(dtype))
    qn = qw / qw.norm(dim=-1, keepdim=True)
    sc = ls.exp()
    per_view, loss = [], None
    for b, cam in enumerate(cam_l):
        V = cam.viewmat.detach().cpu().to(dtype)[:3, :]
        xys, depths, radii, conics, comp, nth, cov3d = TO.project_gaussians(
            mw, sc, glob_scale, qn, V, cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, block, clip_thresh=clip)
        comp = _CompVjp.apply(comp)
        o = SimpleNamespace(xys=xys, depths=depths, radii=radii, conics=conics, comp=comp, num_tiles_hit=nth,
                            cov3d=cov3d)
        if ups is not None:
            vis = (radii > 0).to(dtype)
            for u, t in zip(ups, (xys, depths, conics, comp)):
                if u is None:
                    continue
                u = u.detach().cpu().to(dtype)
                u = u if single else u[b]
                term = u * t
                term = (term.sum(-1) if term.dim() == 2 else term) * vis
                loss = term.sum() if loss is None else loss + term.sum()
        with torch.no_grad():
            o.inter = _intermediates(mw, V, cam, o, clip, block)
        per_view.append(o)
    out = SimpleNamespace()
    for k in ("xys", "depths", "radii", "conics", "comp", "num_tiles_hit", "cov3d"):
        vals = [getattr(o, k).detach() for o in per_view]
        setattr(out, k, vals[0] if single else torch.stack(vals))
    out.inter = per_view[0].inter if single else [o.inter for o in per_view]
    if ups is not None:
        zeros = lambda t: torch.zeros_like(t).detach()
        if loss is None or not loss.requires_grad:
            g = (zeros(m), zeros(ls), zeros(q))
        else:
            g = torch.autograd.grad(loss, (m, ls, q), allow_unused=True)
            g = tuple(zeros(t) if x is None else x for x, t in zip(g, (m, ls, q)))
        out.v_means, out.v_log_scales, out.v_quats = g
    return out


def _intermediates(mw, V, cam, o, clip, block):
    """What the integer outputs were decided from, recomputed from the reference's own fp64 values."""
    pv = mw @ V[:, :3].T + V[:, 3]
    X0, X1, X2 = o.conics.unbind(-1)
    dc = X0 * X2 - X1 * X1                     # = 1 / det
    written = dc != 0
    det = torch.where(written, 1.0 / torch.where(written, dc, torch.ones_like(dc)), torch.zeros_like(dc))
    a, c = X2 * det, X0 * det
    mid = 0.5 * (a + c)
    sq = torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    rw = 1.0 / (pv[:, 2] + 1e-6)
    lim_x, lim_y = 1.3 * 0.5 * cam.width / cam.fx, 1.3 * 0.5 * cam.height / cam.fy
    return SimpleNamespace(
        pvz=pv[:, 2], radius_f=3.0 * torch.sqrt(torch.maximum(mid + sq, mid - sq)), conic_written=written,
        ux=pv[:, 0] * rw * cam.fx + cam.cx, uy=pv[:, 1] * rw * cam.fy + cam.cy, clip=clip, block=block,
        tiles_x=(cam.width + block - 1) // block, tiles_y=(cam.height + block - 1) // block,
        qx=(pv[:, 0] / pv[:, 2]).abs() / lim_x, qy=(pv[:, 1] / pv[:, 2]).abs() / lim_y)


def inside_limits(inter):
    """Rows whose fp64 |pvx/pvz|, |pvy/pvz| lie below 1.3 tan(fov/2) by a relative 1e-6: the rows on which the default
    (un-clamped) vjp and autograd through the oracle are the same function."""
    return (inter.qx < 1.0 - 1e-6) & (inter.qy < 1.0 - 1e-6)


def frustum_clamped(inter):
    return (inter.pvz > inter.clip) & ((inter.qx > 1.0) | (inter.qy > 1.0))


# ---------------------------------------------------------------------------------------------- the statistics
def row_error(x, ref64, vis):
    """[n] per-row ``|x_i - ref_i|_2 / |ref_i|_2`` on the rows ``vis`` (0 elsewhere); a row whose reference norm is 0
    is compared for exact equality: 0 if equal, inf if not."""
    x = x.detach().cpu().double().reshape(x.shape[0], -1)
    r = ref64.detach().cpu().double().reshape(x.shape[0], -1)
    num, den = (x - r).norm(dim=-1), r.norm(dim=-1)
    e = torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)),
                    torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)))
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    return torch.where(vis, e, torch.zeros_like(e))


def _near_integer(v, tol):
    return (v - torch.round(v)).abs() < tol


def threshold_adjacent(inter, tol=1e-3):
    """bool [n], from the fp64 reference alone: the rows whose integer outputs were decided within ``tol`` of a
    threshold — ``3 sqrt(lambda_max)`` next to an integer (the ceil), one of the four ``(c -+ r) / block`` next to an
    integer (the truncation; the clamp bounds 0 and tiles are integers too, and ``+ 1`` on the max side keeps the
    distance) while it lies where the clamp to [0, tiles] can still pass it on, ``pvz`` within a relative 1e-5 of the
    clip plane, or ``det`` 0.  Only these rows may differ in radii / num_tiles_hit or in being culled."""
    front = inter.pvz > inter.clip
    adj = (inter.pvz - inter.clip).abs() <= 1e-5 * abs(inter.clip)
    adj |= front & ~inter.conic_written                                   # det == 0 (or not finite)
    adj |= front & ~torch.isfinite(inter.radius_f)
    rad = torch.where(torch.isfinite(inter.radius_f), inter.radius_f, torch.zeros_like(inter.radius_f))
    adj |= front & _near_integer(rad, tol)
    r = torch.ceil(rad)
    fb = float(inter.block)
    for c, tiles in ((inter.ux, inter.tiles_x), (inter.uy, inter.tiles_y)):
        for v in ((c - r) / fb, (c + r) / fb):
            adj |= front & _near_integer(v, tol) & (v > -2.0) & (v < tiles + 1.0)
    return adj


# ---------------------------------------------------------------------------------------------- input families
def camera():
    return scenes.make_camera(W, H, FOCAL)


def _rot(yaw, pitch):
    Ry = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]])
    return (Ry @ Rx).float()


# table rows: kind (identity / posed / posed with q_o2w * 1.7), pose.  Row 2 owns no Gaussian.  Row 5 sits near the
# camera and to the side (frustum-clamped rows), row 7 astride the clip plane (most of its rows are culled behind it).
KINDS = ("identity", "posed", "posed", "scaled", "identity", "posed", "scaled", "posed")
_POSES = {1: (0.7, -0.3, (0.2, 0.05, 1.1)), 2: (1.1, 0.2, (0.0, 0.0, 3.0)), 3: (-0.5, 0.4, (-0.6, 0.2, 2.4)),
          5: (2.3, -0.6, (0.8, -0.1, 1.5)), 6: (-1.4, 0.1, (0.3, 0.3, 3.2)), 7: (0.4, 0.3, (-0.2, 0.1, -0.5))}


def layout(n):
    """Rows per table row: boundaries at 37, 38, 38 (row 2 is empty) and 338 — segments start mid-wave, as in the
    pose test's ``eight_objects`` — then the rest as 1/2 identity, 1/4 posed, 1/8 scaled, 1/8 astride the clip plane."""
    rest = max(0, n - 338)
    bounds = [0, 37, 38, 38, 338, 338 + rest // 2, 338 + (3 * rest) // 4, 338 + (7 * rest) // 8, max(n, 338)]
    bounds = [min(b, n) for b in bounds]
    return [b - a for a, b in zip(bounds[:-1], bounds[1:])]


def pose_table():
    from sgn_rast import fused
    Rs, ts = [], []
    for k in range(len(KINDS)):
        yaw, pitch, t = _POSES.get(k, (0.0, 0.0, (0.0, 0.0, 0.0)))
        Rs.append(_rot(yaw, pitch))
        ts.append(torch.tensor(t))
    table = fused.make_pose_table(torch.stack(Rs), torch.stack(ts))
    for k, kind in enumerate(KINDS):
        if kind == "scaled":
            table[k, 12:16] *= 1.7
    return table


def _gaussians(n, seed, ls_noise):
    cam = camera()
    g = torch.Generator().manual_seed(seed + 1000)
    raw = scenes.make_gaussians(n, cam, seed=seed, z_range=(0.05, 8.0))
    means = raw["means"].clone()
    # the stretched quarter: every row nearer than 1.5 (18 % of the rows; times 4 they lie beside the camera, or reach the
    # image as frustum-clamped rows) and a random 8 % of the others.  Near rows in the middle of the image are large
    # and round: their compensation is 1 - tiny and every fp32 evaluation of its gradient cancels, the restatement's too
    near = means[:, 2] < 1.5
    stretch = near | (torch.rand(n, generator=g) < 0.08)
    means[stretch, :2] *= 4.0
    quats = raw["quats"] * (10.0 ** (torch.rand(n, 1, generator=g) * 6.0 - 3.0))
    log_scales = raw["log_scales"] + ls_noise * torch.randn(n, 3, generator=g)
    return dict(means=means, log_scales=log_scales, quats=quats), g


def _family(n, seed, ls_noise, copies):
    raw, g = _gaussians(n, seed, ls_noise)
    counts = layout(n)
    ids = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts))
    local = torch.tensor([KINDS[int(k)] != "identity" for k in ids])
    raw["means"][local] = 0.6 * torch.randn(int(local.sum()), 3, generator=g)
    dup = torch.zeros(0, 2, dtype=torch.int64)
    if copies:
        # exact copies inside one segment (same table row): the first rows of the segment again at its end
        offs = [0] + torch.cumsum(torch.tensor(counts), 0).tolist()
        pairs = []
        for seg in (4, 6):
            lo, hi = offs[seg], offs[seg + 1]
            assert hi - lo >= copies
            pairs += [(lo + k, hi - 1 - k) for k in range(copies // 2)]
        dup = torch.tensor(pairs)
        for key in raw:
            raw[key][dup[:, 1]] = raw[key][dup[:, 0]]
    return SimpleNamespace(raw=raw, ids=ids, table=pose_table(), cam=camera(), counts=counts, dup=dup, n=n)


def regular(n, seed=4):
    return _family(n, seed, 0.5, 0)


def stress(n, seed=4):
    return _family(n, seed, 1.0, 32)


def view_cam(yaw=0.0, t=(0.0, 0.0, 0.0)):
    """A yawed camera whose centre sits at ``t`` (world -> camera: R^T (x - t)), as test_gpu_views._cam."""
    c = scenes.make_camera(W, H, FOCAL, yaw=yaw)
    tt = torch.tensor(t, dtype=torch.float32)
    c.viewmat[:3, 3] = -(c.viewmat[:3, :3] @ tt)
    c.cam_pos = tt.clone()
    return c


def views(n, B, seed=4):
    """No pose table; B cameras: camera 1 is yawed and translated (B = 2 already has rows that both views see, and rows
    that one of them sees), camera 2 looks away (sees nothing), camera 3 is camera 0 again, the others are yawed and
    translated so that rows drop out of some views only."""
    raw, _g = _gaussians(n, seed, 0.5)
    cams = []
    for b in range(B):
        if b == 0 or b == 3:
            cams.append(view_cam())
        elif b == 2:
            cams.append(view_cam(yaw=math.pi))
        else:
            y = 0.12 * max(1, b - 2) * (-1) ** b
            cams.append(view_cam(yaw=y, t=(0.3 * y, 0.02 * b, 0.5 * abs(y))))
    return SimpleNamespace(raw=raw, ids=None, table=None, cams=cams, n=n, dup=torch.zeros(0, 2, dtype=torch.int64))


def upstream(n, seed, B=None, dup=None):
    """Random upstream gradients (v_xys, v_depths, v_conics, v_comp) from a seeded generator; the rows ``dup[:, 1]``
    (a family's copies) get the gradients of the rows ``dup[:, 0]`` they are copies of."""
    g = torch.Generator().manual_seed(seed)
    lead = (n,) if B is None else (B, n)
    ups = (torch.randn(*lead, 2, generator=g), torch.randn(*lead, generator=g), torch.randn(*lead, 3, generator=g),
           torch.randn(*lead, generator=g))
    if dup is not None and dup.numel():
        dim = 0 if B is None else 1
        for u in ups:
            u.index_copy_(dim, dup[:, 1], u.index_select(dim, dup[:, 0]))
    return ups


# ---------------------------------------------------------------------------------------------- the comparison
# The fp32 CPU restatements whose own errors set the tolerances.  One evaluation is ONE sample of a row's rounding
# error: a row whose error has scale 3e-5 lands below 1e-5 in one evaluation out of three and draws 6e-5 in the next, so
# the largest error a single restatement shows on its well-conditioned rows under-states what a second evaluation of
# the same definition shows there (test_project_fp64.py measures it: up to 4.5 times the cap, on one to four rows of
# 4000).  The same Gaussians with the raw quaternions times a constant are the same definition — the normalisation
# removes the factor — and round differently from the first operation on: each is another sample.
QUAT_SCALES = (3.0, 5.0, 7.0, 1.0 / 3.0)


def restatements(raw, ids, table, cams, scales=QUAT_SCALES, **kw):
    """[(fp32 restatement, its fp64 reference)]: the inputs as given first, then one pair per quaternion scale."""
    pairs = []
    for sc in (1.0,) + tuple(scales):
        raw_s = raw if sc == 1.0 else dict(raw, quats=raw["quats"] * sc)
        pairs.append((reference(raw_s, ids, table, cams, dtype=torch.float32, **kw),
                      reference(raw_s, ids, table, cams, **kw)))
    return pairs


def compare_float(name, x, pairs, rows, label=""):
    """The floating-point part of the GPU test for one tensor.  ``pairs``: [(fp32 restatement's tensor, its fp64
    reference's)], the inputs as given first; ``k`` is the per-row error of ``x`` against the first fp64 tensor on
    ``rows``, ``r_s`` each restatement's against its own.  Well-conditioned rows are those with ``r_0 <= 1e-5``; every
    statistic of ``r`` a bound refers to is the largest one over the restatements.  Prints the three ratios k / r_0
    and the worst well-conditioned row; returns the violated bounds (empty: all hold) and the share of
    ill-conditioned rows among ``rows``."""
    k = row_error(x, pairs[0][1], rows)[rows]
    rs = [row_error(a, b, rows)[rows] for a, b in pairs]
    r = rs[0]
    if k.numel() == 0:
        return [], 0.0
    well = r <= 1e-5
    ill_share = 1.0 - float(well.double().mean())
    fails = []
    q = lambda t, p: float(torch.quantile(t, p))
    stat = {"median": lambda t: q(t, 0.5), "p99": lambda t: q(t, 0.99), "max": lambda t: float(t.max())}
    stats = {key: (fn(k), fn(r), max(fn(t) for t in rs)) for key, fn in stat.items()}
    ratio = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else math.inf)
    worst_i, worst_k, cap_a = -1, 0.0, 0.0
    if bool(well.any()):
        cap_a = 4.0 * max(float(t[well].max()) for t in rs) + 2.0 ** -20
        kw = torch.where(well, k, torch.zeros_like(k))
        worst_k = float(kw.max())
        index = torch.nonzero(rows)[:, 0]
        worst_i = int(index[int(kw.argmax())])
        if worst_k > cap_a:
            bad = index[kw > cap_a]
            fails.append(f"(a) {name}: {int(bad.numel())} well-conditioned rows above {cap_a:.3e}, worst row "
                         f"{worst_i} k={worst_k:.3e}; rows {bad[:8].tolist()}")
    for key in ("median", "p99"):
        if stats[key][0] > 2.0 * stats[key][2] + 2.0 ** -22:
            fails.append(f"(b) {name}: {key} k={stats[key][0]:.3e} > 2 * {stats[key][2]:.3e} + 2^-22")
    if stats["max"][0] > 4.0 * stats["max"][2]:
        fails.append(f"(b) {name}: max k={stats['max'][0]:.3e} > 4 * max r={stats['max'][2]:.3e}")
    print(f"[project fp64] {label} {name}: rows {int(k.numel())} k/r median {ratio(*stats['median'][:2]):.2f} "
          f"({stats['median'][0]:.2e}/{stats['median'][1]:.2e}) p99 {ratio(*stats['p99'][:2]):.2f} "
          f"({stats['p99'][0]:.2e}/{stats['p99'][1]:.2e}) max {ratio(*stats['max'][:2]):.2f} "
          f"({stats['max'][0]:.2e}/{stats['max'][1]:.2e}); ill-conditioned {100 * ill_share:.2f} %; worst "
          f"well-conditioned row {worst_i} k={worst_k:.2e} (cap {cap_a:.2e})")
    return fails, ill_share

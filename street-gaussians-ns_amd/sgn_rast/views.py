"""Batched views: B cameras of one image size rendered from one set of Gaussians in one fused launch sequence.

:func:`render_views` is :func:`sgn_rast.step.render_fused` for a list of cameras at once.  Logically the batch has
B x N rows — row ``b*N + i`` is Gaussian i seen from camera b — and every output of view b is bit-identical to
``render_fused(P, cams[b])``: the same kernel bodies run on local pixel coordinates.  The launch sequence pays the
latency-bound binning chain once per batch, reads each Gaussian's parameters once for all views (projection, SH) and
waits on the host once (the intersection count).  Gradients of the raw leaves are the sums over the views of the
single-view gradients; the projection, SH and opacity parts are summed in registers in a fixed view order (no float
atomics), the raster backward keeps its atomics.

This is new API beside the gsplat 0.1.x drop-in surface (:mod:`sgn_rast.ops`) and the single-view fused path
(:mod:`sgn_rast.fused`): neither is touched, and the batched path keeps its own state (capacities, launch-order
scratch), so it never serves or evicts a single-view binning.  Scene-graph inputs (object ids, pose tables, Fourier DC,
group accumulations, id ranges) are not supported here.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import torch
from torch.autograd import Function

from . import _lib as L
from . import ops as _ops
from .ops import _f32c, _i32c
from .scenes import Camera

BLOCK = 16
_E_CAPACITY = -100          # SGN_E_CAPACITY
_SPEC_MARGIN = 1.3


class _State:
    """Per-device state of the batched path (never shared with ops' single-view caches)."""

    def __init__(self):
        self.last_count: Dict[tuple, int] = {}       # (B, N, H, W) -> recent intersection count (capacity sizing)
        self.order_scratch: Dict[int, torch.Tensor] = {}
        self.pinned: Optional[torch.Tensor] = None


_STATES: Dict[str, _State] = {}
stats = {"forwards": 0, "capacity_misses": 0, "backwards": 0}


def _state(dev) -> _State:
    key = str(dev)
    if key not in _STATES:
        _STATES[key] = _State()
    return _STATES[key]


def _order_scratch(S: _State, lib, n_tiles: int, dev) -> torch.Tensor:
    t = S.order_scratch.get(n_tiles)
    if t is None:
        if len(S.order_scratch) > 8:
            S.order_scratch.clear()
        t = S.order_scratch[n_tiles] = torch.zeros(int(lib.sgn_tile_order_scratch_bytes(n_tiles)) // 4,
                                                   dtype=torch.int32, device=dev)
    return t


def check_views(P: Dict[str, torch.Tensor], cams: Sequence[Camera], block_width: int = BLOCK, **scene_graph) -> tuple:
    """Host-side validation of a batched call, before anything launches: ``ValueError`` for a bad batch,
    ``NotImplementedError`` for scene-graph inputs.  Returns (B, N, H, W)."""
    used = sorted(k for k, v in scene_graph.items() if v is not None)
    if used:
        raise NotImplementedError(f"render_views does not take scene-graph inputs ({', '.join(used)}); "
                                  "render each view with step.render_fused")
    if block_width != BLOCK:
        raise ValueError(f"render_views needs block_width 16 (got {block_width})")
    cams = list(cams)
    b = len(cams)
    if not 1 <= b <= L.VIEWS_MAX:
        raise ValueError(f"render_views takes 1 to {L.VIEWS_MAX} cameras (got {b})")
    h, w = int(cams[0].height), int(cams[0].width)
    for c in cams[1:]:
        if (int(c.height), int(c.width)) != (h, w):
            raise ValueError(f"all cameras of a batch share one image size: {h}x{w} vs {int(c.height)}x{int(c.width)}")
    if h < 1 or w < 1:
        raise ValueError(f"bad image size {h}x{w}")
    n = int(P["means"].shape[0])
    if n < 1:
        raise ValueError("render_views needs at least one Gaussian")
    if b * n >= (1 << 28):
        raise ValueError(f"B*N = {b}*{n} must stay below 2^28 (sorted ids carry quadrant masks in bits 28-31)")
    if P["features_dc"].dim() != 3 or P["features_dc"].shape[1] != 1:
        raise ValueError("features_dc must be [N,1,3] (no Fourier DC on the batched path)")
    return b, n, h, w


def cam_table(cams: Sequence[Camera]):
    """The host array of ``sgn_view_cam`` rows (float32 values, exactly what the single-view calls read)."""
    arr = (L.ViewCam * len(cams))()
    for b, c in enumerate(cams):
        vm = c.viewmat.detach().to("cpu", torch.float32).reshape(-1, 4)[:3, :].reshape(-1).tolist()
        pos = c.cam_pos.detach().to("cpu", torch.float32).reshape(-1)[:3].tolist()
        arr[b].viewmat[:] = vm
        arr[b].cam_pos[:] = pos
        # (the single-view calls pass fx..cy as Python floats through a c_float: same rounding here)
        arr[b].fx, arr[b].fy, arr[b].cx, arr[b].cy = float(c.fx), float(c.fy), float(c.cx), float(c.cy)
    return arr


class _ProjectViews(Function):
    @staticmethod
    def forward(ctx, means, log_scales, quats, table, b, h, w):
        dev = L.require_device(means, log_scales, quats)
        n = means.shape[0]
        means_c, ls_c, q_c = _f32c(means), _f32c(log_scales), _f32c(quats)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        r = b * n
        cov3d, xys, depths = torch.empty(r, 6, **f32), torch.empty(r, 2, **f32), torch.empty(r, **f32)
        radii, conics, comp, nth = torch.empty(r, **i32), torch.empty(r, 3, **f32), torch.empty(r, **f32), torch.empty(r, **i32)
        sem = _ops.semantics().flags()
        L.check(L.load().sgn_project_views_fwd(b, n, table, L.ptr(means_c), L.ptr(ls_c), 1.0, L.ptr(q_c), h, w, BLOCK,
                                               0.01, L.ptr(cov3d), L.ptr(xys), L.ptr(depths), L.ptr(radii),
                                               L.ptr(conics), L.ptr(comp), L.ptr(nth), sem, L.stream_ptr()),
                "sgn_project_views_fwd")
        ctx.meta = (table, b, h, w, sem)
        ctx.save_for_backward(means_c, ls_c, q_c, cov3d, radii, conics, comp)
        outs = (xys.view(b, n, 2), depths.view(b, n), radii.view(b, n), conics.view(b, n, 3), nth.view(b, n))
        ctx.mark_non_differentiable(outs[2], outs[4])
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, v_xys, v_depths, v_radii, v_conics, v_nth):
        means, ls, q, cov3d, radii, conics, comp = ctx.saved_tensors
        table, b, h, w, sem = ctx.meta
        n, dev = means.shape[0], means.device
        f32 = dict(dtype=torch.float32, device=dev)
        v_xys = _f32c(v_xys) if v_xys is not None else torch.zeros(b * n, 2, **f32)
        v_depths = _f32c(v_depths) if v_depths is not None else None
        v_conics = _f32c(v_conics) if v_conics is not None else torch.zeros(b * n, 3, **f32)
        v_m, v_s, v_q = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32), torch.empty(n, 4, **f32)
        L.check(L.load().sgn_project_views_bwd(b, n, table, L.ptr(means), L.ptr(ls), 1.0, L.ptr(q), L.ptr(cov3d),
                                               L.ptr(radii), L.ptr(conics), L.ptr(comp), L.ptr(v_xys), L.ptr(v_depths),
                                               L.ptr(v_conics), None, L.ptr(v_m), L.ptr(v_s), L.ptr(v_q), sem, h, w,
                                               L.stream_ptr()), "sgn_project_views_bwd")
        return v_m, v_s, v_q, None, None, None, None


class _SHViews(Function):
    @staticmethod
    def forward(ctx, degree, means, features_dc, features_rest, table, b):
        dev = L.require_device(means, features_dc, features_rest)
        n = means.shape[0]
        k = 1 + (features_rest.shape[1] if features_rest is not None else 0)
        means_c, dc_c = _f32c(means), _f32c(features_dc)
        rest_c = _f32c(features_rest) if features_rest is not None else None
        colors = torch.empty(b * n, 3, dtype=torch.float32, device=dev)
        L.check(L.load().sgn_sh_views_fwd(b, n, k, int(degree), table, L.ptr(means_c), L.ptr(dc_c), L.ptr(rest_c), 1,
                                          L.ptr(colors), L.stream_ptr()), "sgn_sh_views_fwd")
        ctx.meta = (int(degree), k, table, b, features_rest is not None)
        ctx.save_for_backward(means_c, colors)
        return colors.view(b, n, 3)

    @staticmethod
    def backward(ctx, v_colors):
        means, colors = ctx.saved_tensors
        degree, k, table, b, has_rest = ctx.meta
        n, dev = means.shape[0], means.device
        if v_colors is None:
            return (None,) * 6
        v_dc = torch.empty(n, 1, 3, dtype=torch.float32, device=dev)
        v_rest = torch.empty(n, k - 1, 3, dtype=torch.float32, device=dev) if has_rest else None
        L.check(L.load().sgn_sh_views_bwd(b, n, k, degree, table, L.ptr(means), 1, L.ptr(colors),
                                          L.ptr(_f32c(v_colors)), L.ptr(v_dc), L.ptr(v_rest), L.stream_ptr()),
                "sgn_sh_views_bwd")
        return None, None, v_dc, v_rest, None, None


class _RasterViews(Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity_logits, background, h, w, want_depth):
        dev = L.require_device(xys, depths, radii, conics, colors, opacity_logits, background)
        b, n = xys.shape[0], xys.shape[1]
        r = b * n
        lib = L.load()
        S = _state(dev)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        xys_c, depths_c, radii_c = _f32c(xys).reshape(r, 2), _f32c(depths).reshape(r), _i32c(radii).reshape(r)
        conics_c, colors_c = _f32c(conics).reshape(r, 3), _f32c(colors).reshape(r, 3)
        logits_c, bg_c = _f32c(opacity_logits).reshape(n), _f32c(background).reshape(3)
        ro = L.opts().copy()
        cull = bool(_ops.tile_culling_enabled)
        qmask = bool(cull and _ops._quadrant_masks_wanted())
        tiles = ((w + BLOCK - 1) // BLOCK) * ((h + BLOCK - 1) // BLOCK) * b
        out_img = torch.empty(b, h, w, 3, **f32)
        final_Ts = torch.empty(b, h, w, **f32)
        final_idx = torch.empty(b, h, w, **i32)
        out_depth = torch.empty(b, h, w, **f32) if want_depth else None
        bins_and_stats = torch.empty(2, tiles, 2, **i32)
        tile_bins, tile_stats = bins_and_stats[0], bins_and_stats[1]
        order = torch.empty(tiles + 2, **i32)
        rows = L.workspace(lib.sgn_raster_workspace_bytes(r, 0, None), dev)
        scratch = _order_scratch(S, lib, tiles, dev)
        if S.pinned is None:
            S.pinned = torch.zeros(8, dtype=torch.int32).pin_memory()
        ckey = (b, n, h, w)
        last = S.last_count.get(ckey, 0)
        cap = min(int(last * _SPEC_MARGIN) + 1024 if last > 0 else 4 * r + 1024, (1 << 31) - 1)
        n_host = C.c_int64(0)
        for attempt in range(2):
            ids = torch.empty(cap, **i32)
            arena = L.workspace(lib.sgn_rasterize_views_arena_bytes(b, n, cap), dev)
            rc = lib.sgn_rasterize_views_fwd_all(
                b, n, L.ptr(xys_c), L.ptr(depths_c), L.ptr(radii_c), L.ptr(conics_c), L.ptr(colors_c), L.ptr(logits_c),
                int(cull), h, w, BLOCK, L.ptr(bg_c), int(qmask), L.ptr(out_img), L.ptr(final_Ts), L.ptr(final_idx),
                L.ptr(out_depth), L.ptr(ids), cap, L.ptr(tile_bins), L.ptr(order), L.ptr(tile_stats), L.ptr(rows),
                rows.numel(), L.ptr(scratch), 4 * scratch.numel(), L.ptr(arena), arena.numel(), S.pinned.data_ptr(),
                C.byref(n_host), L.sort_rank_mode(), _ops.semantics().flags(), C.byref(ro), L.stream_ptr())
            if rc == _E_CAPACITY and attempt == 0:
                stats["capacity_misses"] += 1
                cap = int(n_host.value)
                continue
            L.check(rc, "sgn_rasterize_views_fwd_all")
            break
        count = int(n_host.value)
        S.last_count[ckey] = max(count, int(0.9 * last))
        stats["forwards"] += 1
        if count < 1:                     # nothing visible in any view: the background everywhere
            out_img = bg_c.expand(b, h, w, 3).contiguous()
            final_Ts = torch.ones(b, h, w, **f32)
            if want_depth:
                out_depth = torch.zeros(b, h, w, **f32)
        ro.ids_qmask = int(qmask)
        ctx.meta = (b, n, h, w, count, ro, _ops.semantics().alpha_clamp_bwd, opacity_logits.shape)
        ctx.save_for_backward(ids[:max(count, 0)], tile_bins, tile_stats, conics_c, logits_c, bg_c, final_Ts, final_idx,
                              rows)
        ctx.set_materialize_grads(False)
        alpha = 1 - final_Ts
        if want_depth:
            ctx.mark_non_differentiable(out_depth)
            return out_img, alpha, out_depth
        return out_img, alpha

    @staticmethod
    def backward(ctx, v_img, v_alpha, _v_depth=None):
        ids, tile_bins, tile_stats, conics, logits, bg, final_Ts, final_idx, rows = ctx.saved_tensors
        b, n, h, w, count, ro, alpha_clamp, op_shape = ctx.meta
        dev = conics.device
        f32 = dict(dtype=torch.float32, device=dev)
        r = b * n
        if v_img is None and v_alpha is None:
            return (None,) * 11
        if count < 1:                     # nothing was listed: no Gaussian reaches any pixel
            return (torch.zeros(b, n, 2, **f32), None, None, torch.zeros(b, n, 3, **f32), None,
                    torch.zeros(b, n, 3, **f32), torch.zeros(op_shape, **f32), None, None, None, None)
        v_alpha = _f32c(v_alpha) if v_alpha is not None else torch.zeros(b, h, w, **f32)
        v_img = _f32c(v_img) if v_img is not None else None
        lib = L.load()
        v_xy, v_conic, v_col = torch.empty(r, 2, **f32), torch.empty(r, 3, **f32), torch.empty(r, 3, **f32)
        v_op = torch.empty(n, **f32)
        gws = L.workspace(lib.sgn_raster_bwd_workspace_bytes(r), dev)
        tiles = tile_bins.shape[0]
        order = torch.empty(tiles + 2, dtype=torch.int32, device=dev)
        scratch = _order_scratch(_state(dev), lib, tiles, dev)
        L.check(lib.sgn_rasterize_views_bwd_all(
            b, n, count, h, w, L.ptr(ids), L.ptr(tile_bins), L.ptr(tile_stats), L.ptr(conics), L.ptr(logits),
            L.ptr(bg), L.ptr(final_Ts), L.ptr(final_idx), L.ptr(v_img), L.ptr(v_alpha), alpha_clamp, L.ptr(v_xy),
            L.ptr(v_conic), L.ptr(v_col), L.ptr(v_op), L.ptr(rows), rows.numel(), L.ptr(gws), gws.numel(), L.ptr(order),
            L.ptr(scratch), 4 * scratch.numel(), int(_ops.small_splat_q16), C.byref(ro), L.stream_ptr(),
            L.aux_stream_ptr(dev) if _ops.concurrent_backward else None), "sgn_rasterize_views_bwd_all")
        stats["backwards"] += 1
        return (v_xy.view(b, n, 2), None, None, v_conic.view(b, n, 3), None, v_col.view(b, n, 3), v_op.view(op_shape),
                None, None, None, None)


def _check_rasterize_mode(rasterize_mode: str) -> None:
    """Host-side, before any device work: the batched entries render the classic mode only.  The antialiased mode's
    factor is per (view, Gaussian) while ``sgn_rasterize_views_fwd_all`` repeats the per-Gaussian logits for every view
    inside the C call — per-view opacities need a change in there."""
    from .step import antialiased_mode
    if antialiased_mode(rasterize_mode):
        raise NotImplementedError(
            'rasterize_mode="antialiased" is not available for batched views: the batched rasterize entry takes one '
            "opacity logit per Gaussian and repeats it for every view, the compensation factor differs per view; "
            "render the views one by one (step.render_fused / step.train_step) in this mode")


def render_views(P: Dict[str, torch.Tensor], cams: Sequence[Camera], sh_degree_to_use: int = 3,
                 background: Optional[torch.Tensor] = None, with_depth: bool = False, block_width: int = BLOCK,
                 object_ids=None, poses=None, idft=None, group_split=None, id_range=None,
                 rasterize_mode: str = "classic", absgrad: bool = False) -> SimpleNamespace:
    """Render ``P`` (the raw leaves of :func:`sgn_rast.step.render_fused`: means, log_scales, quats, opacity_logits,
    features_dc [N,1,3], features_rest) from every camera of ``cams`` (1 to 16 :class:`scenes.Camera`, one image size)
    in one batched call.  Returns ``rgb [B,H,W,3]``, ``alpha [B,H,W]``, with ``with_depth`` also ``depth [B,H,W,1]``
    (as ``render_fused``), and the projection's ``xys [B,N,2]`` (gradient retained), ``depths``, ``radii``,
    ``conics``, ``num_tiles_hit`` as ``[B,N,...]`` (per view: feed ``densify.Stats.update`` with ``xys.grad[b]``,
    ``radii[b]``).  View b equals ``render_fused(P, cams[b])`` bit for bit.  ``rasterize_mode``: "classic" only;
    "antialiased" raises ``NotImplementedError`` (per-view compensation factors, see ``_check_rasterize_mode``).
    ``absgrad=True`` raises ``ValueError``: the batched walks do not sum absolute gradients (single views do:
    ``render_fused(absgrad=True)``)."""
    if absgrad:
        raise ValueError("absgrad is not supported for batched views (render each view with render_fused(absgrad=True))")
    _check_rasterize_mode(rasterize_mode)
    b, n, h, w = check_views(P, cams, block_width, object_ids=object_ids, poses=poses, idft=idft,
                             group_split=group_split, id_range=id_range)
    dev = P["means"].device
    if background is None:
        background = torch.zeros(3, dtype=torch.float32, device=dev)
    table = cam_table(cams)
    xys, depths, radii, conics, nth = _ProjectViews.apply(P["means"].contiguous(), P["log_scales"].contiguous(),
                                                          P["quats"].contiguous(), table, b, h, w)
    if xys.requires_grad:
        xys.retain_grad()
    rgbs = _SHViews.apply(sh_degree_to_use, P["means"].detach(), P["features_dc"].contiguous(),
                          P["features_rest"].contiguous() if P.get("features_rest") is not None else None, table, b)
    out = SimpleNamespace(xys=xys, depths=depths, radii=radii, conics=conics, num_tiles_hit=nth, rgbs=rgbs)
    res = _RasterViews.apply(xys, depths, radii, conics, nth, rgbs, P["opacity_logits"].contiguous(), background, h, w,
                             bool(with_depth))
    out.rgb, out.alpha = res[0], res[1]
    if with_depth:
        out.depth = torch.where(out.alpha[..., None] > 1e-3, res[2][..., None] / out.alpha[..., None], 10)
    return out


def train_step_views(P: Dict[str, torch.Tensor], cams: Sequence[Camera], gts: Sequence[torch.Tensor],
                     ssim_lambda: float = 0.2, sh_degree_to_use: int = 3, zero_grad: bool = True,
                     masks: Optional[Sequence[Optional[torch.Tensor]]] = None,
                     rasterize_mode: str = "classic") -> SimpleNamespace:
    """One multi-view step: :func:`render_views`, then the mean over the views of the per-view photometric loss of
    :mod:`sgn_rast.loss` ((1-l) L1 + l (1 - SSIM) on ``rgb.clamp(max=1)``, each view on its own: no SSIM window spans two
    views) — the data-parallel path's averaged-gradient semantics (``sgn_rast/dp.py``) on one GPU — and the backward.
    ``masks``: one pixel mask per view (``sgn_rast.loss.l1_ssim``'s ``mask``; an entry may be ``None``).
    ``rasterize_mode``: as :func:`render_views`."""
    _check_rasterize_mode(rasterize_mode)
    from .loss import check_mask, photometric_loss
    if len(gts) != len(cams):
        raise ValueError(f"{len(cams)} cameras but {len(gts)} ground-truth images")
    if masks is None:
        masks = [None] * len(cams)
    if len(masks) != len(cams):
        raise ValueError(f"{len(cams)} cameras but {len(masks)} masks")
    for c, m in zip(cams, masks):
        if m is not None:
            check_mask(m, c.height, c.width)
    if zero_grad:
        for p in P.values():
            p.grad = None
    out = render_views(P, cams, sh_degree_to_use, rasterize_mode=rasterize_mode)
    b = len(cams)
    loss = sum(photometric_loss(out.rgb[v], gts[v], ssim_lambda, clamp_max=1.0, mask=masks[v]) for v in range(b)) / b
    loss.backward()
    out.loss = loss.detach()
    return out

"""Feature channels composited over the depth list the RGB pass binned (``csrc/raster_features.hip``,
``csrc/semantic_loss.hip``): K arbitrary per-Gaussian values — class logits, the projection's depths, object ids —
alpha-composited in ONE walk per 16 channels, with gradients, where ``rasterize_gaussians`` with ``D != 3`` runs
ceil(D / 3) passes of the 3-channel kernels.  What a street-scene trainer builds on it:

* ``expected_depth``: the differentiable ``sum_g depth_g alpha_g T_g`` for LiDAR supervision (the reference loads depth
  images, ``data_utils.get_depth_image_from_path``; ``rasterize_gaussians_fused(depth_channel=True)`` carries no gradient);
* ``semantic_cross_entropy`` / ``semantic_argmax``: the Street Gaussians semantic term on rendered per-Gaussian logits
  against the bytes ``feed.Batch.semantic`` / ``pyramid`` deliver, and the class map ``scripts/render.py:236`` writes;
* per-object id channels for instance masks.

No CPU fallback, as everywhere in this package."""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function

from . import _lib as L
from . import ops as _ops

MAX_CHANNELS = 64


class _RasterizeFeatures(Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, features, opacity, img_height, img_width, background,
                opacity_is_logit):
        ctx.alpha_clamp_bwd = _ops.semantics().alpha_clamp_bwd      # the backward runs with the CALL's value
        ctx.set_materialize_grads(False)
        dev = L.require_device(xys, depths, radii, conics, num_tiles_hit, features, opacity, background)
        n, K = int(xys.shape[0]), int(features.shape[1])
        H, W = int(img_height), int(img_width)
        f32 = dict(dtype=torch.float32, device=dev)
        xys_c, conics_c, feats_c = _ops._f32c(xys), _ops._f32c(conics), _ops._f32c(features)
        opac_c = _ops._f32c(opacity).reshape(-1)
        bg_c = None if background is None else _ops._f32c(background)
        tile_bounds = ((W + 15) // 16, (H + 15) // 16, 1)
        # the list of the RGB pass over these very tensors (same key: nothing is binned again), or a fresh binning
        n_isect, ids, bins = (0, None, None) if n == 0 else _ops._bin_gaussians_cached(
            n, xys, depths, radii, num_tiles_hit, tile_bounds, 16, conics, opacity, bool(opacity_is_logit))
        if n_isect < 1:                   # nothing on screen: the kernels write the background, T = 1, idx = 0
            n_isect, ids, bins = 0, None, None
        lib = L.load()
        ro = L.opts().copy()              # this call's kernel options: the backward runs with the same ones
        ro.ids_qmask = int(bool(getattr(ids, "_sgn_qmask", False)))
        out_img = torch.empty(H, W, K, **f32)
        final_Ts = torch.empty(H, W, **f32)
        final_idx = torch.empty(H, W, dtype=torch.int32, device=dev)
        ws = L.workspace(lib.sgn_raster_features_workspace_bytes(n), dev) if n_isect else None
        L.check(lib.sgn_raster_features_fwd(
            H, W, 16, n, K, n_isect, L.ptr(ids), L.ptr(bins), L.ptr(xys_c), L.ptr(conics_c), L.ptr(feats_c), L.ptr(opac_c),
            int(bool(opacity_is_logit)), L.ptr(bg_c), L.ptr(out_img), L.ptr(final_Ts), L.ptr(final_idx), L.ptr(ws),
            0 if ws is None else ws.numel(), L.C.byref(ro), L.stream_ptr()), "sgn_raster_features_fwd")
        ctx.dims = (H, W, n, K, n_isect)
        ctx.ro, ctx.opacity_is_logit, ctx.opacity_shape = ro, int(bool(opacity_is_logit)), opacity.shape
        ctx.has_bg = bg_c is not None
        ctx.save_for_backward(*(t for t in (ids, bins, xys_c, conics_c, feats_c, opac_c, final_Ts, final_idx, bg_c)
                                if t is not None))
        return out_img, 1 - final_Ts

    @staticmethod
    def backward(ctx, v_out_img, v_out_alpha):
        H, W, n, K, n_isect = ctx.dims
        saved = list(ctx.saved_tensors)
        ids, bins = (saved.pop(0), saved.pop(0)) if n_isect else (None, None)
        xys, conics, feats, opac, final_Ts, final_idx = saved[:6]
        bg = saved[6] if ctx.has_bg else None
        dev = xys.device
        f32 = dict(dtype=torch.float32, device=dev)
        v_xy, v_conic = torch.empty(n, 2, **f32), torch.empty(n, 3, **f32)
        v_feats, v_opac = torch.empty(n, K, **f32), torch.empty(n, **f32)
        if n > 0:
            lib = L.load()
            v_img_c = None if v_out_img is None else _ops._f32c(v_out_img)
            v_alpha_c = None if v_out_alpha is None else _ops._f32c(v_out_alpha)
            ws = L.workspace(lib.sgn_raster_features_workspace_bytes(n), dev)
            L.check(lib.sgn_raster_features_bwd(
                H, W, 16, n, K, n_isect, L.ptr(ids), L.ptr(bins), L.ptr(xys), L.ptr(conics), L.ptr(feats), L.ptr(opac),
                ctx.opacity_is_logit, L.ptr(bg), L.ptr(final_Ts), L.ptr(final_idx), L.ptr(v_img_c), L.ptr(v_alpha_c),
                float(ctx.alpha_clamp_bwd), L.ptr(v_xy), L.ptr(v_conic), L.ptr(v_feats), L.ptr(v_opac), L.ptr(ws),
                ws.numel(), L.C.byref(ctx.ro), L.stream_ptr()), "sgn_raster_features_bwd")
        need = ctx.needs_input_grad
        return (v_xy if need[0] else None, None, None, v_conic if need[3] else None, None,
                v_feats if need[5] else None, v_opac.reshape(ctx.opacity_shape) if need[6] else None,
                None, None, None, None)


def rasterize_features(xys, depths, radii, conics, num_tiles_hit, features, opacity, img_height: int, img_width: int,
                       block_width: int = 16, background: Optional[torch.Tensor] = None, return_alpha: bool = False,
                       opacity_is_logit: bool = False, absgrad: bool = False):
    """Alpha-composite ``features [N,K]`` (1 <= K <= 64) over the depth list of these projection outputs ->
    ``out [H,W,K]`` or ``(out, alpha [H,W])``: per channel what ``rasterize_gaussians`` composites for a colour, bit for
    bit, from one walk of the lists per 16 channels.

    ``background=None`` means ZEROS — the natural background of features (an uncovered pixel has no depth and no class
    evidence), unlike ``rasterize_gaussians``' ones.  ``opacity`` holds probabilities, or — ``opacity_is_logit=True`` —
    the logits the fused path takes (the sigmoid and its backward run inside the kernels).

    The list comes from the binning cache under the key of the RGB pass over the same tensors: called after
    ``rasterize_gaussians`` / ``rasterize_gaussians_fused`` on the same ``xys, depths, radii, conics, num_tiles_hit,
    opacity`` it bins nothing.  Gradients go to ``xys``, ``conics``, ``features`` and ``opacity`` (none to ``depths``: it
    only orders the list); ``ops.semantics().alpha_clamp_bwd`` and the ``exact_exp`` option are read at call time.
    ``features`` may depend on the projection's outputs: ``depths[:, None]`` as a channel renders the expected depth,
    whose gradient reaches the means through the projection's ``v_depth`` (:func:`expected_depth`).
    ``absgrad=True`` raises ``ValueError``: the feature walks do not sum absolute gradients (the statistic belongs to
    the colour pass, ``rasterize_gaussians_fused(absgrad=True)``)."""
    if absgrad:
        raise ValueError("absgrad is not supported for feature passes (it belongs to the colour pass: "
                         "rasterize_gaussians_fused(absgrad=True))")
    if block_width != 16:
        raise ValueError("rasterize_features exists for 16x16 tiles only (block_width=16)")
    if xys.ndimension() != 2 or xys.size(1) != 2:
        raise ValueError("xys must have dimensions (N, 2)")
    if features.ndimension() != 2 or features.shape[0] != xys.shape[0]:
        raise ValueError("features must have dimensions (N, K)")
    K = int(features.shape[1])
    if not 1 <= K <= MAX_CHANNELS:
        raise ValueError(f"features must have 1..{MAX_CHANNELS} channels, got {K}")
    if background is not None and tuple(background.shape) != (K,):
        raise ValueError(f"incorrect shape of background tensor, expected ({K},)")
    c = _ops._contig
    out, alpha = _RasterizeFeatures.apply(c(xys), c(depths), c(radii), c(conics), c(num_tiles_hit), features, c(opacity),
                                          int(img_height), int(img_width), background, bool(opacity_is_logit))
    return (out, alpha) if return_alpha else out


def expected_depth(xys, depths, radii, conics, num_tiles_hit, opacity, img_height: int, img_width: int,
                   block_width: int = 16, opacity_is_logit: bool = False):
    """``(sum_g depth_g alpha_g T_g [H,W], alpha [H,W])``, differentiable: ``rasterize_features`` with ``depths[:, None]``
    as its one channel over a zero background.  The depth image's gradient reaches the means through the projection's
    depth output, on the drop-in and on the fused projection alike; an L1 against LiDAR depth is the caller's."""
    out, alpha = rasterize_features(xys, depths, radii, conics, num_tiles_hit, depths[:, None], opacity, img_height,
                                    img_width, block_width, None, True, opacity_is_logit)
    return out[..., 0], alpha


class _SemanticCrossEntropy(Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, mask):
        dev = L.require_device(logits, labels, mask)
        H, W, K = (int(s) for s in logits.shape)
        lib = L.load()
        logits_c = _ops._f32c(logits)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(max(int(lib.sgn_semantic_ce_workspace_bytes()), 16), dtype=torch.uint8, device=dev)
        L.check(lib.sgn_semantic_ce_fwd(H, W, K, L.ptr(logits_c), L.ptr(labels), ignore_index, L.ptr(mask), L.ptr(loss),
                                        L.ptr(ws), ws.numel(), L.stream_ptr()), "sgn_semantic_ce_fwd")
        ctx.ignore_index = ignore_index
        ctx.has_mask = mask is not None
        ctx.save_for_backward(logits_c, labels, ws, *(() if mask is None else (mask,)))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, v_loss):
        logits, labels, ws = ctx.saved_tensors[:3]
        mask = ctx.saved_tensors[3] if ctx.has_mask else None
        H, W, K = (int(s) for s in logits.shape)
        v_logits = torch.empty_like(logits)
        v_loss_c = _ops._f32c(v_loss).reshape(1)
        L.check(L.load().sgn_semantic_ce_bwd(H, W, K, L.ptr(logits), L.ptr(labels), ctx.ignore_index, L.ptr(mask),
                                             L.ptr(v_loss_c), L.ptr(ws), ws.numel(), L.ptr(v_logits), L.stream_ptr()),
                "sgn_semantic_ce_bwd")
        return v_logits, None, None, None


def _bytes_hw(t: torch.Tensor, H: int, W: int, what: str) -> torch.Tensor:
    if t.dtype is torch.bool:
        t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
    if t.dtype is not torch.uint8:
        raise ValueError(f"{what} must be uint8 (or bool), got {t.dtype}")
    if tuple(t.shape) == (H, W, 1):
        t = t[..., 0]
    if tuple(t.shape) != (H, W):
        raise ValueError(f"{what} must have shape ({H}, {W}) or ({H}, {W}, 1), got {tuple(t.shape)}")
    return t.contiguous()


def semantic_cross_entropy(logits_img: torch.Tensor, labels: torch.Tensor, ignore_index: Optional[int] = None,
                           mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.cross_entropy(logits_img.view(-1, K), labels.view(-1).long(), ignore_index=...)`` (mean over the counted
    pixels) in one kernel pair: ``logits_img [H,W,K]`` (K <= 64, e.g. ``rasterize_features`` of per-Gaussian class
    logits), ``labels`` uint8 ``[H,W]`` or ``[H,W,1]`` as ``feed.Batch.semantic`` / ``pyramid`` deliver it.  A pixel
    counts when its label is not ``ignore_index``, is below K and — with ``mask`` (uint8 / bool, non-zero = keep, the
    data set's pixel mask) — is kept.  The loss sum and the count stay on the device; an image without a counted pixel
    gives loss 0 and a zero gradient."""
    if logits_img.ndimension() != 3:
        raise ValueError("logits_img must have dimensions (H, W, K)")
    H, W, K = (int(s) for s in logits_img.shape)
    if not 1 <= K <= MAX_CHANNELS:
        raise ValueError(f"logits_img must have 1..{MAX_CHANNELS} classes, got {K}")
    ii = -1 if ignore_index is None else int(ignore_index)
    if ii < -1 or ii > 255:
        ii = -1          # no uint8 label can equal it
    labels_c = _bytes_hw(labels, H, W, "labels")
    mask_c = None if mask is None else _bytes_hw(mask, H, W, "mask")
    return _SemanticCrossEntropy.apply(logits_img, labels_c, ii, mask_c)


def semantic_argmax(logits_img: torch.Tensor) -> torch.Tensor:
    """The uint8 class map ``scripts/render.py:236`` writes for a ``semantic`` output: ``argmax`` over the last axis."""
    return torch.argmax(logits_img, dim=-1).to(torch.uint8)

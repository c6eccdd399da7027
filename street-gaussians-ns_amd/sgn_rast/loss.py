"""Photometric loss of the reference's training step on MI355X: L1 + SSIM, one kernel each way.

SURVEY.md §8f row 3.  The reference computes (``street_gaussians_ns/sgn_splatfacto.py:1084-1087``)

    Ll1 = torch.abs(gt_img - rgb).mean()
    simloss = 1 - self.ssim(gt_img.permute(2, 0, 1)[None, ...], rgb.permute(2, 0, 1)[None, ...])
    loss = (1 - ssim_lambda) * Ll1 + ssim_lambda * simloss

with ``self.ssim = pytorch_msssim.SSIM(data_range=1.0, size_average=True, channel=3)`` (``:330``): ten depthwise
``conv2d`` launches forward plus their autograd graph.  Here both terms come out of ``csrc/loss.hip`` through the C
ABI (``sgn_l1_ssim_fwd/bwd``) directly on the rasterizer's HWC image; fails loudly without the HIP library.

* :func:`l1_ssim` — ``(Ll1, ssim)`` of two [H,W,3] images, gradient to ``pred``.
* ``mask=`` on :func:`l1_ssim` / :func:`photometric_loss` — the batch's boolean pixel mask (``:1081-1083``:
  ``gt_img *= mask; rgb *= mask``) folded into the same two kernels (``sgn_l1_ssim_masked_fwd/bwd``).
* :func:`image_metrics` — ``(psnr, ssim)`` of the evaluation path (``:1135-1151``), one no-grad forward.
* ``gt`` of dtype ``torch.uint8`` on all three — the data set's bytes as they are cached (``cache_images_type:
  "uint8"``), read by the kernels themselves (``sgn_l1_ssim_gt8_fwd/bwd``) as the correctly rounded ``u / 255`` that
  ``get_gt_img`` (``:1003-1012``) forms: bit for bit the float call on ``gt.float() / 255`` computed on the CPU, with no
  float image materialised and the byte tensor, a quarter the size, kept for the backward.
* :class:`SSIM` — ``pytorch_msssim.SSIM`` call shape (``forward(X, Y)`` on [1,3,H,W]) for the import shim; the
  permuted views the reference passes are recognised and used in place (no NCHW copy).
* :func:`sky_accumulation`, :func:`object_acc_entropy`, :func:`accumulation_losses` — the two accumulation
  regularisers of the reference's loss dictionary (``sgn_splatfacto.py:1090-1093``,
  ``sgn_splatfacto_scene_graph.py:386-389``): ``(sky_mask * accumulation).mean()`` and the binary entropy of the clamped
  object accumulation, one streaming pass each way for both (``sgn_acc_losses_fwd/bwd``) instead of ~10 elementwise
  torch launches forward and as many backward.
"""
from __future__ import annotations

import torch

from . import _lib as L


def check_mask(mask, h: int, w: int) -> None:
    """Host-side validation of a pixel mask for an ``h`` x ``w`` image, before anything is launched: a ``bool`` or
    ``uint8`` tensor of shape [H,W] or [H,W,1] (the reference's batch["mask"]).  Any other dtype is a ``TypeError``: a
    float image would be a weight map, which the reference does not have."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        what = mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise TypeError(f"mask must be a bool or uint8 tensor (non-zero = keep), got {what}")
    if tuple(mask.shape) not in ((h, w), (h, w, 1)):
        raise ValueError(f"mask must have the image's {h * w} pixels as [{h},{w}] or [{h},{w},1], "
                         f"got {tuple(mask.shape)}")


def _mask_bytes(mask: torch.Tensor) -> torch.Tensor:
    """The mask as contiguous uint8 [H*W...]; a contiguous ``bool`` is viewed, not copied.  No gradient."""
    m = mask.detach().contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _check_pred(pred) -> None:
    """A rendered image is floating point; an integer ``pred`` (a byte image passed on the wrong side) is a
    ``TypeError`` on the host, not a gradient-less conversion."""
    if isinstance(pred, torch.Tensor) and not pred.is_floating_point():
        raise TypeError(f"pred must be a floating-point image, got {pred.dtype} (uint8 is accepted for gt only)")


def _check_images(pred, gt):
    if pred.dim() != 3 or pred.shape[-1] != 3 or pred.shape != gt.shape:
        raise ValueError(f"l1_ssim expects two [H,W,3] images, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    h, w = pred.shape[0], pred.shape[1]
    if min(h, w) <= 10:
        raise ValueError("images must be larger than the 11-tap SSIM window")   # pytorch_msssim asserts too
    return h, w


def _forward(ctx, pred, gt, data_range, clamp_max, ssim_lambda, mask=None):
    if mask is not None or gt.dtype == torch.uint8:      # the byte entries are the masked ones with a nullable mask
        return _forward_masked(ctx, pred, gt, data_range, clamp_max, ssim_lambda, mask,
                               bool(ctx.needs_input_grad[0]))
    _check_pred(pred)
    L.require_device(pred, gt)
    h, w = _check_images(pred, gt)
    p, g = pred.contiguous().float(), gt.contiguous().float()
    lib = L.load()
    out3 = torch.empty(3, dtype=torch.float32, device=p.device)
    need_grad = int(bool(ctx.needs_input_grad[0]))
    maps = L.workspace(lib.sgn_l1_ssim_workspace_bytes(h, w, need_grad), p.device)
    cmax = float("inf") if clamp_max is None else float(clamp_max)
    L.check(lib.sgn_l1_ssim_fwd(h, w, L.ptr(p), L.ptr(g), float(data_range), cmax, float(ssim_lambda), L.ptr(out3),
                                need_grad, L.ptr(maps), maps.numel(), L.stream_ptr()), "sgn_l1_ssim_fwd")
    ctx.hw, ctx.cmax, ctx.maps, ctx.masked = (h, w), cmax, maps, False
    ctx.save_for_backward(p, g)
    return out3


def _forward_masked(ctx, pred, gt, data_range, clamp_max, ssim_lambda, mask, need_grad):
    """The masked entry points: ``out4 = [Ll1, ssim, weighted sum, mse]`` of ``min(pred, clamp_max) * m`` and
    ``gt * m``; ``mask`` may be ``None`` here (the metrics without a mask).  ``ctx`` None: nothing kept for a backward.
    A ``uint8`` ``gt`` goes to the byte entries as it is (``gt * m`` is then ``(u / 255) * m``)."""
    _check_pred(pred)
    if pred.dim() == 3 and mask is not None:
        check_mask(mask, pred.shape[0], pred.shape[1])                 # TypeError / ValueError before the device check
    L.require_device(pred, gt, mask)
    h, w = _check_images(pred, gt)
    gt8 = gt.dtype == torch.uint8
    p, g = pred.contiguous().float(), gt.detach().contiguous() if gt8 else gt.contiguous().float()
    m = None if mask is None else _mask_bytes(mask)
    lib = L.load()
    out4 = torch.empty(4, dtype=torch.float32, device=p.device)
    maps = L.workspace(lib.sgn_l1_ssim_masked_workspace_bytes(h, w, int(need_grad)), p.device)
    cmax = float("inf") if clamp_max is None else float(clamp_max)
    name = "sgn_l1_ssim_gt8_fwd" if gt8 else "sgn_l1_ssim_masked_fwd"
    L.check(getattr(lib, name)(h, w, L.ptr(p), L.ptr(g), L.ptr(m), float(data_range), cmax, float(ssim_lambda),
                               L.ptr(out4), int(need_grad), L.ptr(maps), maps.numel(), L.stream_ptr()), name)
    if ctx is not None:
        ctx.hw, ctx.cmax, ctx.maps, ctx.masked, ctx.gt8 = (h, w), cmax, maps, True, gt8
        ctx.save_for_backward(p, g, m)
    return out4


def _backward(ctx, gscale):
    h, w = ctx.hw
    if ctx.masked:
        p, g, m = ctx.saved_tensors
        v = torch.empty_like(p)
        name = "sgn_l1_ssim_gt8_bwd" if ctx.gt8 else "sgn_l1_ssim_masked_bwd"
        L.check(getattr(L.load(), name)(h, w, L.ptr(p), L.ptr(g), L.ptr(m), ctx.cmax, L.ptr(ctx.maps), L.ptr(gscale),
                                        L.ptr(v), L.stream_ptr()), name)
        return v
    p, g = ctx.saved_tensors
    v = torch.empty_like(p)
    L.check(L.load().sgn_l1_ssim_bwd(h, w, L.ptr(p), L.ptr(g), ctx.cmax, L.ptr(ctx.maps), L.ptr(gscale), L.ptr(v),
                                     L.stream_ptr()), "sgn_l1_ssim_bwd")
    return v


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, data_range, clamp_max, mask=None):
        out3 = _forward(ctx, pred, gt, data_range, clamp_max, 0.0, mask)
        return out3[0], out3[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        gscale = torch.stack([g_l1.reshape(()), g_ssim.reshape(())]).float().contiguous()
        return _backward(ctx, gscale), None, None, None, None


_LAMBDA_VEC: dict = {}


class _Photometric(torch.autograd.Function):
    """(1 - l) Ll1 + l (1 - ssim) as ONE node: the weighted sum is formed in the reduction kernel, the backward
    turns the upstream scalar into the two weights with a single tiny multiply."""

    @staticmethod
    def forward(ctx, pred, gt, ssim_lambda, clamp_max, mask=None):
        out3 = _forward(ctx, pred, gt, 1.0, clamp_max, ssim_lambda, mask)
        ctx.lam = float(ssim_lambda)
        return out3[2]

    @staticmethod
    def backward(ctx, g):
        key = (ctx.lam, str(g.device))
        if key not in _LAMBDA_VEC:
            _LAMBDA_VEC[key] = torch.tensor([1.0 - ctx.lam, -ctx.lam], dtype=torch.float32, device=g.device)
        gscale = (_LAMBDA_VEC[key] * g.reshape(())).contiguous()
        return _backward(ctx, gscale), None, None, None, None


def l1_ssim(pred: torch.Tensor, gt: torch.Tensor, data_range: float = 1.0, clamp_max=None, mask=None):
    """(mean |gt - pred|, SSIM(gt, pred)) for [H,W,3] images; differentiable w.r.t. ``pred``.
    ``clamp_max`` folds the caller's ``torch.clamp(rgb, max=clamp_max)`` (``sgn_splatfacto.py:969``) into the kernels:
    ``pred`` is read as ``min(pred, clamp_max)`` and the gradient is zero where ``pred > clamp_max``.

    ``mask`` ([H,W] or [H,W,1], ``bool`` or ``uint8``, non-zero = keep) is the reference's batch["mask"]
    (``:1081-1083``): both terms are taken of ``min(pred, clamp_max) * mask`` and ``gt * mask``.  As in the reference the
    means keep their unmasked denominators (3HW and 3(H-10)(W-10): nothing is normalised by the number of kept
    pixels), SSIM windows that straddle the mask edge see zeros on both images, and the clamp comes before the mask.
    The gradient is an exact 0 at masked pixels; the mask gets none; unlike the reference, neither ``pred`` nor ``gt``
    is modified.  ``mask=None`` is the unmasked path, unchanged.

    ``gt`` of dtype ``torch.uint8`` is the cached byte image: each byte is read in the kernel as the correctly rounded
    fp32 ``u / 255`` (not ``u * (1 / 255)``, which differs in the last bit for 126 of the 256 values), so the results are
    those of ``gt.cpu().float() / 255`` bit for bit, and the bytes are what is saved for the backward.  An integer
    ``pred`` is a ``TypeError``; any other ``gt`` dtype is converted with ``.float()`` as before."""
    if mask is None:
        return _L1SSIM.apply(pred, gt, data_range, clamp_max)
    return _L1SSIM.apply(pred, gt, data_range, clamp_max, mask)


def photometric_loss(pred: torch.Tensor, gt: torch.Tensor, ssim_lambda: float = 0.2, clamp_max=None,
                     mask=None) -> torch.Tensor:
    """``(1 - l) * Ll1 + l * (1 - ssim)`` — the sum of losses["Ll1"] and losses["simloss"] (``:1086-1087``), one
    forward and one backward kernel plus a single scalar multiply.  ``mask`` and a ``uint8`` ``gt``: see
    :func:`l1_ssim`."""
    if mask is None:
        return _Photometric.apply(pred, gt, ssim_lambda, clamp_max)
    return _Photometric.apply(pred, gt, ssim_lambda, clamp_max, mask)


def _metrics_out4(pred: torch.Tensor, gt: torch.Tensor, mask=None, data_range: float = 1.0) -> torch.Tensor:
    """``[Ll1, ssim, Ll1, mse]`` of the (masked) images: one forward launch plus the reduce, no graph, no clamp."""
    with torch.no_grad():
        return _forward_masked(None, pred.detach(), gt.detach(), data_range, None, 0.0, mask, False)


def image_metrics(pred: torch.Tensor, gt: torch.Tensor, mask=None, data_range: float = 1.0):
    """``(psnr, ssim)`` of two [H,W,3] images as the reference's evaluation computes them (``:1135-1151``: ``gt *
    mask``, ``rgb * mask``, then ``PeakSignalNoiseRatio(data_range=1.0)`` and ``SSIM``): ``psnr = 10 log10(data_range^2 /
    mse)`` with ``mse`` the mean over all 3HW elements of the masked images (identical images: ``+inf``).  0-dim device
    tensors without an autograd graph and without a host sync.  ``mask``, ``uint8`` ``gt``: see :func:`l1_ssim`."""
    out4 = _metrics_out4(pred, gt, mask, data_range)
    psnr = 10.0 * torch.log10(float(data_range) ** 2 / out4[3].double())
    return psnr.float(), out4[1]


def _as_hwc(t: torch.Tensor) -> torch.Tensor:
    """[1,3,H,W] -> [H,W,3] without a copy when ``t`` is the permuted view of an HWC image (the reference's case)."""
    if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 3:
        raise ValueError(f"SSIM expects [1,3,H,W] inputs, got {tuple(t.shape)}")
    return t[0].permute(1, 2, 0)


class SSIM(torch.nn.Module):
    """``pytorch_msssim.SSIM`` for the configuration the reference builds (``sgn_splatfacto.py:330``):
    ``data_range`` free, ``size_average=True``, ``channel=3``, 11-tap window, sigma 1.5, 2-D images, batch 1.
    Anything else raises.  SSIM is symmetric, so the gradient goes to whichever argument requires it."""

    def __init__(self, data_range: float = 255, size_average: bool = True, win_size: int = 11,
                 win_sigma: float = 1.5, channel: int = 3, spatial_dims: int = 2, K=(0.01, 0.03),
                 nonnegative_ssim: bool = False):
        super().__init__()
        if not size_average or win_size != 11 or win_sigma != 1.5 or channel != 3 or spatial_dims != 2 \
                or tuple(K) != (0.01, 0.03) or nonnegative_ssim:
            raise NotImplementedError("sgn_rast.loss.SSIM implements the reference's configuration only")
        self.data_range = float(data_range)

    def forward(self, X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        x, y = _as_hwc(X), _as_hwc(Y)
        if x.requires_grad and y.requires_grad:
            # both sides differentiable: d/dX from f(X, Y.detach()), d/dY from f(Y, X.detach()) (symmetry)
            a = l1_ssim(x, y.detach(), self.data_range)[1]
            b = l1_ssim(y, x.detach(), self.data_range)[1]
            return a + b - a.detach()
        if x.requires_grad:
            return l1_ssim(x, y, self.data_range)[1]
        return l1_ssim(y, x, self.data_range)[1]


# ------------------------------------------------------------------------------------------- accumulation regularisers
SKY = 2   # street_gaussians_ns/data/utils/data_utils.py:26-29  SemanticType.SKY


def _sem_arg(semantic: torch.Tensor, n: int):
    """(contiguous integer tensor, bytes per element) the C ABI accepts: 1 (uint8 / bool), 4 (int32), 8 (int64)."""
    if semantic.numel() != n:
        raise ValueError(f"semantic has {semantic.numel()} elements, the accumulation image {n}")
    t = semantic.detach()
    if t.dtype == torch.bool:
        t = t.contiguous().view(torch.uint8)
    elif t.dtype not in (torch.uint8, torch.int32, torch.int64):
        t = t.to(torch.int64)
    t = t.contiguous()
    return t, t.element_size()


class _AccLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, accumulation, semantic, sky_value, object_acc):
        dev = L.require_device(accumulation, semantic, object_acc)
        if accumulation is None and object_acc is None:
            raise ValueError("accumulation_losses needs an accumulation image, an object accumulation image or both")
        if accumulation is not None and semantic is None:
            raise ValueError("the sky-accumulation term needs the semantic image")
        n = (accumulation if accumulation is not None else object_acc).numel()
        if n < 1 or (accumulation is not None and object_acc is not None and object_acc.numel() != n):
            raise ValueError("accumulation images must be non-empty and of one size")
        acc = None if accumulation is None else accumulation.detach().float().contiguous()
        obj = None if object_acc is None else object_acc.detach().float().contiguous()
        sem, sem_bytes = (None, 0) if accumulation is None else _sem_arg(semantic, n)
        if sem is not None and sem.dtype == torch.uint8 and semantic.dtype == torch.bool:
            sky_value = 1 if sky_value else 0      # a boolean mask: "is sky" is True
        lib = L.load()
        out2 = torch.empty(2, dtype=torch.float32, device=dev)
        ws = L.workspace(lib.sgn_acc_losses_workspace_bytes(n), dev)
        L.check(lib.sgn_acc_losses_fwd(n, L.ptr(acc), L.ptr(sem), sem_bytes, int(sky_value), L.ptr(obj), L.ptr(out2),
                                       L.ptr(ws), ws.numel(), L.stream_ptr()), "sgn_acc_losses_fwd")
        ctx.n, ctx.sem_bytes, ctx.sky_value = n, sem_bytes, int(sky_value)
        ctx.acc_shape = None if accumulation is None else accumulation.shape
        ctx.obj_shape = None if object_acc is None else object_acc.shape
        ctx.has_sem, ctx.has_obj = sem is not None, obj is not None
        ctx.save_for_backward(*[t for t in (sem, obj) if t is not None])   # in-place edits before backward are detected
        return out2[0], out2[1]

    @staticmethod
    def backward(ctx, g_sky, g_ent):
        want_acc = ctx.acc_shape is not None and ctx.needs_input_grad[0]
        want_obj = ctx.obj_shape is not None and ctx.needs_input_grad[3]
        if not (want_acc or want_obj):
            return None, None, None, None
        saved = list(ctx.saved_tensors)
        sem = saved.pop(0) if ctx.has_sem else None
        obj = saved.pop(0) if ctx.has_obj else None
        gscale = torch.stack([g_sky.reshape(()), g_ent.reshape(())]).float().contiguous()
        f32 = dict(dtype=torch.float32, device=gscale.device)
        v_acc = torch.empty(ctx.n, **f32) if want_acc else None
        v_obj = torch.empty(ctx.n, **f32) if want_obj else None
        L.check(L.load().sgn_acc_losses_bwd(ctx.n, L.ptr(sem) if want_acc else None, ctx.sem_bytes, ctx.sky_value,
                                            L.ptr(obj) if want_obj else None, L.ptr(gscale), L.ptr(v_acc),
                                            L.ptr(v_obj), L.stream_ptr()), "sgn_acc_losses_bwd")
        return (v_acc.reshape(ctx.acc_shape) if want_acc else None, None, None,
                v_obj.reshape(ctx.obj_shape) if want_obj else None)


def accumulation_losses(accumulation, semantic, object_acc, sky_value: int = SKY):
    """``((sky_mask * accumulation).mean(), -(o log o + (1 - o) log(1 - o)).mean())`` with ``sky_mask = (semantic ==
    sky_value)`` and ``o = clamp(object_acc, 1e-5, 1 - 1e-5)`` — the reference's two accumulation regularisers BEFORE
    their config multipliers (``sky_acc_loss_mult`` 0.5, ``object_acc_entropy_loss_mult`` 0.001), in one forward and
    one backward pass.  ``accumulation`` / ``object_acc``: [H,W,1] (or [H,W]) float images; ``semantic``: integer (the
    reference's int64 [H,W,1]) or boolean "is sky" image.  Either image may be ``None`` (its term is then 0)."""
    return _AccLosses.apply(accumulation, semantic, sky_value, object_acc)


def sky_accumulation(accumulation, semantic, sky_value: int = SKY) -> torch.Tensor:
    """``(sky_mask * accumulation).mean()`` (``sgn_splatfacto.py:1092-1093``)."""
    return _AccLosses.apply(accumulation, semantic, sky_value, None)[0]


def object_acc_entropy(object_acc) -> torch.Tensor:
    """``-(o log o + (1 - o) log(1 - o)).mean()``, ``o = clamp(object_acc, 1e-5, 1 - 1e-5)``
    (``sgn_splatfacto_scene_graph.py:387-389``)."""
    return _AccLosses.apply(None, None, 0, object_acc)[1]

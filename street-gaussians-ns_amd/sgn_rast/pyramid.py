"""Coarse-to-fine training on the byte path: the resolution schedule and one pyramid level of a batch's ground truth.

The reference trains coarse to fine.  ``SplatfactoModel._get_downscale_factor`` returns
``d = 2 ** max(num_downscales - step // resolution_schedule, 0)``, and while ``d > 1`` the reference rescales the camera
by ``1 / d``, resizes the batch's image with ``TF.resize(..., antialias=None)`` — plain bilinear, ``align_corners=False``
— and the mask and the semantic map with ``InterpolationMode.NEAREST`` (``sgn_splatfacto.py:766-784``, ``:822-823``,
``:1055-1071``).  Here one HIP kernel (``csrc/gt_pyramid.hip`` through ``sgn_gt_downscale``) turns a
:class:`sgn_rast.feed.Batch` — the ``uint8`` bytes as the feed caches them — into the ground truth of one level, and
three small host functions follow the schedule:

* :func:`downscale_factor` — the reference's expression.
* :func:`level_size` — ``(ceil(h / d), ceil(w / d))``, the size ``get_loss_dict`` resizes the ground truth to.
* :func:`scaled_camera` — nerfstudio's ``rescale_output_resolution(1 / d)`` on a :class:`sgn_rast.scenes.Camera`.
* :func:`downscale` — the level: float32 image, mask and semantic bytes, fresh tensors on the current stream.

The loop (``feed`` an :class:`sgn_rast.feed.ImageFeed`)::

    feed.prefetch(order[0])
    for s in range(steps):
        d = downscale_factor(s, num_downscales, resolution_schedule)
        cam_d = scaled_camera(cam, d)
        b = feed.get(order[s])
        lv = downscale(b, d, size=(cam_d.height, cam_d.width))
        feed.prefetch(order[s + 1])
        out = train_step(P, cam_d, w_img, w_a, gt=lv.image, mask=lv.mask, fused=True)
        sky, entropy = accumulation_losses(acc, lv.semantic, object_acc)

The arithmetic of the kernel is a contract (``include/sgn_rast.h``, ``tests/pyramid_oracle.py``): fp32, no FMA, each tap
the correctly rounded ``u / 255`` the byte loss forms, so a level is bit for bit its restatement.  No CPU path.
"""
from __future__ import annotations

import dataclasses
import operator
from typing import List, NamedTuple, Optional, Tuple, Union

import torch

from . import _lib as L
from .loss import check_mask
from .scenes import Camera

MAX_DIM = 16384      # sgn_gt_downscale: 32-bit element indices


class Level(NamedTuple):
    """One pyramid level of a batch: ``image`` float32 [oh,ow,3] (``uint8`` [H,W,3], the batch's own, at ``d == 1``);
    ``mask`` ``None`` or in the dtype and trailing-``1`` shape it came in as ([oh,ow] or [oh,ow,1]); ``semantic``
    ``None`` or ``uint8`` in the same trailing shape."""
    image: torch.Tensor
    mask: Optional[torch.Tensor]
    semantic: Optional[torch.Tensor]


def _nonneg_int(name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{name} must be a non-negative int, got {v!r}")
    if v < 0:
        raise ValueError(f"{name} must be a non-negative int, got {v}")
    return v


def downscale_factor(step: int, num_downscales: int, resolution_schedule: int) -> int:
    """``2 ** max(num_downscales - step // resolution_schedule, 0)``: ``SplatfactoModel._get_downscale_factor``."""
    step, num_downscales = _nonneg_int("step", step), _nonneg_int("num_downscales", num_downscales)
    if _nonneg_int("resolution_schedule", resolution_schedule) < 1:
        raise ValueError("resolution_schedule must be >= 1")
    return 2 ** max(num_downscales - step // resolution_schedule, 0)


def _check_d(d) -> int:
    if isinstance(d, bool) or not isinstance(d, int):
        raise TypeError(f"d must be an int (a power of two >= 1), got {type(d).__name__}")
    if d < 1 or d & (d - 1):
        raise ValueError(f"d must be a power of two >= 1, got {d}")
    return d


def level_size(h: int, w: int, d: int) -> Tuple[int, int]:
    """``(ceil(h / d), ceil(w / d))``: the size ``get_loss_dict`` resizes the ground truth to
    (``sgn_splatfacto.py:1055-1071``)."""
    d = _check_d(d)
    if h < 1 or w < 1:
        raise ValueError(f"h and w must be >= 1, got {h} x {w}")
    return (h + d - 1) // d, (w + d - 1) // d


def scaled_camera(cam: Camera, d: int) -> Camera:
    """``cam`` for level ``d``, as nerfstudio's ``Cameras.rescale_output_resolution(1 / d)`` leaves it: ``fx, fy, cx,
    cy`` times ``1 / d``, ``width`` and ``height`` ``int(W * (1 / d))`` (floor, where :func:`level_size` is ceil: on
    sizes ``d`` does not divide, pass this camera's size to :func:`downscale`).  ``viewmat`` and ``cam_pos`` are shared,
    not copied; ``d == 1`` returns ``cam`` itself."""
    if _check_d(d) == 1:
        return cam
    s = 1.0 / d
    return dataclasses.replace(cam, width=int(cam.width * s), height=int(cam.height * s), fx=cam.fx * s, fy=cam.fy * s,
                               cx=cam.cx * s, cy=cam.cy * s)


def _check_triple(item):
    """Host-side validation of one ``(image, mask, semantic)``: ``TypeError`` / ``ValueError``; returns ``(h, w)``."""
    try:
        if isinstance(item, torch.Tensor):
            raise TypeError
        image, mask, semantic = item
    except (TypeError, ValueError):
        raise TypeError("batch must be a feed.Batch or an (image, mask, semantic) triple (or a list of them), got "
                        f"{type(item).__name__}") from None
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
        what = image.dtype if isinstance(image, torch.Tensor) else type(image).__name__
        raise TypeError(f"image must be a uint8 tensor (the bytes the feed caches), got {what}")
    if image.dim() != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"image must be [H,W,3], got {tuple(image.shape)}")
    h, w = int(image.shape[0]), int(image.shape[1])
    if h > MAX_DIM or w > MAX_DIM:
        raise ValueError(f"image sides are limited to {MAX_DIM}, got {h} x {w}")
    if mask is not None:
        check_mask(mask, h, w)
    if semantic is not None:
        if not isinstance(semantic, torch.Tensor) or semantic.dtype != torch.uint8:
            what = semantic.dtype if isinstance(semantic, torch.Tensor) else type(semantic).__name__
            raise TypeError(f"semantic must be a uint8 tensor of class ids (as the feed stores it), got {what}")
        if tuple(semantic.shape) not in ((h, w), (h, w, 1)):
            raise ValueError(f"semantic must be [{h},{w}] or [{h},{w},1] like its image, got {tuple(semantic.shape)}")
    return h, w


def _check_size(size, h: int, w: int) -> Tuple[int, int]:
    try:
        oh, ow = size
        oh, ow = operator.index(oh), operator.index(ow)
    except (TypeError, ValueError):
        raise TypeError(f"size must be a pair of ints (oh, ow), got {size!r}") from None
    if not (1 <= oh <= h and 1 <= ow <= w):
        raise ValueError(f"size must lie in 1..{h} x 1..{w} (a level is never larger than its image), got {oh} x {ow}")
    return oh, ow


def _bytes(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _one(item, hw: Tuple[int, int], out_hw: Tuple[int, int]) -> Level:
    image, mask, semantic = item
    dev = L.require_device(image, mask, semantic)
    (h, w), (oh, ow) = hw, out_hw
    img = image.detach().contiguous()
    m = None if mask is None else _bytes(mask)
    s = None if semantic is None else _bytes(semantic)
    image_out = torch.empty(oh, ow, 3, dtype=torch.float32, device=dev)
    tail = lambda t: (oh, ow, 1) if t.dim() == 3 else (oh, ow)
    mask_out = None if m is None else torch.empty(tail(mask), dtype=torch.uint8, device=dev)
    sem_out = None if s is None else torch.empty(tail(semantic), dtype=torch.uint8, device=dev)
    L.check(L.load().sgn_gt_downscale(h, w, oh, ow, L.ptr(img), L.ptr(m), L.ptr(s), L.ptr(image_out), L.ptr(mask_out),
                                      L.ptr(sem_out), L.stream_ptr()), "sgn_gt_downscale")
    if mask_out is not None and mask.dtype == torch.bool:
        mask_out = mask_out.view(torch.bool)           # nearest copies source bytes: 0 / 1 stay 0 / 1
    return Level(image_out, mask_out, sem_out)


def downscale(batch, d: int, size: Optional[Tuple[int, int]] = None) -> Union[Level, List[Level]]:
    """The ground truth of pyramid level ``d`` of ``batch``, in one launch per item.

    ``batch``: a :class:`sgn_rast.feed.Batch` or any ``(image, mask, semantic)`` triple of device tensors — ``image``
    ``uint8`` [H,W,3]; ``mask`` ``None`` or ``bool`` / ``uint8`` [H,W] or [H,W,1]; ``semantic`` ``None`` or ``uint8``
    [H,W] or [H,W,1] — or a list of them, which returns a list (``train_step_views`` with ``gts=[lv.image ...]`` and
    ``masks=[lv.mask ...]``).  ``d``: a power of two ``>= 1``.  ``size=(oh, ow)`` overrides :func:`level_size`: the
    reference's ground truth uses ceil and its camera floor, so on sizes ``d`` does not divide the reference itself fails
    with a shape mismatch; pass the scaled camera's ``(height, width)``.

    The image is resized as the reference's ``TF.resize(..., antialias=None)`` does (bilinear, ``align_corners=False``)
    from the correctly rounded ``u / 255`` of each byte, the mask and the semantic map by nearest neighbour; the
    arithmetic is the contract of ``sgn_gt_downscale`` (``include/sgn_rast.h``).  The pieces go straight into
    ``step.train_step(P, scaled_camera(cam, d), ..., gt=lv.image, mask=lv.mask)``,
    ``loss.accumulation_losses(acc, lv.semantic, ...)`` and ``views.train_step_views(..., gts=, masks=)``.

    Everything is validated on the host first (``TypeError`` / ``ValueError`` before any device call); CPU tensors then
    fail the library's device check (``SgnRastError``): there is no CPU path.  The launch goes to the current stream
    and nothing synchronises the host.

    **Lifetime.**  The outputs are fresh tensors: unlike the batch they come from, they outlive the feed slot.  Once
    ``downscale`` is enqueued the feed's slot contract is satisfied for that batch — the next ``prefetch`` orders its
    copy behind this launch — and the level may be kept as long as it is needed.

    ``d == 1`` with ``size=None`` returns ``Level(batch.image, batch.mask, batch.semantic)`` untouched: the image stays
    ``uint8``, which the byte loss takes as it is (and the slot contract applies to it as to the batch).
    """
    single = not isinstance(batch, list)
    items = [batch] if single else batch
    if not items:
        raise ValueError("batch is an empty list")
    hws = [_check_triple(it) for it in items]
    d = _check_d(d)
    if size is None:
        if d == 1:
            out = [Level(*it) for it in items]
            return out[0] if single else out
        sizes = [level_size(h, w, d) for h, w in hws]
    else:
        sizes = [_check_size(size, h, w) for h, w in hws]
    out = [_one(it, hw, ohw) for it, hw, ohw in zip(items, hws, sizes)]
    return out[0] if single else out

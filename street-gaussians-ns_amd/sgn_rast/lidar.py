"""LiDAR depth supervision on the device (``csrc/lidar_depth.hip``): sweep -> per-pixel target -> loss and gradient ->
evaluation depth metrics, with no host read in the training step.

The reference trains its depth term against depth images made offline, point by point on the CPU
(``data_utils.get_depth_image_from_path`` loads them).  Here:

* ``splat_depth(sweeps, cam)``                   one or several ``(points, l2w)`` sweeps — several sweeps, several LiDARs —
  splatted into one camera's ``[H,W]`` target: the nearest return per pixel, then the occlusion filter the LiDAR / camera
  parallax makes necessary; ``0`` marks a pixel without a return;
* ``depth_loss(dsum, alpha, target, kind)``      the L1 (or inverse-depth L1) of ``D = dsum / alpha`` against the target,
  mean over the counted pixels, on the pair ``features.expected_depth`` returns; an ``autograd.Function``, gradients to
  ``dsum`` and ``alpha``;
* ``depth_metrics(dsum, alpha, target)``         abs_rel / rmse / mae / delta1 / count over the same pixels, for evaluation.

``step.train_step(..., lidar_depth=target)`` adds the term to the single-view step.  The scene-graph and multi-view step
functions do not take it: their callers compose ``features.expected_depth`` and ``depth_loss`` themselves, over the
projection outputs and the opacity tensor their RGB pass binned under.

The arithmetic is the contract of ``include/sgn_rast.h`` ("LiDAR DEPTH"), which ``tests/lidar_depth_oracle.py`` restates:
the target bit for bit in float32, the loss against float64.  No CPU fallback, as everywhere in this package.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
from torch.autograd import Function

from . import _lib as L
from . import seed as _seed
from .loss import _mask_bytes, check_mask

MAX_RADIUS = 8                  # SGN_LIDAR_DEPTH_MAX_RADIUS
WS_BYTES = 64                   # SGN_DEPTH_LOSS_WS_BYTES
KINDS = {"l1": 0, "inverse": 1}  # SGN_DEPTH_LOSS_L1 / SGN_DEPTH_LOSS_INVERSE


def _validate_sweep(k, points):
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"sweep {k}: points must be a torch.Tensor, got {type(points).__name__}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"sweep {k}: points must have shape (N, 3), got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise ValueError(f"sweep {k}: points must be float32, got {points.dtype}")
    if not 1 <= points.shape[0] <= _seed.MAX_POINTS:
        raise ValueError(f"sweep {k}: points must hold between 1 and 2**27 rows, got {points.shape[0]}")


def splat_depth(sweeps, cam: _seed.SeedCamera, min_z: float = -2.0, max_depth: float = math.inf, radius: int = 2,
                rel_tol: float = 0.05) -> torch.Tensor:
    """The LiDAR depth target of one camera, ``[H,W]`` float32 on the device: camera-frame ``z`` of the nearest return
    per pixel, ``0`` where there is none.

    ``sweeps`` is one ``(points, l2w)`` pair or a list of them: ``points`` [N,3] float32 on the device, in the LiDAR
    frame (rows may hold NaN), ``l2w`` LiDAR -> world ([3,4] or [4,4], host).  A point counts when it is live and
    visible, exactly as ``seed.seed_sweep`` decides it (no NaN, ``z_lidar > min_z``, in front of the camera, inside the
    image), and its camera depth is at most ``max_depth``.  After all sweeps a return survives when no return within
    ``radius`` pixels (a square window clipped to the image) is nearer by more than the fraction ``rel_tol``: the LiDAR
    sits above the camera and sees background between foreground returns, which the camera does not.  ``radius=0``
    keeps every return.

    One fill, one launch per sweep and one filter launch on the current stream; no host read.  The nearest return wins
    by an integer atomic minimum, so the result is bit-identical from run to run and does not depend on how the points
    are split into sweeps.  A level of the coarse-to-fine schedule is a call with ``pyramid.scaled_camera``'s intrinsics
    and size in ``cam``."""
    if isinstance(sweeps, tuple) and len(sweeps) == 2 and isinstance(sweeps[0], torch.Tensor):
        sweeps = [sweeps]
    sweeps = list(sweeps)
    if not sweeps:
        raise ValueError("sweeps must hold at least one (points, l2w) pair")
    if not isinstance(cam, _seed.SeedCamera):
        raise ValueError(f"cam must be a SeedCamera, got {type(cam).__name__}")
    w, h = int(cam.width), int(cam.height)
    if not (1 <= w <= _seed.MAX_IMAGE_DIM and 1 <= h <= _seed.MAX_IMAGE_DIM):
        raise ValueError(f"the image size must be within [1, {_seed.MAX_IMAGE_DIM}], got {w} x {h}")
    if int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"radius must be an integer within [0, {MAX_RADIUS}], got {radius}")
    if not 0.0 <= float(rel_tol) < 1.0:
        raise ValueError(f"rel_tol must be within [0, 1), got {rel_tol}")
    if not float(max_depth) > 0.0:
        raise ValueError(f"max_depth must be positive, got {max_depth}")
    host = []
    for k, pair in enumerate(sweeps):
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError(f"sweep {k} must be a (points, l2w) pair")
        _validate_sweep(k, pair[0])
        host.append((pair[0], _seed._host_matrix(f"sweep {k}: l2w", pair[1])))
    w2c32 = _seed._host_matrix("cam.w2c", cam.w2c)
    dev = host[0][0].device
    for k, (pts, _) in enumerate(host):
        if not pts.is_cuda:
            raise ValueError(f"sweep {k}: points must be a device tensor; there is no CPU fallback")
        if pts.device != dev:
            raise ValueError(f"the sweeps live on different devices: {dev}, {pts.device}")
    host = [(pts.contiguous(), m) for pts, m in host]
    L.require_device(*(p for p, _ in host))
    c = L.SeedCam()
    c.w2c[:] = w2c32.reshape(-1).tolist()
    c.fx, c.fy, c.cx, c.cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
    c.width, c.height = w, h
    lib = L.load()
    depth = torch.empty(h, w, dtype=torch.float32, device=dev)
    out = torch.empty(h, w, dtype=torch.float32, device=dev)
    L.check(lib.sgn_lidar_depth_begin(L.ptr(depth), h, w, L.stream_ptr()), "sgn_lidar_depth_begin")
    for pts, l2w32 in host:
        L.check(lib.sgn_lidar_depth_splat(pts.shape[0], L.ptr(pts), l2w32.ctypes.data, float(min_z), float(max_depth),
                                          L.C.addressof(c), L.ptr(depth), L.stream_ptr()), "sgn_lidar_depth_splat")
    L.check(lib.sgn_lidar_depth_finish(L.ptr(depth), h, w, int(radius), float(np.float32(rel_tol)), L.ptr(out),
                                       L.stream_ptr()), "sgn_lidar_depth_finish")
    return out


def _hw(t, what: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch.Tensor, got {type(t).__name__}")
    if t.dim() == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "(H, W)" if shape is None else f"{tuple(shape)}"
        raise ValueError(f"{what} must have shape {want}, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    return t


def check_target(target, h: int, w: int) -> None:
    """Host-side validation of a depth target for an ``h`` x ``w`` image, before anything is launched."""
    _hw(target, "lidar_depth", (h, w))


def _inputs(dsum, alpha, target, mask):
    dsum = _hw(dsum, "dsum")
    H, W = (int(s) for s in dsum.shape)
    if not (1 <= W <= _seed.MAX_IMAGE_DIM and 1 <= H <= _seed.MAX_IMAGE_DIM):
        raise ValueError(f"the image size must be within [1, {_seed.MAX_IMAGE_DIM}], got {W} x {H}")
    alpha, target = _hw(alpha, "alpha", (H, W)), _hw(target, "target", (H, W))
    mask_c = None
    if mask is not None:
        check_mask(mask, H, W)
        mask_c = _mask_bytes(mask)
    return dsum, alpha, target.detach().contiguous(), mask_c, H, W


class _DepthLoss(Function):
    @staticmethod
    def forward(ctx, dsum, alpha, target, kind, mask):
        dev = L.require_device(dsum, alpha, target, mask)
        H, W = (int(s) for s in dsum.shape)
        dsum_c, alpha_c = dsum.detach().contiguous(), alpha.detach().contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev)
        L.check(L.load().sgn_depth_loss_fwd(H, W, L.ptr(dsum_c), L.ptr(alpha_c), L.ptr(target), L.ptr(mask), kind,
                                            L.ptr(loss), L.ptr(count), L.ptr(ws), ws.numel(), L.stream_ptr()),
                "sgn_depth_loss_fwd")
        ctx.kind, ctx.has_mask = kind, mask is not None
        ctx.save_for_backward(dsum_c, alpha_c, target, count, *(() if mask is None else (mask,)))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, v_loss):
        dsum, alpha, target, count = ctx.saved_tensors[:4]
        mask = ctx.saved_tensors[4] if ctx.has_mask else None
        H, W = (int(s) for s in dsum.shape)
        v_dsum, v_alpha = torch.empty_like(dsum), torch.empty_like(alpha)
        v_loss_c = v_loss.detach().to(torch.float32).contiguous().reshape(1)
        L.check(L.load().sgn_depth_loss_bwd(H, W, L.ptr(dsum), L.ptr(alpha), L.ptr(target), L.ptr(mask), ctx.kind,
                                            L.ptr(v_loss_c), L.ptr(count), L.ptr(v_dsum), L.ptr(v_alpha),
                                            L.stream_ptr()), "sgn_depth_loss_bwd")
        return v_dsum, v_alpha, None, None, None


def depth_loss(dsum: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, kind: str = "l1",
               mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The LiDAR depth term on the pair ``features.expected_depth`` returns, a scalar on the device.

    With ``D = dsum / alpha`` and ``z = target`` (``[H,W]`` float32, ``0`` = no return, as ``splat_depth`` makes it) a
    pixel counts when ``z > 0``, ``alpha > 1e-3`` (the reference's validity rule for its depth output,
    ``sgn_splatfacto.py:995``), ``dsum > 0`` and — with ``mask`` (bool / uint8 ``[H,W]`` or ``[H,W,1]``, non-zero = keep,
    as ``loss.check_mask``) — it is kept.  ``kind="l1"``: the mean of ``|D - z|`` over the counted pixels;
    ``kind="inverse"``: the mean of ``|1/D - 1/z|``.  One kernel and a one-thread launch forward, one kernel backward;
    the count stays on the device.  Gradients go to ``dsum`` and ``alpha`` only; an image without a counted pixel gives
    loss 0 and zero gradients."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    dsum, alpha, target_c, mask_c, _, _ = _inputs(dsum, alpha, target, mask)
    return _DepthLoss.apply(dsum, alpha, target_c, KINDS[kind], mask_c)


def depth_metrics(dsum: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor,
                  mask: Optional[torch.Tensor] = None) -> dict:
    """Evaluation depth figures over the pixels ``depth_loss`` counts, in one launch and one host read: ``abs_rel``
    (mean ``|D - z| / z``), ``rmse``, ``mae``, ``delta1`` (the share with ``max(D / z, z / D) < 1.25``) as floats and
    ``count`` as an int; all 0 without a counted pixel."""
    dsum, alpha, target_c, mask_c, H, W = _inputs(dsum, alpha, target, mask)
    dev = L.require_device(dsum, alpha, target_c, mask_c)
    dsum_c, alpha_c = dsum.detach().contiguous(), alpha.detach().contiguous()
    out = torch.empty(5, dtype=torch.float32, device=dev)
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev)
    L.check(L.load().sgn_depth_metrics(H, W, L.ptr(dsum_c), L.ptr(alpha_c), L.ptr(target_c), L.ptr(mask_c), L.ptr(out),
                                       L.ptr(ws), ws.numel(), L.stream_ptr()), "sgn_depth_metrics")
    abs_rel, rmse, mae, delta1, count = out.tolist()            # the one host read
    return {"abs_rel": abs_rel, "rmse": rmse, "mae": mae, "delta1": delta1, "count": int(count)}

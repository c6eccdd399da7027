"""Rolling-shutter rendering: a per-Gaussian screen-space shear directly behind the projection.

A street camera reads its sensor line by line over tens of milliseconds while the vehicle (and the tracked objects)
move; the ground truth is therefore sheared by several pixels, most at the image borders.  To first order a Gaussian's
centre crosses the image at a constant velocity during the readout, and what the rolling sensor records of it is again
an exact Gaussian with a shifted centre and a sheared conic — so the whole correction is one streaming pass
(``csrc/rolling_shutter.hip``; the fp32 contract is in ``include/sgn_rast.h``, "ROLLING SHUTTER") over the projection's
``xys, depths, radii, conics, num_tiles_hit``.  Binning, the rasterizers, the depth and feature passes, absgrad and
densification run unchanged on what comes out.

Out of scope: the batched views (``sgn_rast.views``, ``train_step_views``), ``step.render_scene_graph_eval``, the
per-line rotation of the sky lookup and of the SH view directions, object ANGULAR velocity, learnable velocities (they
are data: no gradient), and the data-parallel exchange (there is nothing to exchange).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import torch
from torch.autograd import Function

from . import _lib as L
from . import ops as _ops
from .ops import _f32c, _i32c

AXES = {"rows": L.SHUTTER_ROWS, "cols": L.SHUTTER_COLS}


def _vec3(name: str, v) -> tuple:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().reshape(-1).tolist()
    v = tuple(float(c) for c in v)
    if len(v) != 3 or not all(math.isfinite(c) for c in v):
        raise ValueError(f"{name} must be three finite numbers, got {v!r}")
    return v


class RollingShutter:
    """The sensor's motion during one readout.  ``lin_vel`` [m/s] and ``ang_vel`` [rad/s] are the camera's linear and
    angular velocity in WORLD axes, ``duration`` the signed readout time T in seconds (``> 0``: top to bottom, or left
    to right; ``< 0``: reversed), ``axis`` ``"rows"`` or ``"cols"``: line ``c`` of that axis is read at
    ``T * (c / extent - 0.5)`` around the camera's (mid-exposure) pose.  ``margin`` (pixels): the projection runs on an
    image padded by that much on every side, so that a Gaussian just off the image at mid-exposure can still be moved
    onto the border lines; two side effects when it is not 0 — the projection's ``1.3 * tan(fov / 2)`` Jacobian clamp is
    taken from the padded size, and ``xys`` carries the rounding of adding and subtracting the margin.
    Validated here, on the host: a bad axis, a non-finite value or a negative margin raises ``ValueError``."""

    def __init__(self, lin_vel: Sequence[float], ang_vel: Sequence[float], duration: float, axis: str = "rows",
                 margin: int = 16):
        self.lin_vel = _vec3("lin_vel", lin_vel)
        self.ang_vel = _vec3("ang_vel", ang_vel)
        if isinstance(duration, bool) or not isinstance(duration, (int, float)) or not math.isfinite(duration):
            raise ValueError(f"duration must be a finite number of seconds, got {duration!r}")
        self.duration = float(duration)
        if axis not in AXES:
            raise ValueError(f"axis must be \"rows\" or \"cols\", got {axis!r}")
        self.axis = axis
        if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
            raise ValueError(f"margin must be a non-negative integer number of pixels, got {margin!r}")
        self.margin = margin

    def __repr__(self) -> str:
        return (f"RollingShutter(lin_vel={self.lin_vel}, ang_vel={self.ang_vel}, duration={self.duration}, "
                f"axis={self.axis!r}, margin={self.margin})")


def check(rs) -> Optional[RollingShutter]:
    """``rolling_shutter=`` of the :mod:`sgn_rast.step` entries: None or a :class:`RollingShutter` (``ValueError``)."""
    if rs is not None and not isinstance(rs, RollingShutter):
        raise ValueError(f"rolling_shutter must be a sgn_rast.shutter.RollingShutter or None, got {type(rs).__name__}")
    return rs


def projection_frame(cam, rs: Optional[RollingShutter]):
    """(cx, cy, img_height, img_width) the projection runs with: the camera's own, or the margin-padded virtual image."""
    if rs is None or rs.margin == 0:
        return cam.cx, cam.cy, cam.height, cam.width
    m = rs.margin
    return cam.cx + m, cam.cy + m, cam.height + 2 * m, cam.width + 2 * m


_ROT: dict = {}


def _cam_rotation(cam) -> torch.Tensor:
    """``cam.viewmat[:3, :3]`` as a CPU float64 tensor; one read-back per view matrix, not per call (the entry HOLDS
    the tensor, so "same address, same version" means "same bytes")."""
    vm = cam.viewmat
    if not vm.is_cuda:
        return vm[:3, :3].detach().to(torch.float64)
    key = (vm.data_ptr(), vm._version)
    hit = _ROT.get(key)
    if hit is None or hit[0] is not vm:
        if len(_ROT) > 64:
            _ROT.clear()
        hit = _ROT[key] = (vm, vm[:3, :3].detach().to("cpu", torch.float64))
    return hit[1]


_DEV_CONST: dict = {}


def _device_constants(cam, rs: RollingShutter, device):
    """(R^T [3,3], v_cam [1,3]) float32 on ``device`` for the per-object table, uploaded once per (view matrix, shutter)
    rather than per call (the entry holds both objects, as above)."""
    vm = cam.viewmat
    key = (vm.data_ptr(), vm._version, id(rs), str(device))
    hit = _DEV_CONST.get(key)
    if hit is None or hit[0] is not vm or hit[1] is not rs or hit[2] != rs.lin_vel:
        if len(_DEV_CONST) > 64:
            _DEV_CONST.clear()
        hit = _DEV_CONST[key] = (vm, rs, rs.lin_vel, _cam_rotation(cam).to(torch.float32).T.contiguous().to(device),
                                 torch.tensor([rs.lin_vel], dtype=torch.float32).to(device))
    return hit[3], hit[4]


def camera_twist(cam, rs: RollingShutter):
    """The constant camera-frame twist ``(R v_cam, R w_cam)``, ``R = cam.viewmat[:3, :3]`` -> two float64 [3]."""
    R = _cam_rotation(cam)
    return R @ torch.tensor(rs.lin_vel, dtype=torch.float64), R @ torch.tensor(rs.ang_vel, dtype=torch.float64)


def viewmat_at(cam, rs: RollingShutter, t: float) -> torch.Tensor:
    """The exact world-to-camera matrix [4,4] at time ``t`` (seconds from mid-exposure) of a camera that moves with the
    constant camera-frame twist of :func:`camera_twist`: ``Exp(-t * twist) @ cam.viewmat``, in ``cam.viewmat``'s dtype
    and on its device (computed in float64 on the host).  Line ``c`` of the shutter axis is read at
    ``rs.duration * (c / extent - 0.5)``."""
    l, w = camera_twist(cam, rs)
    xi = torch.zeros(4, 4, dtype=torch.float64)
    xi[0, 1], xi[0, 2], xi[1, 2] = -w[2], w[1], -w[0]
    xi[1, 0], xi[2, 0], xi[2, 1] = w[2], -w[1], w[0]
    xi[:3, 3] = l
    vm = cam.viewmat
    full = torch.eye(4, dtype=torch.float64)
    full[:vm.shape[0]] = vm.detach().to("cpu", torch.float64)
    out = torch.linalg.matrix_exp(-float(t) * xi) @ full
    return out.to(vm.dtype).to(vm.device)


def _struct(cam, rs: RollingShutter, block_width: int, clip_thresh: float) -> L.Shutter:
    l, w = camera_twist(cam, rs)
    s = L.Shutter()
    s.fx, s.fy, s.cx, s.cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
    s.lin[:] = [float(c) for c in l]
    s.ang[:] = [float(c) for c in w]
    s.duration, s.margin, s.clip_thresh = rs.duration, float(rs.margin), float(clip_thresh)
    s.axis, s.img_h, s.img_w, s.block_width = AXES[rs.axis], int(cam.height), int(cam.width), int(block_width)
    s.semantics = _ops.semantics().flags()
    return s


class _Shear(Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, object_ids, lin_table, st):
        dev = L.require_device(xys, depths, radii, conics, object_ids, lin_table)
        n = xys.shape[0]
        xys_c, depths_c, radii_c, conics_c = _f32c(xys), _f32c(depths), _i32c(radii), _f32c(conics)
        f32 = dict(dtype=torch.float32, device=dev)
        xys_o, depths_o, conics_o = torch.empty(n, 2, **f32), torch.empty(n, **f32), torch.empty(n, 3, **f32)
        radii_o = torch.empty(n, dtype=torch.int32, device=dev)
        nth_o = torch.empty(n, dtype=torch.int32, device=dev)
        m = 0 if lin_table is None else int(lin_table.shape[0])
        L.check(L.load().sgn_rolling_shutter_fwd(n, L.ptr(xys_c), L.ptr(depths_c), L.ptr(radii_c), L.ptr(conics_c),
                                                 L.ptr(object_ids), L.ptr(lin_table), m, C.byref(st), L.ptr(xys_o),
                                                 L.ptr(depths_o), L.ptr(radii_o), L.ptr(conics_o), L.ptr(nth_o),
                                                 L.stream_ptr()), "sgn_rolling_shutter_fwd")
        ctx.st, ctx.m = st, m
        ctx.save_for_backward(xys_c, depths_c, conics_c, radii_o, object_ids, lin_table)
        ctx.mark_non_differentiable(radii_o, nth_o)
        ctx.set_materialize_grads(False)
        return xys_o, depths_o, radii_o, conics_o, nth_o

    @staticmethod
    def backward(ctx, v_xys_o, v_depths_o, _v_radii, v_conics_o, _v_nth):
        if (v_xys_o is None and v_depths_o is None and v_conics_o is None) or not any(ctx.needs_input_grad[:4]):
            return (None,) * 7
        xys, depths, conics, radii_o, object_ids, lin_table = ctx.saved_tensors
        n, f32 = xys.shape[0], dict(dtype=torch.float32, device=xys.device)
        v_xys_o = torch.zeros(n, 2, **f32) if v_xys_o is None else _f32c(v_xys_o)
        v_conics_o = torch.zeros(n, 3, **f32) if v_conics_o is None else _f32c(v_conics_o)
        v_depths_o = None if v_depths_o is None else _f32c(v_depths_o)
        v_xys, v_depths, v_conics = torch.empty(n, 2, **f32), torch.empty(n, **f32), torch.empty(n, 3, **f32)
        L.check(L.load().sgn_rolling_shutter_bwd(n, L.ptr(xys), L.ptr(depths), L.ptr(conics), L.ptr(radii_o),
                                                 L.ptr(object_ids), L.ptr(lin_table), ctx.m, C.byref(ctx.st),
                                                 L.ptr(v_xys_o), L.ptr(v_depths_o), L.ptr(v_conics_o), L.ptr(v_xys),
                                                 L.ptr(v_depths), L.ptr(v_conics), L.stream_ptr()),
                "sgn_rolling_shutter_bwd")
        return v_xys, v_depths, None, v_conics, None, None, None


def apply(xys, depths, radii, conics, num_tiles_hit, cam, rs: RollingShutter, block_width: int,
          object_ids: Optional[torch.Tensor] = None, object_velocities: Optional[torch.Tensor] = None,
          clip_thresh: float = 0.01):
    """The projection's ``xys, depths, radii, conics, num_tiles_hit`` -> the same five as the rolling sensor ``rs`` of
    camera ``cam`` records them (the contract is in ``include/sgn_rast.h``): centres moved to where the shutter meets
    them, conics sheared, radii grown conservatively (``ceil(r * sigma)``, never below the sheared footprint's 3-sigma
    radius, and exactly ``r`` when nothing moves), tiles recounted on ``cam``'s own grid.  A row the pass culls (it
    nearly keeps pace with the shutter, ends behind the clip plane or off the image) holds zeros like a row the
    projection culled, and gets zero gradients.  The projection must have run on :func:`projection_frame` of
    ``(cam, rs)``; ``num_tiles_hit`` itself is not read (it is recomputed).  ``object_ids`` int32 [N] with
    ``object_velocities`` [M,3]: the WORLD linear velocity of every pose-table entry (zero for the background); a
    Gaussian of object k then moves with ``v_cam - object_velocities[k]`` relative to the camera.  Gradients reach
    ``xys``, ``depths`` and ``conics`` through the analytic backward kernel; the velocities are data."""
    if not isinstance(rs, RollingShutter):
        raise ValueError(f"rs must be a RollingShutter, got {type(rs).__name__}")
    if (object_ids is None) != (object_velocities is None):
        raise ValueError("object_ids and object_velocities go together")
    if xys.dim() != 2 or xys.shape[1] != 2 or conics.shape != (xys.shape[0], 3) or depths.shape != xys.shape[:1] \
            or radii.shape != xys.shape[:1]:
        raise ValueError("xys [N,2], depths [N], radii [N] and conics [N,3] expected")
    lin_table = None
    if object_velocities is not None:
        if object_velocities.dim() != 2 or object_velocities.shape[1] != 3 or object_velocities.shape[0] < 1:
            raise ValueError(f"object_velocities must be [M,3], got {tuple(object_velocities.shape)}")
        if object_ids.shape != xys.shape[:1]:
            raise ValueError("object_ids must hold one id per row")
        R_t, v_cam = _device_constants(cam, rs, xys.device)
        v_rel = v_cam - object_velocities.detach().to(xys.device, torch.float32)
        lin_table = (v_rel @ R_t).contiguous()                 # l_k = R (v_cam - v_obj[k])
        object_ids = _i32c(object_ids)
    st = _struct(cam, rs, block_width, clip_thresh)
    return _Shear.apply(xys, depths, radii, conics, object_ids, lin_table, st)

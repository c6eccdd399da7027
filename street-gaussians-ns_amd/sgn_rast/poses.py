"""Learnable tracked-object poses for the fused scene graph (the reference's ``BBoxOptimizer``,
``data/utils/bbox_optimizers.py``, configured by ``BBoxOptimizerConfig``: ``mode="simple"`` in ``sgn_config.py:45``,
parameter group ``"bbox_opt"`` at ``sgn_config.py:80-83``).

:class:`ObjectPoses` keeps the per-(frame, track) corrections and builds the ``[M,16]`` pose table of
:func:`sgn_rast.step.render_scene_graph` from the original box annotations with differentiable torch ops on the device;
the fused projection's backward (``csrc/project.hip``, ``sgn_project_bwd_fused_pose``) returns the table's gradient, and
:func:`pose_rows` carries it back to the corrections.

Three defects of the reference are deliberately NOT reproduced:

- the detach: ``apply_to_bbox`` (``:140-166``) writes the corrected pose back through ``.detach().numpy()``, so no
  gradient ever reaches the pose parameters;
- the accumulation: ``apply_to_bbox`` mutates the annotation in place, so the correction is applied again on every visit
  to a frame; here it is applied to the original annotation each time;
- the regulariser axis: ``get_loss_dict`` (``:168``) takes ``pose_adjustment[:, :3]`` of a ``[frames, boxes, 6]`` tensor,
  which slices the box axis; here the norms run over the last axis (translation part, rotation part).  In ``"simple"``
  mode the reference reads a parameter that does not exist; here the regulariser is 0 there.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

MODES = ("off", "SO3xR3", "SE3", "simple")


def _skew(w: torch.Tensor) -> torch.Tensor:
    """[...,3] -> [...,3,3] cross-product matrices."""
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1),
                        torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def exp_map_SO3xR3(tangent: torch.Tensor) -> torch.Tensor:
    """[...,6] (translation, axis-angle) -> [...,3,4]: Rodrigues' rotation of the last three, the first three as the
    translation.  The squared angle is clamped at 1e-4 as nerfstudio's ``exp_map_SO3xR3`` does."""
    w = tangent[..., 3:]
    ang = torch.clamp((w * w).sum(-1), min=1e-4).sqrt()
    inv = 1.0 / ang
    fac1, fac2 = inv * ang.sin(), inv * inv * (1.0 - ang.cos())
    K = _skew(w)
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)
    R = fac1[..., None, None] * K + fac2[..., None, None] * (K @ K) + eye
    return torch.cat([R, tangent[..., :3, None]], -1)


def exp_map_SE3(tangent: torch.Tensor) -> torch.Tensor:
    """[...,6] (rho, omega) -> [...,3,4] = exp of the twist [[omega]x rho; 0 0]: R = I + A K + B K^2, t = V rho with
    V = I + B K + C K^2, A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3.  Below t = 1e-2 the three come from
    their Taylor series in t^2 (no square root there, so the gradient at the zero twist is finite)."""
    rho, w = tangent[..., :3], tangent[..., 3:]
    th2 = (w * w).sum(-1)
    small = th2 < 1e-4
    th = torch.where(small, torch.ones_like(th2), th2).sqrt()
    th2s = torch.where(small, torch.ones_like(th2), th2)
    A = torch.where(small, 1.0 - th2 / 6.0 + th2 * th2 / 120.0, th.sin() / th)
    B = torch.where(small, 0.5 - th2 / 24.0 + th2 * th2 / 720.0, (1.0 - th.cos()) / th2s)
    C = torch.where(small, 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0, (th - th.sin()) / (th2s * th))
    K = _skew(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)
    R = eye + A[..., None, None] * K + B[..., None, None] * K2
    V = eye + B[..., None, None] * K + C[..., None, None] * K2
    return torch.cat([R, (V @ rho[..., None])], -1)


def quat_from_rot(R: torch.Tensor) -> torch.Tensor:
    """[K,3,3] -> [K,4] wxyz with the branch order of :func:`sgn_rast.fused.make_pose_table` (trace > 0, else the
    largest diagonal entry, first on ties), batched with ``torch.where``.  Every branch's square root is taken of a
    clamped argument, so the branches not taken stay finite and pass no NaN into the gradient."""
    r = lambda a, b: R[:, a, b]
    tr = r(0, 0) + r(1, 1) + r(2, 2)
    st = (torch.clamp(tr + 1.0, min=1e-12)).sqrt() * 2
    q_tr = torch.stack([0.25 * st, (r(2, 1) - r(1, 2)) / st, (r(0, 2) - r(2, 0)) / st, (r(1, 0) - r(0, 1)) / st], -1)
    cands = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        s = (torch.clamp(r(i, i) - r(j, j) - r(k, k) + 1.0, min=1e-12)).sqrt() * 2
        v = [None, None, None]
        v[i] = 0.25 * s
        v[j] = (r(j, i) + r(i, j)) / s
        v[k] = (r(k, i) + r(i, k)) / s
        cands.append(torch.stack([(r(k, j) - r(j, k)) / s, v[0], v[1], v[2]], -1))
    d0, d1, d2 = r(0, 0), r(1, 1), r(2, 2)
    pick0 = (d0 >= d1) & (d0 >= d2)                  # torch.argmax: the first maximum
    pick1 = ~pick0 & (d1 >= d2)
    q_diag = torch.where(pick0[:, None], cands[0], torch.where(pick1[:, None], cands[1], cands[2]))
    return torch.where((tr > 0)[:, None], q_tr, q_diag)


def pose_rows(rot: torch.Tensor, center: torch.Tensor) -> torch.Tensor:
    """[K,3,3] object->world rotations + [K,3] centres -> [K,16] pose-table rows (R row-major, t, q_o2w wxyz),
    differentiable.  Evaluated in float64 and returned in the input dtype, so float32 rows equal
    :func:`sgn_rast.fused.make_pose_table`'s."""
    R = rot.to(torch.float64)
    q = quat_from_rot(R)
    out = torch.cat([R.reshape(-1, 9), center.to(torch.float64).reshape(-1, 3), q], 1)
    return out.to(rot.dtype)


def quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Hamilton product, wxyz, real part first (pytorch3d ``quaternion_multiply`` without its sign standardisation)."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def quat_matrix(q: torch.Tensor) -> torch.Tensor:
    """[K,4] wxyz (any norm) -> [K,3,3], as nerfstudio's ``quaternion_matrix`` (normalises first)."""
    q = q * (2.0 / (q * q).sum(-1, keepdim=True)).sqrt()
    w, x, y, z = q.unbind(-1)
    return torch.stack([torch.stack([1.0 - y * y - z * z, x * y - z * w, x * z + y * w], -1),
                        torch.stack([x * y + z * w, 1.0 - x * x - z * z, y * z - x * w], -1),
                        torch.stack([x * z - y * w, y * z + x * w, 1.0 - x * x - y * y], -1)], -2)


class ObjectPoses(torch.nn.Module):
    """Per-(frame, track) pose corrections of the scene graph's object boxes, in the modes of ``BBoxOptimizerConfig``:

    - ``"off"``: no parameters, boxes as annotated;
    - ``"SO3xR3"`` / ``"SE3"``: ``pose_adjustment`` [F,T,6] (translation, rotation); with ``C = exp(adj)``:
      ``R' = C[:3,:3] R`` and ``center' = center + C[:3,3]`` (``apply_to_bbox``);
    - ``"simple"``: ``delta_center`` [F,T,3] and ``delta_yaw`` [F,T]; ``center' = center + delta_center`` and
      ``q' = q_box (x) (cos psi, 0, 0, sin psi)``, as the reference writes it.

    Tracks listed in ``non_trainable`` get the identity correction (and so no gradient).  Everything runs as batched
    device ops on the ``K`` boxes of a frame, with no device-to-host transfer."""

    def __init__(self, num_frames: int, num_tracks: int, mode: str = "off", device="cpu",
                 non_trainable: Optional[List[int]] = None, center_l2_penalty: float = 1e-2,
                 rot_l2_penalty: float = 1e-3):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.mode = mode
        self.center_l2_penalty, self.rot_l2_penalty = float(center_l2_penalty), float(rot_l2_penalty)
        trainable = torch.ones(num_tracks, dtype=torch.bool)
        if non_trainable is not None:
            trainable[torch.as_tensor(list(non_trainable), dtype=torch.long)] = False
        self.register_buffer("trainable", trainable.to(device))
        if mode in ("SO3xR3", "SE3"):
            self.pose_adjustment = torch.nn.Parameter(torch.zeros(num_frames, num_tracks, 6, device=device))
        elif mode == "simple":
            self.delta_center = torch.nn.Parameter(torch.zeros(num_frames, num_tracks, 3, device=device))
            self.delta_yaw = torch.nn.Parameter(torch.zeros(num_frames, num_tracks, device=device))

    def param_groups(self) -> Dict[str, list]:
        return {"bbox_opt": list(self.parameters())}

    def apply(self, frame_idx, track_idx, centers: torch.Tensor, rots: torch.Tensor):
        """Corrected ``(centers [K,3], rots [K,3,3])`` of the boxes ``track_idx`` [K] in frames ``frame_idx`` (a scalar
        or [K]), from the ORIGINAL annotation ``centers`` / ``rots``; differentiable w.r.t. the parameters."""
        centers, rots = centers.to(torch.float64), rots.to(torch.float64)
        if self.mode == "off":
            return centers, rots
        keep = self.trainable[track_idx]
        if self.mode == "simple":
            dc = torch.where(keep[:, None], self.delta_center[frame_idx, track_idx], 0.0).to(torch.float64)
            psi = torch.where(keep, self.delta_yaw[frame_idx, track_idx], 0.0).to(torch.float64)
            z = torch.zeros_like(psi)
            q = quat_mul(quat_from_rot(rots), torch.stack([psi.cos(), z, z, psi.sin()], -1))
            return centers + dc, torch.where(keep[:, None, None], quat_matrix(q), rots)
        exp = exp_map_SO3xR3 if self.mode == "SO3xR3" else exp_map_SE3
        C = exp(self.pose_adjustment[frame_idx, track_idx].to(torch.float64))
        eye = torch.eye(4, dtype=torch.float64, device=C.device)[:3]
        C = torch.where(keep[:, None, None], C, eye)
        return centers + C[:, :, 3], C[:, :, :3] @ rots

    def table(self, frame_idx, track_idx, centers: torch.Tensor, rots: torch.Tensor) -> torch.Tensor:
        """float32 [K+1,16] pose table for :func:`sgn_rast.step.render_scene_graph`: row 0 the background (identity, no
        gradient), row k+1 the corrected box k."""
        c, R = self.apply(frame_idx, track_idx, centers, rots)
        R = torch.cat([torch.eye(3, dtype=R.dtype, device=R.device)[None], R])
        c = torch.cat([torch.zeros(1, 3, dtype=c.dtype, device=c.device), c])
        return pose_rows(R, c).to(torch.float32).contiguous()

    def regularizer(self) -> torch.Tensor:
        """Opt-in L2 penalty with the reference's weights, over the LAST axis: ``center_l2_penalty`` times the mean norm
        of the translation part plus ``rot_l2_penalty`` times that of the rotation part.  0 in ``"off"`` / ``"simple"``."""
        if self.mode not in ("SO3xR3", "SE3"):
            return torch.zeros((), device=self.trainable.device)
        a = self.pose_adjustment
        return (a[..., :3].norm(dim=-1).mean() * self.center_l2_penalty
                + a[..., 3:].norm(dim=-1).mean() * self.rot_l2_penalty)

    @torch.no_grad()
    def corrected(self, frame_idx, track_idx, centers, rots):
        """Host numpy ``(centers [K,3], rots [K,3,3])`` float64 of the corrected boxes, for export (what
        ``apply_to_bbox`` writes into the annotation, without mutating anything)."""
        dev = self.trainable.device
        c, R = self.apply(torch.as_tensor(frame_idx, device=dev), torch.as_tensor(track_idx, device=dev),
                          torch.as_tensor(centers, device=dev), torch.as_tensor(rots, device=dev))
        return c.cpu().numpy(), R.cpu().numpy()

"""Nearest neighbours across two point clouds and the LiDAR chamfer metric (``csrc/cloud_nn.hip``).

The reference's only geometric measure of a fit is ``evaluate_lidar_geometric``
(``street_gaussians_ns/data/utils/geometric_metric.py:72-100``): the mean distance from every Gaussian centre to the
nearest point of the aggregated LiDAR cloud and the mean of the reverse direction, in units of ``CD_UNIT``
(``calc_chamfer_distance``, ``:59-69``), computed with two open3d KD-tree sweeps on the CPU.  Here both directions run
on the device:

* ``nearest(query, target)``          device tensors in, ``(dist [Nq] f32, idx [Nq] int64)`` out, on the current stream;
* ``chamfer_distance(pred, gt)``      the two means over ``CD_UNIT`` as Python floats, device tensors in;
* ``calc_chamfer_distance(pred, gt)`` the reference function's contract (numpy in, the same tuple out), for
  ``geometric_metric.calc_chamfer_distance = sgn_rast.geometry.calc_chamfer_distance``;
* ``filter_lidar`` / ``lidar_to_scene``  the row filters of ``read_pcd_file`` (``:36-48``) and the world -> scene
  arithmetic of ``evaluate_lidar_geometric`` (``:86-92``);
* ``evaluate_lidar_geometric(means, lidar_points, ...)``  the reference's three result keys from arrays (reading the
  point-cloud file stays with the caller).

open3d's ``compute_point_cloud_distance`` is by definition the exact distance to the nearest point of the other cloud,
which is what the search returns; the agreement is by that definition, not by a run against open3d (it is neither
vendored nor required).  The search takes float32 coordinates where the reference computes in float64: a cloud is rounded
once to float32 (at most half an ulp of its largest coordinate per axis) before distances are taken.  On equal distances
the INDEX is one of the nearest rows, this library's choice.  Results are bit-identical from run to run.  No autograd,
no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

CD_UNIT = 1e-4


def _validate(name, x):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, got {type(x).__name__}")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name} must have shape (N, 3), got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {x.dtype}")
    n = x.shape[0]
    if n < 1:
        raise ValueError(f"{name} is empty: need at least one point")
    if n > (1 << 30):
        raise ValueError(f"at most 2**30 points, {name} has {n}")


def nearest(query: torch.Tensor, target: torch.Tensor, visited: torch.Tensor | None = None):
    """For every row of ``query`` [Nq,3] the nearest row of ``target`` [Nt,3] (both float32, finite, on the device).

    Returns ``(dist [Nq] float32, idx [Nq] int64)``; no row is excluded, the clouds are unrelated.  ``visited``
    (optional int64 device tensor of one element) is increased by the number of candidate distances evaluated.  One
    host read: the finiteness check of both clouds.
    """
    _validate("query", query)
    _validate("target", target)
    L.require_device(query, target, visited)
    if visited is not None and (visited.dtype != torch.int64 or visited.numel() < 1):
        raise ValueError("visited must be an int64 device tensor")
    if not bool(torch.isfinite(query).all() & torch.isfinite(target).all()):
        raise ValueError("query or target holds non-finite coordinates")
    qc, tc = query.contiguous(), target.contiguous()
    nq, nt = qc.shape[0], tc.shape[0]
    lib = L.load()
    dist = torch.empty(nq, dtype=torch.float32, device=query.device)
    idx = torch.empty(nq, dtype=torch.int32, device=query.device)
    ws = L.workspace(lib.sgn_cloud_nn_workspace_bytes(nt, nq), query.device)
    L.check(lib.sgn_cloud_nn(nt, L.ptr(tc), nq, L.ptr(qc), L.ptr(dist), L.ptr(idx), L.ptr(visited), L.ptr(ws),
                             ws.numel(), L.stream_ptr()), "sgn_cloud_nn")
    return dist, idx.to(torch.int64)


def chamfer_distance(pred: torch.Tensor, gt: torch.Tensor):
    """``(d1, d2)`` as Python floats: the mean distance from every row of ``pred`` to its nearest row of ``gt``, and
    from every row of ``gt`` to its nearest row of ``pred``, each over ``CD_UNIT`` (``geometric_metric.py:59-69``).
    The means are taken in float64 on the device."""
    d1 = nearest(pred, gt)[0].double().mean() / CD_UNIT
    d2 = nearest(gt, pred)[0].double().mean() / CD_UNIT
    both = torch.stack([d1, d2]).tolist()
    return both[0], both[1]


def _device():
    if not torch.cuda.is_available():
        raise L.SgnRastError("sgn_rast.geometry runs on the GPU; there is no CPU fallback")
    return torch.device("cuda", L.current_device())


def _on_device(a, dtype):
    """A tensor or array as a detached tensor of `dtype` on the current device (a device tensor stays where it is)."""
    t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    return t.to(device=t.device if t.is_cuda else _device(), dtype=dtype)


def calc_chamfer_distance(pred: np.ndarray, gt: np.ndarray):
    """Drop-in for ``calc_chamfer_distance`` (``geometric_metric.py:59-69``): numpy arrays [N,3] in, ``(d1, d2)`` out.
    The arrays are moved to the current device as float32; the search itself never runs on the CPU."""
    assert isinstance(gt, np.ndarray) and isinstance(pred, np.ndarray)
    assert gt.shape[1] == 3 and pred.shape[1] == 3
    return chamfer_distance(_on_device(pred, torch.float32), _on_device(gt, torch.float32))


def filter_lidar(points: torch.Tensor, ignore_nan: bool = True, filter_ego: bool = True) -> torch.Tensor:
    """The two row filters of ``read_pcd_file`` (``geometric_metric.py:36-48``) on a device tensor [N,3], order kept:
    rows with any NaN are dropped, then rows inside the ego vehicle's box ``-1 < x < 3``, ``|y| < 1``, ``-1 < z < 2``
    (every inequality strict: a point on a face of the box stays)."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a tensor of shape (N, 3)")
    if ignore_nan:
        points = points[~torch.isnan(points).any(dim=1)]
    if filter_ego:
        x, y, z = points[:, 0], points[:, 1].abs(), points[:, 2]
        ego = (x < 3) & (x > -1) & (y < 1) & (z < 2) & (z > -1)
        points = points[~ego]
    return points


def lidar_to_scene(points, translation, transform, scale) -> torch.Tensor:
    """World-frame LiDAR points [N,3] in the model's scene frame, as ``evaluate_lidar_geometric`` moves them
    (``geometric_metric.py:86-92``): the dataparser's colmap translation ``(tx, ty, tz)`` is added as ``(ty, tx, -tz)``
    (the reference's ``gl2cv``: first two rows swapped, third negated), then ``R p + T`` with the dataparser transform
    ``[R | T]`` ([3,4] or [4,4]), then the dataparser scale.  Computed in float64 and rounded once to float32."""
    p = _on_device(points, torch.float64)
    t = _on_device(translation, torch.float64).reshape(3).to(p.device)
    m = _on_device(transform, torch.float64).to(p.device)
    if m.dim() != 2 or m.shape[1] != 4 or m.shape[0] not in (3, 4):
        raise ValueError(f"transform must have shape (3, 4) or (4, 4), got {tuple(m.shape)}")
    shift = torch.stack([t[1], t[0], -t[2]])
    out = (p + shift) @ m[:3, :3].T + m[:3, 3]
    return (out * float(scale)).to(torch.float32)


def evaluate_lidar_geometric(means, lidar_points, translation=None, transform=None, scale=1.0) -> dict:
    """The reference's LiDAR result (``geometric_metric.py:72-100``) from arrays: ``means`` [N,3] are the Gaussian
    centres (a tensor or array), ``lidar_points`` [M,3] the aggregated cloud as read from its file, unfiltered, in the
    world frame.  The cloud goes through ``filter_lidar`` and ``lidar_to_scene`` (``translation`` =
    ``applied_translation_in_colmap``, default zero; ``transform`` = ``dataparser_transform``, default identity;
    ``scale`` = ``dataparser_scale``), then both chamfer directions are taken."""
    translation = np.zeros(3) if translation is None else translation
    transform = np.eye(4)[:3] if transform is None else transform
    lidar = lidar_to_scene(filter_lidar(_on_device(lidar_points, torch.float64)), translation, transform, scale)
    d1, d2 = chamfer_distance(_on_device(means, torch.float32), lidar)
    return {"lidar_chamfer_distance_1": d1, "lidar_chamfer_distance_2": d2, "lidar_chamfer_distance_avg": (d1 + d2) / 2}

"""LiDAR seeding: the Gaussians a scene graph starts from, made on the device (``csrc/seed.hip``).

The reference makes its seed clouds in two offline scripts, each a Python ``for`` over every point of every sweep of
every camera with open3d's box test on the CPU:

* ``scripts/pythons/pcd2colmap_points3D.py:114-235``  the background: LiDAR points outside every moving box, coloured
  from the camera image they project into, in the world frame;
* ``scripts/pythons/extract_object_pts.py:114-273``   per tracked object: points inside its box scaled 1.1, coloured
  the same way, stored in the box's own frame.

``street_gaussians_ns/data/utils/dynamic_annotation.py:348-365`` loads those clouds ("fewer than 10 000 points is no
seed") and ``street_gaussians_ns/sgn_splatfacto.py:253-300`` turns them into parameters.  Here:

* ``seed_sweep(points, l2w, boxes, cam, image)``  one sweep against one camera and up to 64 boxes: device tensors in,
  ``(ObjectSeeds, BackgroundSeeds)`` out, on the current stream, one host read (the counts that size the outputs);
* ``make_boxes(centers, rots, extents)``          the box table of a call, with the reference's 1.1 scale;
* ``sweep_to_world(l2w, t0)``                     the LiDAR pose as the scripts use it (``extract_object_pts.py:157-166``);
* ``SeedAccumulator``                             the clouds over all (sweep, camera) pairs and the 10 000-point rule;
* ``init_gaussians(xyz, rgb255)``                 the parameter tensors of ``populate_modules``.

With ``knn.init_log_scales`` this completes ``seed -> init_log_scales -> train -> densify -> eval`` without open3d or
OpenCV.  Every output of ``seed_sweep`` is stable (input point order kept) and bit-identical from run to run; its
arithmetic is the contract of ``include/sgn_rast.h`` ("LiDAR SEEDING"), which ``tests/seed_oracle.py`` restates.

Deviations from the reference, all deliberate:

* float32 where the scripts compute in float64: box membership and the pixel can differ for points within rounding
  of a box face, of the camera plane or of a pixel edge (``tests/test_seed_oracle.py`` bounds who may differ: points
  within 5e-5 of a face or of ``pc.z = 0``, or whose pixel coordinate is within 5e-4 of an integer; under 1 % of the
  live points of its scenes);
* the background script's ``0 < v`` (``pcd2colmap_points3D.py``), which drops the top image row, is not reproduced:
  ``0 <= v`` holds for both kinds, as in the object script;
* the colour is the image's bytes in the caller's channel order (the scripts read BGR through OpenCV and keep it);
* the background script's random 10 000-point subsample per sweep stays with the caller, as do reading point-cloud
  and image files and undistorting images.

No autograd, no CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import knn

MAX_BOXES = L.SEED_MAX_BOXES
MAX_POINTS = 1 << 27
MAX_IMAGE_DIM = 16384
BOX_SCALE = 1.1                 # extract_object_pts.py:144-147
SH_C0 = 0.28209479177387814     # sgn_splatfacto.py:61


@dataclass
class SeedCamera:
    """The camera of a seeding call: ``w2c`` world -> camera ([3,4] or [4,4], host), pinhole intrinsics, image size."""
    w2c: object
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int


class ObjectSeeds(NamedTuple):
    """Rows of all boxes, box after box: rows ``offsets[b]:offsets[b + 1]`` belong to box b, in input point order."""
    local: torch.Tensor         # [M,3] float32, the point in its box's frame
    rgb: torch.Tensor           # [M,3] uint8
    src: torch.Tensor           # [M] int64, row of `points`
    offsets: list               # B + 1 ints, on the host


class BackgroundSeeds(NamedTuple):
    world: torch.Tensor         # [K,3] float32
    rgb: torch.Tensor           # [K,3] uint8
    src: torch.Tensor           # [K] int64
    n_live: int                 # points that passed the NaN / min_z / |x| filters, visible or not


def _host_matrix(name, m, rows=(3, 4)):
    a = np.asarray(m.detach().cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] not in rows:
        raise ValueError(f"{name} must have shape (3, 4) or (4, 4), got {a.shape}")
    return np.ascontiguousarray(a[:3].astype(np.float32))


def make_boxes(centers, rots, extents, scale: float = BOX_SCALE) -> np.ndarray:
    """The box table ``seed_sweep`` takes, float32 [B,15] on the host: per box ``center[3] | rot[9] | half[3]`` with
    ``rot`` the box -> world rotation, row-major, and ``half = extents * scale / 2`` (full side lengths in; the
    reference grows every box by 1.1, ``extract_object_pts.py:144-148``).  Computed in float64, rounded once."""
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(rots, dtype=np.float64).reshape(-1, 9)
    e = np.asarray(extents, dtype=np.float64).reshape(-1, 3)
    if not (c.shape[0] == r.shape[0] == e.shape[0]):
        raise ValueError(f"centers, rots and extents disagree on the number of boxes: {c.shape[0]}, {r.shape[0]}, {e.shape[0]}")
    return np.concatenate([c, r, e * (float(scale) * 0.5)], axis=1).astype(np.float32)


def _box_table(boxes) -> np.ndarray:
    if boxes is None:
        return np.zeros((0, 15), dtype=np.float32)
    a = np.asarray(boxes.detach().cpu() if isinstance(boxes, torch.Tensor) else boxes)
    if a.size == 0:
        return np.zeros((0, 15), dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 15:
        raise ValueError(f"boxes must have shape (B, 15) (center, rot, half: make_boxes), got {a.shape}")
    if a.shape[0] > MAX_BOXES:
        raise ValueError(f"at most {MAX_BOXES} boxes per call, got {a.shape[0]}")
    return np.ascontiguousarray(a, dtype=np.float32)


def _validate(points, image, cam):
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"points must be a torch.Tensor, got {type(points).__name__}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must have shape (N, 3), got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if not 1 <= points.shape[0] <= MAX_POINTS:
        raise ValueError(f"points must hold between 1 and 2**27 rows, got {points.shape[0]}")
    if not isinstance(image, torch.Tensor):
        raise ValueError(f"image must be a torch.Tensor, got {type(image).__name__}")
    if image.dtype != torch.uint8:
        raise ValueError(f"image must be uint8, got {image.dtype}")
    if not isinstance(cam, SeedCamera):
        raise ValueError(f"cam must be a SeedCamera, got {type(cam).__name__}")
    w, h = int(cam.width), int(cam.height)
    if not (1 <= w <= MAX_IMAGE_DIM and 1 <= h <= MAX_IMAGE_DIM):
        raise ValueError(f"the image size must be within [1, {MAX_IMAGE_DIM}], got {w} x {h}")
    if image.dim() != 3 or tuple(image.shape) != (h, w, 3):
        raise ValueError(f"image must have shape (height, width, 3) = ({h}, {w}, 3), got {tuple(image.shape)}")
    if not image.is_contiguous():
        raise ValueError("image must be contiguous")
    if not (points.is_cuda and image.is_cuda):
        raise ValueError("points and image must be device tensors; there is no CPU fallback")
    if points.device != image.device:
        raise ValueError(f"points and image live on different devices: {points.device}, {image.device}")


def seed_sweep(points: torch.Tensor, l2w, boxes, cam: SeedCamera, image: torch.Tensor, min_z: float = -2.0):
    """One LiDAR sweep against one camera and its boxes.

    ``points`` [N,3] float32 on the device, in the LiDAR frame (rows may hold NaN); ``l2w`` LiDAR -> world ([3,4] or
    [4,4], host); ``boxes`` the host table of ``make_boxes`` ([B,15], B <= 64; ``None`` or empty: no boxes); ``image``
    [H,W,3] uint8 on the device, contiguous.  A point is *live* with no NaN, ``z_lidar > min_z`` and not
    ``|x_world| > 1e5``; *visible* when it projects in front of the camera into the image.  Returns
    ``(ObjectSeeds, BackgroundSeeds)``: for every box, in box order, the live visible points inside it (closed test; a
    point inside two boxes is in both) in the box's frame, and the live visible points inside no box in the world
    frame, each with the pixel's 3 bytes and the index of its row in ``points``.  Empty tensors when nothing passes.
    """
    _validate(points, image, cam)
    table = _box_table(boxes)
    n, nb = points.shape[0], table.shape[0]
    L.require_device(points, image)
    dev = points.device
    pts = points.contiguous()
    l2w32 = _host_matrix("l2w", l2w)
    c = L.SeedCam()
    c.w2c[:] = _host_matrix("cam.w2c", cam.w2c).reshape(-1).tolist()
    c.fx, c.fy, c.cx, c.cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
    c.width, c.height = int(cam.width), int(cam.height)
    lib = L.load()
    ws = L.workspace(lib.sgn_seed_workspace_bytes(n, nb), dev)
    totals = torch.empty(nb + 2, dtype=torch.int32, device=dev)
    L.check(lib.sgn_seed_classify(n, L.ptr(pts), l2w32.ctypes.data, float(min_z), nb,
                                  table.ctypes.data if nb else None, L.C.addressof(c), L.ptr(ws), ws.numel(),
                                  L.ptr(totals), L.stream_ptr()), "sgn_seed_classify")
    counts = totals.tolist()                                    # the one host read
    offsets = [0]
    for b in range(nb):
        offsets.append(offsets[-1] + counts[b])
    m, k = offsets[-1], counts[nb]
    local = torch.empty(m, 3, dtype=torch.float32, device=dev)
    o_rgb = torch.empty(m, 3, dtype=torch.uint8, device=dev)
    o_src = torch.empty(m, dtype=torch.int32, device=dev)
    world = torch.empty(k, 3, dtype=torch.float32, device=dev)
    b_rgb = torch.empty(k, 3, dtype=torch.uint8, device=dev)
    b_src = torch.empty(k, dtype=torch.int32, device=dev)
    if m or k:
        p = lambda t, rows: L.ptr(t) if rows else None
        L.check(lib.sgn_seed_emit(n, L.ptr(pts), nb, L.ptr(image), c.width, c.height, L.ptr(ws), ws.numel(),
                                  p(local, m), p(o_rgb, m), p(o_src, m), m, p(world, k), p(b_rgb, k), p(b_src, k), k,
                                  L.stream_ptr()), "sgn_seed_emit")
    return (ObjectSeeds(local, o_rgb, o_src.to(torch.int64), offsets),
            BackgroundSeeds(world, b_rgb, b_src.to(torch.int64), counts[nb + 1]))


def sweep_to_world(l2w, t0) -> np.ndarray:
    """The LiDAR -> world matrix the scripts transform a sweep with, [4,4] float64 on the host.

    ``extract_object_pts.py:157-166`` negates columns 1-2 of the dataset's ``transform_matrix``, swaps rows 0 and 1,
    negates row 2, subtracts ``T0`` from the translation, and undoes the three shuffles in reverse order.  The net
    effect: the rotation part is unchanged and the translation is reduced by ``(t0[1], t0[0], -t0[2])``."""
    m = np.array(l2w, dtype=np.float64)
    t = np.asarray(t0, dtype=np.float64).reshape(3)
    if m.shape == (3, 4):
        m = np.concatenate([m, np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)
    if m.shape != (4, 4):
        raise ValueError(f"l2w must have shape (3, 4) or (4, 4), got {m.shape}")
    m[:3, 3] -= np.array([t[1], t[0], -t[2]])
    return m


def _rgb_as_loaded(rgb_u8: torch.Tensor) -> torch.Tensor:
    """uint8 colours as ``load_object_3D_points`` hands them on: stored as float32 ``byte / 255``
    (``extract_object_pts.py:254,272``), read back ``* 255`` in float32 (``dynamic_annotation.py:361``)."""
    table = ((torch.arange(256, dtype=torch.float64) / 255.0).to(torch.float32) * 255.0).to(rgb_u8.device)   # on the host
    return table[rgb_u8.to(torch.int64)]


class SeedAccumulator:
    """The seed clouds over many ``seed_sweep`` calls: one cloud per track id and the background.

    ``add`` keeps the device tensors of one (sweep, camera) call; ``finish`` concatenates them in the reference's order
    (per call, then per box, then per point) and applies ``load_object_3D_points``' rule
    (``dynamic_annotation.py:348-365``): a track with fewer than ``min_points`` points has no seed."""

    def __init__(self):
        self._tracks: dict = {}
        self._background: list = []

    def add(self, track_ids, objects: ObjectSeeds, background: BackgroundSeeds | None = None) -> None:
        track_ids = list(track_ids)
        if len(track_ids) + 1 != len(objects.offsets):
            raise ValueError(f"{len(track_ids)} track ids for {len(objects.offsets) - 1} boxes")
        for b, tid in enumerate(track_ids):
            lo, hi = objects.offsets[b], objects.offsets[b + 1]
            self._tracks.setdefault(tid, []).append((objects.local[lo:hi], objects.rgb[lo:hi]))
        if background is not None:
            self._background.append((background.world, background.rgb))

    @staticmethod
    def _cat(parts):
        return torch.cat([p[0] for p in parts]), _rgb_as_loaded(torch.cat([p[1] for p in parts]))

    def finish(self, scale_factor: float = 1.0, min_points: int = 10000):
        """``(objects, background)``: ``objects[track_id]`` is ``(xyz [n,3] float32 * scale_factor, rgb [n,3] float32
        in 0..255)`` or ``None`` below ``min_points``; ``background`` is ``(xyz, rgb)`` in the world frame, unscaled
        (the dataparser scales it with the scene), or ``None`` when no call brought any."""
        objects = {}
        for tid, parts in self._tracks.items():
            xyz, rgb = self._cat(parts)
            objects[tid] = None if xyz.shape[0] < int(min_points) else (xyz * float(scale_factor), rgb)
        return objects, (self._cat(self._background) if self._background else None)


def random_quats(n: int, generator: torch.Generator | None = None, device=None) -> torch.Tensor:
    """``random_quat_tensor`` (``sgn_splatfacto.py:39-54``): three uniform draws per row, from ``generator``."""
    draw_dev = generator.device if generator is not None else torch.device("cpu")
    u, v, w = (torch.rand(n, generator=generator, device=draw_dev) for _ in range(3))
    q = torch.stack([torch.sqrt(1 - u) * torch.sin(2 * math.pi * v), torch.sqrt(1 - u) * torch.cos(2 * math.pi * v),
                     torch.sqrt(u) * torch.sin(2 * math.pi * w), torch.sqrt(u) * torch.cos(2 * math.pi * w)], dim=-1)
    return q.to(device) if device is not None else q


def init_gaussians(xyz: torch.Tensor, rgb255: torch.Tensor, sh_degree: int = 3, fourier_features_dim: int = 1,
                   generator: torch.Generator | None = None) -> dict:
    """The tensors ``populate_modules`` wraps in its ``ParameterDict`` (``sgn_splatfacto.py:255-300``) from a seed cloud
    ``xyz`` [N,3] float32 on the device and its colours ``rgb255`` [N,3] in 0..255: ``means``; ``scales`` =
    ``knn.init_log_scales(means)``; ``quats`` by ``random_quat_tensor`` (drawn on ``generator``'s device, the CPU
    without one, as the reference does); ``opacities`` = logit(0.1) [N,1]; ``features_dc`` [N,F,3] with slot 0 =
    ``RGB2SH(rgb255 / 255)`` — ``logit(rgb255 / 255, eps=1e-10)`` with ``sh_degree == 0`` (``:280``) — and the other
    Fourier slots zero; ``features_rest`` [N,(sh_degree + 1)^2 - 1,3] zeros.  Both divisions are true divisions."""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32:
        raise ValueError("xyz must be a float32 tensor of shape (N, 3)")
    if not isinstance(rgb255, torch.Tensor) or tuple(rgb255.shape) != tuple(xyz.shape):
        raise ValueError(f"rgb255 must have xyz's shape {tuple(xyz.shape)}")
    if int(sh_degree) < 0 or int(fourier_features_dim) < 1:
        raise ValueError("sh_degree must be >= 0 and fourier_features_dim >= 1")
    dev, n = xyz.device, xyz.shape[0]
    means = xyz.detach().contiguous()
    # tensor divisors: a Python-scalar divisor becomes a multiplication by its reciprocal on the device
    rgb = rgb255.to(device=dev, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32, device=dev)
    if int(sh_degree) > 0:
        dc0 = (rgb - 0.5) / torch.tensor(SH_C0, dtype=torch.float32, device=dev)
    else:
        dc0 = torch.logit(rgb, eps=1e-10)
    features_dc = torch.zeros(n, int(fourier_features_dim), 3, dtype=torch.float32, device=dev)
    features_dc[:, 0, :] = dc0
    return {
        "means": means,
        "scales": knn.init_log_scales(means),
        "quats": random_quats(n, generator, dev),
        "features_dc": features_dc,
        "features_rest": torch.zeros(n, (int(sh_degree) + 1) ** 2 - 1, 3, dtype=torch.float32, device=dev),
        "opacities": torch.logit(0.1 * torch.ones(n, 1)).to(dev),                  # on the host, as the reference
    }

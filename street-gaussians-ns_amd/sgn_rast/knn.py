"""Exact k-nearest neighbours of the seed points, for the Gaussians' initial scales (``csrc/knn.hip``).

The reference sets every model's starting scales in ``SplatfactoModel.populate_modules``
(``street_gaussians_ns/sgn_splatfacto.py:260-264``) from ``k_nearest_sklearn(means.data, 3)`` (``:439-457``): sklearn's
``NearestNeighbors(n_neighbors=k + 1)`` on the CPU, first column dropped.  The scene graph does it once per sub-model
(``sgn_splatfacto_scene_graph.py:85``) before the first step.  Here the search runs on the device:

* ``k_nearest(x, k)``          device tensors in, ``(dist [N,k] f32, idx [N,k] int64)`` out, on the current stream;
* ``k_nearest_sklearn(x, k)``  the reference method's return contract (numpy float32 distances and indices), for
  ``SplatfactoModel.k_nearest_sklearn = staticmethod(sgn_rast.knn.k_nearest_sklearn)``;
* ``init_log_scales(means)``   the scales tensor ``populate_modules`` builds, computed on the device.

Distances are exactly the multiset sklearn returns in its columns 1..k (duplicate points included: a duplicate sits
at distance 0, whichever of the equal points sklearn lists first).  On equal distances the INDICES may differ from
sklearn's; they are always distinct, never the query itself, and at the distance reported.  Results are bit-identical
from run to run.  No autograd, no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

K_MAX = 16


def _validate(x, k):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"x must be a torch.Tensor, got {type(x).__name__}")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"x must have shape (N, 3), got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"x must be float32, got {x.dtype}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= K_MAX:
        raise ValueError(f"k must be an integer in [1, {K_MAX}], got {k!r}")
    n = x.shape[0]
    if n <= int(k):
        # sklearn: "Expected n_neighbors <= n_samples_fit" for NearestNeighbors(k + 1)
        raise ValueError(f"k + 1 = {int(k) + 1} neighbours requested from {n} points: need N > k")
    if n > (1 << 30):
        raise ValueError(f"at most 2**30 points, got {n}")


def k_nearest(x: torch.Tensor, k: int, visited: torch.Tensor | None = None):
    """For every row of ``x`` [N,3] (float32, finite, on the device): the ``k`` nearest OTHER rows.

    Returns ``(dist [N,k] float32 ascending, idx [N,k] int64)``.  ``visited`` (optional int64 device tensor of one
    element) is increased by the number of candidate distances evaluated.  One host read: the finiteness check.
    """
    _validate(x, k)
    k = int(k)
    L.require_device(x, visited)
    if visited is not None and (visited.dtype != torch.int64 or visited.numel() < 1):
        raise ValueError("visited must be an int64 device tensor")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("x holds non-finite coordinates")
    xc = x.contiguous()
    n = xc.shape[0]
    lib = L.load()
    dist = torch.empty(n, k, dtype=torch.float32, device=x.device)
    idx = torch.empty(n, k, dtype=torch.int32, device=x.device)
    ws = L.workspace(lib.sgn_knn_workspace_bytes(n, k), x.device)
    L.check(lib.sgn_knn(n, k, L.ptr(xc), L.ptr(dist), L.ptr(idx), L.ptr(visited), L.ptr(ws), ws.numel(),
                        L.stream_ptr()), "sgn_knn")
    return dist, idx.to(torch.int64)


def k_nearest_sklearn(x: torch.Tensor, k: int):
    """Drop-in for ``SplatfactoModel.k_nearest_sklearn`` (``sgn_splatfacto.py:439-457``) without ``self``:
    ``(distances float32 [N,k], indices float32 [N,k])`` as numpy arrays.  A CPU tensor (what the reference passes) is
    moved to the current device for the search; the search itself never runs on the CPU."""
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        if not torch.cuda.is_available():
            raise L.SgnRastError("k_nearest_sklearn runs on the GPU; there is no CPU fallback")
        x = x.to(torch.device("cuda", L.current_device()))
    if isinstance(x, torch.Tensor) and x.dtype != torch.float32 and x.is_floating_point():
        x = x.float()        # the reference hands sklearn whatever means.data is; sklearn computes in float64
    dist, idx = k_nearest(x.detach(), k)
    return dist.cpu().numpy(), idx.to(torch.float32).cpu().numpy()


def init_log_scales(means: torch.Tensor, k: int = 3) -> torch.Tensor:
    """``log(mean of the k nearest-neighbour distances)`` repeated over the three axes, [N,3] on the device: the
    tensor ``populate_modules`` wraps in ``torch.nn.Parameter`` (``sgn_splatfacto.py:260-264``), with its arithmetic
    (fp32 mean, then log, then repeat) — including ``-inf`` for a point with k exact duplicates."""
    dist, _ = k_nearest(means.detach(), k)
    return torch.log(dist.mean(dim=-1, keepdim=True)).repeat(1, 3)

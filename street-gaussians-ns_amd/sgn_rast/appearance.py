"""Per-image colour correction: bilateral grids sliced by one fused kernel pair (``csrc/bilagrid.hip``).

The cameras of a street rig meter on their own and change exposure from frame to frame; the Gaussians would otherwise
have to explain one wall at several brightnesses.  gsplat's trainer answers with a bilateral grid per image — a small
3-D table of 3x4 colour affines indexed by pixel position and luminance, held smooth by a total-variation prior — and the
original Street Gaussians code with one learnable 3x4 affine per image / sensor, which is the 1 x 1 x 1 grid.

* :class:`BilateralGrids` — the parameter ``grids [num, L, Hg, Wg, 12]`` (cell-major: a cell's 12 coefficients are
  contiguous, coefficient ``4 r + c`` is row ``r``, column ``c`` of the affine, ``c = 3`` the bias), identity at start;
* :func:`slice_image` — ``rgb [H,W,3] -> [H,W,3]`` through grid ``index``, an autograd ``Function`` over
  ``sgn_bilagrid_slice_fwd / _bwd`` (the definition is in include/sgn_rast.h "BILATERAL GRID" and DESIGN.md §4);
* :func:`total_variation` — the prior, plain torch on the small tensor.

An identity grid returns its input bit for bit, so switching the feature on with fresh grids moves nothing.  No CPU
fallback: a CPU tensor raises, as everywhere in the package.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib as L

_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def check_slice_args(grids: torch.Tensor, index: int, rgb: torch.Tensor) -> None:
    """The host-side ``ValueError``s of :func:`slice_image`, before anything is launched."""
    if not isinstance(grids, torch.Tensor) or grids.dim() != 5 or grids.shape[-1] != 12 or 0 in grids.shape:
        raise ValueError(f"grids must be [num, L, Hg, Wg, 12], got {tuple(getattr(grids, 'shape', ()))}")
    if grids.dtype != torch.float32:
        raise ValueError(f"grids must be float32, got {grids.dtype}")
    if isinstance(index, bool) or not isinstance(index, int):
        raise ValueError(f"index must be a Python int, got {type(index).__name__}")
    if not 0 <= index < grids.shape[0]:
        raise ValueError(f"index {index} is out of range for {grids.shape[0]} grids")
    if not isinstance(rgb, torch.Tensor) or rgb.dim() != 3 or rgb.shape[-1] != 3 or 0 in rgb.shape:
        raise ValueError(f"rgb must be [H, W, 3], got {tuple(getattr(rgb, 'shape', ()))}")
    if rgb.dtype != torch.float32:
        raise ValueError(f"rgb must be float32, got {rgb.dtype}")


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, index, rgb):
        check_slice_args(grids, index, rgb)
        L.require_device(grids, rgb)
        ctx.set_materialize_grads(False)
        grid = grids[index].contiguous()            # the one row that is read (a view when grids is contiguous)
        rgb_c = rgb.contiguous()
        H, W = rgb_c.shape[:2]
        out = torch.empty_like(rgb_c)
        L.check(L.load().sgn_bilagrid_slice_fwd(grid.shape[0], grid.shape[1], grid.shape[2], L.ptr(grid), H, W, H * W,
                                                L.ptr(rgb_c), L.ptr(out), L.stream_ptr()), "sgn_bilagrid_slice_fwd")
        ctx.save_for_backward(grids, rgb_c)
        ctx.index = index
        return out

    @staticmethod
    def backward(ctx, v_out):
        if v_out is None:
            return None, None, None
        grids, rgb_c = ctx.saved_tensors
        grid = grids[ctx.index].contiguous()
        H, W = rgb_c.shape[:2]
        v = v_out.contiguous().float()
        want_grid, _, want_rgb = ctx.needs_input_grad
        v_grids = torch.zeros(grids.shape, dtype=torch.float32, device=grids.device) if want_grid else None
        v_rgb = torch.empty_like(rgb_c) if want_rgb else None
        L.check(L.load().sgn_bilagrid_slice_bwd(grid.shape[0], grid.shape[1], grid.shape[2], L.ptr(grid), H, W, H * W,
                                                L.ptr(rgb_c), L.ptr(v), L.ptr(v_rgb),
                                                L.ptr(v_grids[ctx.index]) if want_grid else None, L.stream_ptr()),
                "sgn_bilagrid_slice_bwd")
        return v_grids, None, v_rgb


def slice_image(grids: torch.Tensor, index: int, rgb: torch.Tensor) -> torch.Tensor:
    """``rgb`` [H,W,3] float32 corrected by grid ``index`` of ``grids`` [num, L, Hg, Wg, 12] float32 (a
    :class:`BilateralGrids` module is taken as its parameter).  Differentiable in both; the gradient of ``grids`` has the
    full shape and is exactly zero outside row ``index``, and the other rows are never read.  Non-contiguous inputs are
    accepted.  Wrong shapes, dtypes or an ``index`` out of range raise ``ValueError`` before any launch; CPU tensors
    raise ``SgnRastError``."""
    if isinstance(grids, BilateralGrids):
        grids = grids.grids
    check_slice_args(grids, index, rgb)
    return _Slice.apply(grids, index, rgb)


def total_variation(grids: torch.Tensor) -> torch.Tensor:
    """The smoothness prior of ``grids`` [num, L, Hg, Wg, 12]: the sum, over the axes L, Hg, Wg of size greater than 1,
    of the mean squared forward difference along that axis, divided by ``num``.  Plain torch (the tensor is small)."""
    if isinstance(grids, BilateralGrids):
        grids = grids.grids
    if grids.dim() != 5 or grids.shape[-1] != 12:
        raise ValueError(f"grids must be [num, L, Hg, Wg, 12], got {tuple(grids.shape)}")
    tv = grids.new_zeros(())
    for axis in (1, 2, 3):
        n = grids.shape[axis]
        if n > 1:
            diff = grids.narrow(axis, 1, n - 1) - grids.narrow(axis, 0, n - 1)
            tv = tv + diff.pow(2).mean()
    return tv / grids.shape[0]


class BilateralGrids(torch.nn.Module):
    """``num`` bilateral grids of ``grid = (Wg, Hg, L)`` cells — gsplat's argument order: x, y, luminance — as one
    parameter ``grids [num, L, Hg, Wg, 12]``, every cell the identity affine.  ``grid=(1, 1, 1)`` is the per-image
    affine; "per sensor" means the caller passes the sensor's number as the index."""

    def __init__(self, num: int, grid: Tuple[int, int, int] = (16, 16, 8), device=None):
        super().__init__()
        Wg, Hg, Lz = (int(v) for v in grid)
        if num < 1 or min(Wg, Hg, Lz) < 1:
            raise ValueError(f"num and the grid's sizes must be >= 1, got num={num}, grid={tuple(grid)}")
        eye = torch.tensor(_IDENTITY, dtype=torch.float32, device=device)
        self.grids = torch.nn.Parameter(eye.repeat(num, Lz, Hg, Wg, 1))

    @classmethod
    def from_channel_major(cls, t: torch.Tensor) -> "BilateralGrids":
        """From gsplat's layout ``[num, 12, L, Hg, Wg]``."""
        if t.dim() != 5 or t.shape[1] != 12:
            raise ValueError(f"expected [num, 12, L, Hg, Wg], got {tuple(t.shape)}")
        num, _, Lz, Hg, Wg = t.shape
        m = cls(num, (Wg, Hg, Lz), device=t.device)
        with torch.no_grad():
            m.grids.copy_(t.detach().permute(0, 2, 3, 4, 1))
        return m

    def to_channel_major(self) -> torch.Tensor:
        """gsplat's layout ``[num, 12, L, Hg, Wg]`` (a copy, detached)."""
        return self.grids.detach().permute(0, 4, 1, 2, 3).contiguous()

    def forward(self, index: int, rgb: torch.Tensor) -> torch.Tensor:
        return slice_image(self.grids, index, rgb)

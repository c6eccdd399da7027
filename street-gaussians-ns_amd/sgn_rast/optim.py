"""Multi-tensor Adam for the per-Gaussian parameter groups.

The reference builds one ``torch.optim.Adam`` per parameter group through nerfstudio's ``AdamOptimizerConfig``
(``street_gaussians_ns/sgn_config.py:71-108``: xyz, features_dc, features_rest, opacity, scaling, rotation, sky_sphere;
eps 1e-15; the scene graph multiplies that by the number of sub-models) and steps them one after the other.
:class:`FusedAdam` is a ``torch.optim.Optimizer`` with Adam's constructor and **state layout** (``state[p]['step']``,
``['exp_avg']``, ``['exp_avg_sq']`` — the tensors the reference's densification rewrites in place,
``sgn_splatfacto.py:459-511``), whose ``step()`` updates every parameter of every group in ONE kernel launch
(``sgn_adam_step``, ``csrc/optim.hip``).  :func:`step_many` does the same across several optimizer objects (the
reference's one-optimizer-per-group layout).  No CPU fallback: parameters must live on the ROCm device.

``step(visible=...)`` / ``step_many(..., visible=...)`` step only the rows a view saw (``sgn_adam_step_visible``): gsplat's
``SelectiveAdam``, fed with the projection's ``radii`` as they are; :func:`visibility` builds the argument for a scene graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Union

import torch

from . import _lib as L


def _launch(rows: List[tuple]) -> None:
    """rows: (param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step)."""
    if not rows:
        return
    n = len(rows)
    ptrs = lambda k: (C.c_void_p * n)(*[r[k].data_ptr() for r in rows])
    f32 = lambda k: (C.c_double * n)(*[float(r[k]) for r in rows])   # doubles: torch's Python scalars
    numel = (C.c_int64 * n)(*[r[0].numel() for r in rows])
    steps = (C.c_int64 * n)(*[int(r[8]) for r in rows])
    L.check(L.load().sgn_adam_step(n, ptrs(0), ptrs(1), ptrs(2), ptrs(3), numel, f32(4), f32(5), f32(6), f32(7), steps,
                                   L.stream_ptr()), "sgn_adam_step")
    # the kernel wrote through raw pointers: tell autograd, as torch.optim.Adam's in-place ops do.  This package's own
    # caches (ops._bin_key, ops._window_info, step._world_scene_params) read "same data_ptr, same version" as "same bytes".
    torch.autograd.graph.increment_version([t for r in rows for t in (r[0], r[2], r[3])])


_VIS_KINDS = {torch.bool: 1, torch.uint8: 1, torch.int32: 2}       # SGN_ADAM_VIS_U8 / SGN_ADAM_VIS_I32 of include/sgn_rast.h
Visible = Union[None, torch.Tensor, Mapping[torch.Tensor, torch.Tensor]]


def _resolve_visible(optimizers: Sequence["FusedAdam"], visible: Visible) -> Dict[torch.Tensor, Optional[torch.Tensor]]:
    """parameter -> its visibility tensor (None: steps densely) for every parameter that has a gradient.  Raises on
    anything the kernel could not take, BEFORE a ``state['step']`` is incremented and before anything launches."""
    if not isinstance(visible, (torch.Tensor, Mapping)):
        raise TypeError(f"visible must be None, a tensor or a mapping parameter -> tensor, got {type(visible).__name__}")
    out = {}
    for opt in optimizers:
        for group in opt.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                vis = visible if isinstance(visible, torch.Tensor) else visible.get(p)
                if vis is not None:
                    if not isinstance(vis, torch.Tensor):
                        raise TypeError(f"a visibility must be a tensor, got {type(vis).__name__}")
                    if vis.dtype not in _VIS_KINDS:
                        raise TypeError(f"a visibility is torch.bool, torch.uint8 or torch.int32 (radii), got {vis.dtype}")
                    if p.dim() == 0 or vis.dim() != 1 or vis.shape[0] != p.shape[0]:
                        raise ValueError(f"a visibility has one entry per row: parameter {tuple(p.shape)}, "
                                         f"visibility {tuple(vis.shape)}")
                    if not vis.is_contiguous():
                        raise ValueError("a visibility must be contiguous")
                    if vis.device != p.device:
                        raise ValueError(f"a visibility lives on its parameter's device: {vis.device} against {p.device}")
                out[p] = vis
    return out


def _launch_visible(rows: List[tuple], vis_of: Dict[torch.Tensor, Optional[torch.Tensor]]) -> None:
    """:func:`_launch` through ``sgn_adam_step_visible``; ``vis_of`` from :func:`_resolve_visible`."""
    if not rows:
        return
    n = len(rows)
    ptrs = lambda k: (C.c_void_p * n)(*[r[k].data_ptr() for r in rows])
    f32 = lambda k: (C.c_double * n)(*[float(r[k]) for r in rows])
    numel = (C.c_int64 * n)(*[r[0].numel() for r in rows])
    steps = (C.c_int64 * n)(*[int(r[8]) for r in rows])
    vis = [vis_of[r[0]] for r in rows]
    n_rows = (C.c_int64 * n)(*[r[0].shape[0] if r[0].dim() else 1 for r in rows])
    vis_ptr = (C.c_void_p * n)(*[None if v is None else v.data_ptr() for v in vis])     # the caller's tensors: no copy
    kinds = (C.c_int32 * n)(*[0 if v is None else _VIS_KINDS[v.dtype] for v in vis])
    L.check(L.load().sgn_adam_step_visible(n, ptrs(0), ptrs(1), ptrs(2), ptrs(3), numel, f32(4), f32(5), f32(6), f32(7),
                                           steps, n_rows, vis_ptr, kinds, L.stream_ptr()), "sgn_adam_step_visible")
    torch.autograd.graph.increment_version([t for r in rows for t in (r[0], r[2], r[3])])    # as _launch does


def visibility(models: Sequence[Mapping[str, torch.Tensor]], radii_parts: Sequence[torch.Tensor]) -> Dict[torch.Tensor, torch.Tensor]:
    """The ``visible`` mapping of a scene graph: every parameter of sub-model ``i`` (a dict name -> parameter, all with
    one row per Gaussian) -> ``radii_parts[i]``, the sub-model's slice of the projection's ``radii`` (``out.radii_parts``
    of :func:`sgn_rast.step.render`).  The parts are handed over as they are, views of one tensor: no copy."""
    if len(models) != len(radii_parts):
        raise ValueError(f"{len(models)} sub-models against {len(radii_parts)} radii parts")
    out = {}
    for i, (model, part) in enumerate(zip(models, radii_parts)):
        for name, p in model.items():
            if p.dim() == 0 or part.dim() != 1 or p.shape[0] != part.shape[0]:
                raise ValueError(f"sub-model {i}: {name} {tuple(p.shape)} against radii {tuple(part.shape)}")
            out[p] = part
    return out


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps)`` (no weight decay / amsgrad / maximize — the reference uses none)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, maximize: bool = False):
        if weight_decay != 0.0 or amsgrad or maximize:
            raise NotImplementedError("FusedAdam implements the configuration the reference uses: plain Adam")
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))

    def _rows(self) -> List[tuple]:
        rows = []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                L.require_device(p, p.grad)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedAdam needs contiguous fp32 parameters")
                st = self.state[p]
                if len(st) == 0:                      # same lazy initialisation as torch.optim.Adam
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                rows.append((p, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], group["lr"], b1, b2,
                             group["eps"], int(st["step"].item())))
        return rows

    @torch.no_grad()
    def step(self, closure=None, *, visible: Visible = None):
        """``visible``: step only the rows a view saw (gsplat's ``SelectiveAdam``).  One tensor ``[R]`` for every
        parameter with a gradient (each must have ``shape[0] == R``), or a mapping parameter -> tensor (a parameter absent
        from it steps densely); ``torch.bool`` / ``torch.uint8`` (visible if nonzero) or ``torch.int32`` (visible if
        ``> 0``: the projection's ``radii``), contiguous, on the parameter's device.  A visible row gets the dense step's
        result bit for bit.  An invisible row keeps ``param``, ``exp_avg`` and ``exp_avg_sq`` bit for bit and its gradient
        is never read.  ``state['step']`` advances for every parameter that has a gradient, whether or not a row of it is
        visible, and the bias corrections use that global count.  This is NOT ``torch.optim.Adam`` on a zero gradient:
        the moments of an invisible row do not decay and its parameter does not coast on them."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if visible is None:
            _launch(self._rows())
        else:
            vis_of = _resolve_visible([self], visible)
            _launch_visible(self._rows(), vis_of)
        return loss


@torch.no_grad()
def step_many(optimizers: Iterable[FusedAdam], visible: Visible = None) -> None:
    """One launch for several :class:`FusedAdam` objects (nerfstudio keeps one optimizer per parameter group).
    ``visible``: as in :meth:`FusedAdam.step`, e.g. ``step_many(adam, visible=out.radii)``."""
    if visible is not None:
        optimizers = list(optimizers)
        vis_of = _resolve_visible(optimizers, visible)      # raises before _rows() counts a step
    rows: List[tuple] = []
    for opt in optimizers:
        rows.extend(opt._rows())
    if visible is None:
        _launch(rows)
    else:
        _launch_visible(rows, vis_of)

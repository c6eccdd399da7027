"""Host side of the layered evaluation forward (``csrc/raster_layers.hip``): one walk of the depth list composites the
whole scene, the ids below ``split`` (the scene graph's background sub-model) and the ids from ``split`` (the objects), and
one elementwise launch finishes all three the way the reference's eval mode does (``sgn_splatfacto.py:968-996`` with
``self.training == False``).  Forward only: nothing here builds an autograd graph."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L
from . import ops as _ops

# the objects layer finishes on its own compacted list (sgn_list_window) when it is a small part of the scene: carried on
# the shared list it never finishes where no object is and drags every tile's walk to the end of its list
# (DESIGN.md "Layered evaluation forward"; False: A/B runs and the tests of the shared-list form)
tail_own_list = True
stats = {"calls": 0, "own_lists": 0}


def rasterize_layers(xys, depths, radii, conics, num_tiles_hit, colors, opacity_logits, img_height: int,
                     img_width: int, block_width: int, background: torch.Tensor, split: int,
                     own_list: Optional[bool] = None, opacity_is_logit: bool = True):
    """-> ``(img [3,H,W,3], final_T [3,H,W], depth [H,W])`` for the layers all / ids < split / ids >= split; each layer's
    image (``C + T * background``) and transmittance are bit-equal to ``rasterize_gaussians_fused`` with that
    ``id_range`` (``tests/test_gpu_layers.py``).  The binning is the whole scene's, shared with the binning cache.
    ``opacity_is_logit=False``: ``opacity_logits`` holds probabilities (the antialiased mode's
    ``fused.antialiased_opacities``), as the same argument of ``rasterize_gaussians_fused``."""
    if block_width != 16:
        raise L.SgnRastError("the layered forward exists for 16x16 tiles only (block_width=16)")
    with torch.no_grad():
        dev = L.require_device(xys, depths, radii, conics, num_tiles_hit, colors, opacity_logits, background)
        n = xys.shape[0]
        split = min(max(int(split), 0), n)
        H, W = int(img_height), int(img_width)
        f32 = dict(dtype=torch.float32, device=dev)
        c = _ops._contig
        xys, depths, radii, conics, num_tiles_hit = c(xys), c(depths), c(radii), c(conics), c(num_tiles_hit)
        opacity_logits = c(opacity_logits)
        xys_c, conics_c, colors_c, depths_c = (_ops._f32c(t.detach()) for t in (xys, conics, colors, depths))
        opac_c, bg_c = _ops._f32c(opacity_logits.detach()).reshape(-1), _ops._f32c(background.detach())
        img = torch.empty(3, H, W, 3, **f32)
        Ts = torch.empty(3, H, W, **f32)
        D = torch.empty(H, W, **f32)
        tile_bounds = ((W + 15) // 16, (H + 15) // 16, 1)
        n_isect, ids, bins = (0, None, None) if n == 0 else _ops._bin_gaussians_cached(
            n, xys, depths, radii, num_tiles_hit, tile_bounds, 16, conics, opacity_logits, bool(opacity_is_logit))
        if n_isect < 1:                       # nothing on screen: every layer is empty (T = 1, image = background)
            img[:] = bg_c
            Ts.fill_(1.0)
            D.zero_()
            return img, Ts, D
        lib = L.load()
        ro = L.opts().copy()
        ro.ids_qmask = int(bool(getattr(ids, "_sgn_qmask", False)))
        order = _ops._tile_order(bins, None, _ops._fwd_long_thresh(ro, 16))
        want_own = tail_own_list if own_list is None else bool(own_list)
        own_ids = own_bins = None
        if want_own and 0 < n - split < _ops.list_window_max_frac * n:
            own_ids, own_bins = _ops._list_window(ids, bins, split, n, ro.ids_qmask)
            stats["own_lists"] += 1
        recs = L.workspace(lib.sgn_raster_workspace_bytes(n, n_isect, L.C.byref(ro)), dev)
        L.check(lib.sgn_raster_layers_fwd(
            H, W, 16, n, n_isect, L.ptr(ids), L.ptr(bins), L.ptr(xys_c), L.ptr(conics_c), L.ptr(colors_c), L.ptr(opac_c),
            int(bool(opacity_is_logit)),
            L.ptr(bg_c), L.ptr(depths_c), split, L.ptr(own_ids), L.ptr(own_bins), L.ptr(img), L.ptr(Ts), L.ptr(D),
            L.ptr(recs), recs.numel(), 0, L.ptr(order), L.C.byref(ro), L.stream_ptr()), "sgn_raster_layers_fwd")
        stats["calls"] += 1
        return img, Ts, D


def finish(img: torch.Tensor, Ts: torch.Tensor, D: torch.Tensor, sky: Optional[torch.Tensor] = None):
    """The reference's per-pixel eval finish of the three layers in one launch (``sgn_layers_finish``) ->
    ``(rgb [3,H,W,3], acc [3,H,W], depth [H,W])``: ``rgb = clamp(clamp(img, max=1) * acc + sky * (1 - acc), 0, 1)`` for
    the scene and the head layer, no sky on the tail layer (``sgn_splatfacto_scene_graph.py:371``), ``depth =
    where(acc > 1e-3, D / acc, 10)``; without ``sky`` no layer is blended."""
    with torch.no_grad():
        dev = L.require_device(img, Ts, D, sky)
        H, W = int(D.shape[0]), int(D.shape[1])
        assert img.shape == (3, H, W, 3) and Ts.shape == (3, H, W), (img.shape, Ts.shape)
        assert sky is None or sky.shape == (H, W, 3), sky.shape
        img_c, Ts_c, D_c = _ops._f32c(img), _ops._f32c(Ts), _ops._f32c(D)
        sky_c = None if sky is None else _ops._f32c(sky.detach())
        rgb, acc = torch.empty_like(img_c), torch.empty_like(Ts_c)
        depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        L.check(L.load().sgn_layers_finish(H, W, L.ptr(img_c), L.ptr(Ts_c), L.ptr(D_c), L.ptr(sky_c), L.ptr(rgb),
                                           L.ptr(acc), L.ptr(depth), L.stream_ptr()), "sgn_layers_finish")
        return rgb, acc, depth

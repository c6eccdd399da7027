"""Call-site replay of the reference's per-step use of the hot path.

``render`` reproduces, line for line, the argument construction of
``SplatfactoModel.get_outputs`` / ``render_gaussian_attrs``
(``street_gaussians_ns/sgn_splatfacto.py:857-873, 889-890, 933-996``) with
``self.training=True``; ``train_step`` adds the synthetic loss of SURVEY.md §8d
(fixed random weights on rgb and alpha) and the backward.  ``ops`` is the operator
namespace: the product passes :mod:`sgn_rast.ops`; the parity tests run the very same
function a second time with the CPU oracle's namespace to get the expected tensors.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import ops as _hip_ops
from . import shutter as _shutter
from .quat import quaternion_multiply   # what `from pytorch3d.transforms import quaternion_multiply` resolves to
from .scenes import Camera


_CONST: Dict[tuple, torch.Tensor] = {}


def _zeros3(dev, dtype=torch.float32) -> torch.Tensor:
    """The reference keeps its background colour as a module attribute made once (sgn_splatfacto.py:311); the replay
    does the same instead of launching a fill kernel per step."""
    key = (str(dev), dtype)
    if key not in _CONST:
        _CONST[key] = torch.zeros(3, device=dev, dtype=dtype)
    return _CONST[key]


def _zero_colors(n: int, dev) -> torch.Tensor:
    """[n,3] zeros for an accumulation-only pass, made once per size (a 12 MB fill per sub-model pass otherwise)."""
    key = ("zero_colors", str(dev), int(n))
    if key not in _CONST:
        if len(_CONST) > 64:
            _CONST.clear()
        _CONST[key] = torch.zeros(n, 3, device=dev)
    return _CONST[key]


def leaf_params(raw: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Raw scene tensors -> autograd leaves (what nn.Parameter would be in SplatfactoModel)."""
    return {k: v.detach().clone().requires_grad_(True) for k, v in raw.items()}


def antialiased_mode(rasterize_mode: str) -> bool:
    """``rasterize_mode`` ("classic" | "antialiased", the reference's config field, sgn_splatfacto.py:214-222) -> is it
    the antialiased one; anything else raises ``ValueError`` as the reference does (:951), before anything is launched."""
    if rasterize_mode == "classic":
        return False
    if rasterize_mode == "antialiased":
        return True
    raise ValueError(f"Unknown rasterize_mode: {rasterize_mode!r} (\"classic\" or \"antialiased\")")


def _split_recat(t: torch.Tensor, counts, retain_grad: bool = False):
    """The scene graph's property setters (sgn_splatfacto_scene_graph.py:153-215): every projection output is split
    per sub-model (views; `retain_grad` on the xys views, which is what each sub-model's `after_train` reads) and
    concatenated again — so the tensor the rasterizer receives is a COPY of the projection's output."""
    parts = torch.split(t, counts)                                               # set_split_tensor_variable :153-167
    if retain_grad:
        for part in parts:
            if part.requires_grad:
                part.retain_grad()
    return torch.concat(parts, dim=0), parts                                     # get_aggreated_variable :138-146


def render(P: Dict[str, torch.Tensor], cam: Camera, sh_degree_to_use: int = 3, block_width: int = 16,
           background: Optional[torch.Tensor] = None, with_depth: bool = False, ops=_hip_ops,
           retain_xys_grad: bool = True, split_counts=None, caller_syncs: bool = True,
           rasterize_mode: str = "classic", rolling_shutter=None, object_velocities=None) -> SimpleNamespace:
    """``split_counts``: per-sub-model Gaussian counts when the caller is the scene graph (its property setters split
    and re-concatenate every projection output).  ``caller_syncs``: also replay the two host syncs the reference's
    own code performs per pass (`radii.sum() == 0` at :878, `assert (num_tiles_hit > 0).any()` at :944).
    ``rasterize_mode="antialiased"``: the opacities are the reference's own commented-out expression (:947),
    ``torch.sigmoid(opacities) * comp[:, None]``, with autograd through the projection's compensation output.
    ``rolling_shutter`` (a :class:`sgn_rast.shutter.RollingShutter`; None: global shutter, today's path untouched): the
    projection's outputs pass through :func:`sgn_rast.shutter.apply` directly behind the projection call, so ``out.xys``
    and the other projection outputs — what the rasterizer, the depth pass, ``xys.grad`` and the scene graph's splits
    see — are the sheared ones.  ``object_velocities`` [M,3] (with ``split_counts``: one row per sub-model, world
    axes, zero for the background): each sub-model's Gaussians move with their own linear velocity.  Out of scope: the
    per-line rotation of the SH view directions, object angular velocity, learnable velocities."""
    antialiased = antialiased_mode(rasterize_mode)
    rs = _shutter.check(rolling_shutter)
    if object_velocities is not None and (rs is None or split_counts is None):
        raise ValueError("object_velocities needs rolling_shutter and the scene graph's split_counts")
    dev = P["means"].device
    H, W = cam.height, cam.width
    if background is None:
        background = _zeros3(dev, P["means"].dtype)                              # :311,931
    scales = torch.exp(P["log_scales"])                                          # :857
    colors = torch.cat((P["features_dc"], P["features_rest"]), dim=1)            # :858
    quats = P["quats"] / P["quats"].norm(dim=-1, keepdim=True)                   # :864
    xys, depths, radii, conics, comp, num_tiles_hit, _cov3d = ops.project_gaussians(   # :860-873
        P["means"], scales, 1, quats, cam.viewmat[:3, :], cam.fx, cam.fy, *_shutter.projection_frame(cam, rs),
        block_width)
    if rs is not None:
        ids = None
        if object_velocities is not None:
            from .fused import object_ids_for
            ids = object_ids_for(split_counts, dev)
        xys, depths, radii, conics, num_tiles_hit = _shutter.apply(
            xys, depths, radii, conics, num_tiles_hit, cam, rs, block_width, object_ids=ids,
            object_velocities=object_velocities)
    out = SimpleNamespace()
    if split_counts is not None:                       # tuple-assign through the scene graph's setters, in order
        xys, out.xys_parts = _split_recat(xys, split_counts, retain_grad=retain_xys_grad)
        depths, out.depths_parts = _split_recat(depths, split_counts)
        radii, out.radii_parts = _split_recat(radii, split_counts)
        conics, out.conics_parts = _split_recat(conics, split_counts)
        num_tiles_hit, out.num_tiles_hit_parts = _split_recat(num_tiles_hit, split_counts)
        if antialiased:
            comp, out.comp_parts = _split_recat(comp, split_counts)
    out.xys, out.depths, out.radii, out.conics, out.num_tiles_hit = xys, depths, radii, conics, num_tiles_hit
    if caller_syncs and bool(radii.sum() == 0):                                  # :878 (host sync)
        # the reference's empty outputs (:879-886): background colour, zero accumulation / depth, no autograd graph
        # — a data-parallel rank whose view sees nothing must fall through to the collectives, not abort
        out.rgb = background.repeat(H, W, 1)
        out.alpha = torch.zeros(H, W, device=dev)
        out.depth = torch.zeros(H, W, 1, device=dev)
        out.empty = True
        return out
    if retain_xys_grad and xys.requires_grad:
        xys.retain_grad()                                                        # :889-890
    viewdirs = P["means"].detach() - cam.cam_pos.to(P["means"].dtype)            # :934
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)                    # :935
    rgbs = ops.spherical_harmonics(sh_degree_to_use, viewdirs, colors)           # :939
    rgbs = torch.clamp(rgbs + 0.5, min=0.0)                                      # :940
    if caller_syncs:
        assert (num_tiles_hit > 0).any()                                         # :944 (host sync)
    if antialiased:
        opacities = torch.sigmoid(P["opacity_logits"]) * comp.reshape(-1, *P["opacity_logits"].shape[1:])   # :947
    else:
        opacities = torch.sigmoid(P["opacity_logits"])                           # :949
    rgb, alpha = ops.rasterize_gaussians(                                        # :954-967
        xys, depths, radii, conics, num_tiles_hit, rgbs, opacities, H, W, block_width,
        background=background, return_alpha=True)
    out.rgb, out.alpha, out.rgbs, out.opacities = rgb, alpha, rgbs, opacities
    if with_depth:                                                               # :982-996
        depth_im = ops.rasterize_gaussians(
            xys, depths, radii, conics, num_tiles_hit, depths[:, None].repeat(1, 3), opacities, H, W,
            block_width, torch.zeros(3, device=dev, dtype=P["means"].dtype))[..., 0:1]     # :993 (a new tensor)
        out.depth = torch.where(alpha[..., None] > 1e-3, depth_im / alpha[..., None], 10)
    return out


def render_fused(P: Dict[str, torch.Tensor], cam: Camera, sh_degree_to_use: int = 3, block_width: int = 16,
                 background: Optional[torch.Tensor] = None, with_depth: bool = False,
                 object_ids: Optional[torch.Tensor] = None, poses: Optional[torch.Tensor] = None,
                 idft: Optional[torch.Tensor] = None, depth_channel: bool = True,
                 group_split: Optional[int] = None, rasterize_mode: str = "classic",
                 absgrad: bool = False, rolling_shutter=None, object_velocities=None) -> SimpleNamespace:
    """Same result as :func:`render` on the scene-graph-aggregated parameters, through the fused front
    ends (:mod:`sgn_rast.fused`): raw parameters in, no activation / concat / transform kernels.
    ``P["means"]`` / ``P["quats"]`` are in each object's LOCAL frame when ``object_ids``/``poses`` are given;
    ``P["features_dc"]`` is [N,F,3] with F Fourier coefficients weighted by ``idft[object]``.
    ``rasterize_mode="antialiased"``: ``fused.antialiased_opacities(logits, compensation)`` is formed once and every
    pass takes that one tensor as probabilities; ``out.opacities`` holds it (what a caller's further passes over the
    same render — ``features.rasterize_features``, ``expected_depth`` — take with ``opacity_is_logit=False``).
    ``absgrad=True``: the COLOUR pass also sums the absolute screen-space gradients — ``out.xys.absgrad`` [N,2] after
    ``backward()`` (:func:`sgn_rast.fused.rasterize_gaussians_fused`); the separate depth pass of
    ``depth_channel=False`` does not take part.
    ``rolling_shutter`` (a :class:`sgn_rast.shutter.RollingShutter`; None: global shutter, today's path untouched): the
    projection's outputs pass through :func:`sgn_rast.shutter.apply` directly behind the projection call; ``out.xys``
    and the other projection outputs are its results, so the binning prefetch, every raster pass, ``xys.grad`` /
    ``xys.absgrad`` and the antialiased opacities (the compensation factor passes through) work on the sheared
    Gaussians.  ``object_velocities`` [M,3] (with ``object_ids`` / ``poses``; world axes, one row per pose-table entry,
    zero for the background): each object's Gaussians move with their own linear velocity.  Out of scope: the per-line
    rotation of the SH view directions, object angular velocity, learnable velocities."""
    from . import fused
    antialiased = antialiased_mode(rasterize_mode)
    rs = _shutter.check(rolling_shutter)
    if object_velocities is not None and (rs is None or object_ids is None):
        raise ValueError("object_velocities needs rolling_shutter and object_ids / poses")
    dev = P["means"].device
    H, W = cam.height, cam.width
    if background is None:
        background = _zeros3(dev)
    xys, depths, radii, conics, comp, num_tiles_hit, _cov3d = fused.project_gaussians_fused(
        P["means"], P["log_scales"], P["quats"], cam.viewmat[:3, :], cam.fx, cam.fy,
        *_shutter.projection_frame(cam, rs), block_width, object_ids=object_ids, poses=poses)
    if rs is not None:
        xys, depths, radii, conics, num_tiles_hit = _shutter.apply(
            xys, depths, radii, conics, num_tiles_hit, cam, rs, block_width,
            object_ids=object_ids if object_velocities is not None else None, object_velocities=object_velocities)
    out = SimpleNamespace(xys=xys, depths=depths, radii=radii, conics=conics, num_tiles_hit=num_tiles_hit)
    if xys.requires_grad:
        xys.retain_grad()
    # the opacity argument of every pass below: the logits (sigmoid inside the row build), or the antialiased mode's
    # effective opacities — ONE tensor, so the binning cache keeps hitting and autograd sums the passes' gradients
    opac, logit = P["opacity_logits"], True
    if antialiased:
        opac = out.opacities = fused.antialiased_opacities(P["opacity_logits"], comp)
        logit = False
    # start the binning now: its host read-back then overlaps the SH evaluation queued below
    _hip_ops.prefetch_binning(xys, depths, radii, conics, num_tiles_hit, opac, H, W, block_width,
                              opacity_is_logit=logit)
    # SH view directions use WORLD means (scene_graph.py:355): the kernel applies the pose itself
    rgbs = fused.spherical_harmonics_fused(sh_degree_to_use, P["means"], cam.cam_pos, P["features_dc"],
                                           P["features_rest"], object_ids=object_ids, idft=idft, poses=poses)
    if with_depth and depth_channel:
        # the depth image rides in the colour pass as a fourth channel (no second rasterization) — and, with
        # `group_split`, so do the accumulations of the ids below / from the split (the scene graph's two sub-model passes)
        if group_split is not None:
            rgb, alpha, depth_im, out.acc_head, out.acc_tail = fused.rasterize_gaussians_fused(
                xys, depths, radii, conics, num_tiles_hit, rgbs, opac, H, W, block_width,
                background=background, return_alpha=True, depth_channel=True, group_split=group_split,
                opacity_is_logit=logit, absgrad=absgrad)
        else:
            rgb, alpha, depth_im = fused.rasterize_gaussians_fused(
                xys, depths, radii, conics, num_tiles_hit, rgbs, opac, H, W, block_width,
                background=background, return_alpha=True, depth_channel=True, opacity_is_logit=logit,
                absgrad=absgrad)
        out.rgb, out.alpha, out.rgbs = rgb, alpha, rgbs
        out.depth = torch.where(alpha[..., None] > 1e-3, depth_im[..., None] / alpha[..., None], 10)   # :995
        return out
    rgb, alpha = fused.rasterize_gaussians_fused(xys, depths, radii, conics, num_tiles_hit, rgbs, opac, H, W,
                                                 block_width, background=background, return_alpha=True,
                                                 opacity_is_logit=logit, absgrad=absgrad)
    out.rgb, out.alpha, out.rgbs = rgb, alpha, rgbs
    if with_depth:
        depth_im = fused.rasterize_gaussians_fused(
            xys, depths, radii, conics, num_tiles_hit, depths[:, None].repeat(1, 3), opac, H, W,
            block_width, _zeros3(dev), opacity_is_logit=logit)[..., 0:1]
        out.depth = torch.where(alpha[..., None] > 1e-3, depth_im / alpha[..., None], 10)
    return out


def _fused_scene_params(models, idft: torch.Tensor, sh_parts: bool = True):
    """What the fused front ends take for a scene graph: the raw per-model parameters concatenated, the object id of
    every row and the Fourier weights padded to the widest model -> (P, object_ids, idft_p)."""
    from . import fused as F_
    dev = models[0]["means"].device
    counts = [m["means"].shape[0] for m in models]
    cat = lambda key: torch.cat([m[key] for m in models], dim=0)                        # :355-360
    # the SH coefficients stay UN-concatenated (one pair per sub-model: sgn_sh_fwd_parts); `sh_parts=False` keeps the
    # round-3 form (torch.cat of features_rest, zero-padded cat of features_dc) for A/B and for the tests
    if sh_parts and len(models) <= F_.SH_MAX_PARTS:
        sh_dc, sh_rest = [m["features_dc"] for m in models], [m["features_rest"] for m in models]
    else:
        sh_dc, sh_rest = F_.cat_features_dc([m["features_dc"] for m in models]), cat("features_rest")
    P = dict(means=cat("means"), log_scales=cat("log_scales"), quats=cat("quats"),
             opacity_logits=cat("opacity_logits"), features_rest=sh_rest, features_dc=sh_dc)
    object_ids = F_.object_ids_for(counts, dev)       # per layout, built once (no per-step device work)
    # Fourier weights padded to the widest model: rows beyond a model's own dimension stay zero
    Fs = [m["features_dc"].shape[1] for m in models]
    Fmax = max(Fs)
    mask_key = ("fmask", str(dev), tuple(Fs), Fmax)
    if mask_key not in _CONST:
        if len(_CONST) > 64:
            _CONST.clear()
        _CONST[mask_key] = (torch.arange(Fmax)[None, :] < torch.tensor(Fs)[:, None]).to(dev, torch.float32)
    idft_p = torch.zeros(len(models), Fmax, device=dev)
    fw = min(Fmax, idft.shape[1])
    idft_p[:, :fw] = idft[:, :fw]
    idft_p = idft_p * _CONST[mask_key]
    return P, object_ids, idft_p


def _world_scene_params(models, poses: torch.Tensor, idft: torch.Tensor):
    """The aggregation at the head of ``SplatfactoSceneGraphModel.get_outputs`` (:320-360): object Gaussians moved to
    the world frame, Fourier features collapsed for the frame, everything concatenated -> (P, world_means, dcs)."""
    dev = models[0]["means"].device
    cat = lambda key: torch.cat([m[key] for m in models], dim=0)                        # :355-360
    world_means, world_quats, dcs = [], [], []
    # the reference's quat_o2w is a CPU float64 4-vector per object (`torch.from_numpy(quaternion_from_matrix(rot))`,
    # :412): one small read-back per step here, where the reference runs numpy on the host
    # (the cache entry HOLDS the pose tensor: while it lives no other tensor can take its address, so "same
    # data_ptr, same version" really means "same bytes" — keyed on the address alone a freed table's successor at
    # the same address was served the old quaternions: found in round 4 as a test that failed only in the full suite)
    pk = ("q_o2w", poses.data_ptr(), poses._version, str(dev))
    hit = _CONST.get(pk)
    if hit is None or hit[0] is not poses:
        if len(_CONST) > 64:
            _CONST.clear()
        hit = _CONST[pk] = (poses, poses[:, 12:16].detach().to("cpu", torch.float64))
    q_o2w = hit[1]
    for i, m in enumerate(models):
        Fi = m["features_dc"].shape[1]
        dcs.append((m["features_dc"] * idft[i][:Fi, None]).sum(dim=1, keepdim=True) if Fi > 1
                   else m["features_dc"])                                          # :239-247
        if i == 0:
            world_means.append(m["means"]); world_quats.append(m["quats"])
        else:
            R, t, q = poses[i, :9].reshape(3, 3), poses[i, 9:12], poses[i, 12:16]
            world_means.append(m["means"] @ R.T + t[None, :])                      # :415
            world_quats.append(quaternion_multiply(q_o2w[i], m["quats"]))           # :416
    P = dict(means=torch.cat(world_means), quats=torch.cat(world_quats), features_dc=torch.cat(dcs),
             opacity_logits=cat("opacity_logits"), features_rest=cat("features_rest"),
             log_scales=cat("log_scales"))
    return P, world_means, dcs


def _submodel_raster(models, world_means, dcs, out, sub, cam: Camera, sh_degree_to_use: int, block_width: int,
                     background: torch.Tensor, ops, caller_syncs: bool, antialiased: bool = False):
    """``get_submodel_output`` (:255-303) for the sub-models ``sub`` up to its rasterization -> (rgb, alpha) of the
    drop-in operator; ``out`` holds the per-model splits of the main projection (``antialiased``: the compensation's
    among them, aggregated like the others)."""
    # get_submodel_output (:255-303): per-model tensors are aggregated with torch.cat — the geometry from the
    # per-model SPLITS of the main projection (copies again), the parameters from the sub-models themselves
    agg = lambda parts: torch.cat([parts[i] for i in sub], dim=0)               # aggregate_submodel_var :249-253
    means_s = torch.cat([world_means[i] for i in sub], dim=0)
    dc_s = torch.cat([dcs[i] for i in sub], dim=0)
    opac_s = torch.cat([models[i]["opacity_logits"] for i in sub], dim=0)
    rest_s = torch.cat([models[i]["features_rest"] for i in sub], dim=0)
    xys_s, depths_s, radii_s = agg(out.xys_parts), agg(out.depths_parts), agg(out.radii_parts)
    conics_s, nth_s = agg(out.conics_parts), agg(out.num_tiles_hit_parts)
    colors = torch.cat((dc_s, rest_s), dim=1)                                       # :280
    viewdirs = means_s.detach() - cam.cam_pos
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    rgbs = torch.clamp(ops.spherical_harmonics(sh_degree_to_use, viewdirs, colors) + 0.5, min=0.0)  # :285 (unused)
    # render_gaussian_attrs (:916-967) evaluates the SH again from the colours it is handed
    viewdirs = means_s.detach() - cam.cam_pos
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    rgbs = torch.clamp(ops.spherical_harmonics(sh_degree_to_use, viewdirs, colors) + 0.5, min=0.0)  # :939
    if caller_syncs:
        assert (out.num_tiles_hit > 0).any()                                         # :944 (self.num_tiles_hit)
    opacities = torch.sigmoid(opac_s)                                                # :949
    if antialiased:
        opacities = opacities * agg(out.comp_parts).reshape(-1, *opac_s.shape[1:])   # :947
    return ops.rasterize_gaussians(xys_s, depths_s, radii_s, conics_s, nth_s, rgbs, opacities, cam.height,
                                   cam.width, block_width, background=background, return_alpha=True)   # :954-967


def render_scene_graph(models, poses: torch.Tensor, idft: torch.Tensor, cam: Camera, sh_degree_to_use: int = 3,
                       block_width: int = 16, ops=_hip_ops, fused: bool = False,
                       caller_syncs: bool = True, sh_parts: bool = True, groups: bool = True,
                       rasterize_mode: str = "classic", absgrad: bool = False, rolling_shutter=None,
                       object_velocities=None) -> SimpleNamespace:
    """Replay of ``SplatfactoSceneGraphModel.get_outputs`` in training mode
    (``sgn_splatfacto_scene_graph.py:305-366``): ``models[0]`` is the background, ``models[i>0]`` rigid objects
    whose parameters live in the object's local frame; ``poses[i]`` = [R(9) t(3) q_o2w(4)], ``idft[i]`` = Fourier
    weights of the frame.  Four raster passes like the reference: rgb+alpha, depth, objects-only accumulation,
    background-only accumulation.  ``fused=True`` runs the main pass through :mod:`sgn_rast.fused` (no transform /
    activation / concat kernels) and skips the SH evaluation whose result the reference throws away in the two
    accumulation passes (``:285``).  ``rasterize_mode``: as :func:`render` / :func:`render_fused`, in every pass.
    ``absgrad=True`` (fused path only; ``ValueError`` otherwise): the main colour pass sums the absolute screen-space
    gradients (:func:`render_fused`); after ``backward()``, ``out.xys_absgrad_parts()`` returns the per-sub-model
    slices of ``out.xys.absgrad`` in model order — what each sub-model's ``after_train`` reads under
    ``DensifyConfig(absgrad=True)``.  The accumulation passes add nothing to it.
    ``rolling_shutter`` / ``object_velocities`` [len(models), 3]: as :func:`render` / :func:`render_fused`, on both
    paths — the main projection's outputs are sheared once, and every pass (depth, the two accumulations) reads them;
    a moving object shears with its own velocity.  (:func:`render_scene_graph_eval` does not take them.)"""
    antialiased = antialiased_mode(rasterize_mode)
    _shutter.check(rolling_shutter)
    if absgrad and not fused:
        raise ValueError("absgrad is not supported on the drop-in operators (gsplat 0.1.x surface): use fused=True")
    dev = models[0]["means"].device
    H, W = cam.height, cam.width
    counts = [m["means"].shape[0] for m in models]
    bg_zero = _zeros3(dev)
    cat = lambda key: torch.cat([m[key] for m in models], dim=0)                        # :355-360
    if fused:
        from . import fused as F_
        P, object_ids, idft_p = _fused_scene_params(models, idft, sh_parts)
        # `groups`: object_acc / background_acc ride on the main pass's walk (rasterize_gaussians_fused(group_split));
        # False keeps the round-3 form, two more id-range passes, for A/B and for the tests
        out = render_fused(P, cam, sh_degree_to_use, block_width, with_depth=True, object_ids=object_ids,
                           poses=poses, idft=idft_p, group_split=counts[0] if groups else None,
                           rasterize_mode=rasterize_mode, absgrad=absgrad, rolling_shutter=rolling_shutter,
                           object_velocities=object_velocities)
        if absgrad:
            out.xys_absgrad_parts = lambda: torch.split(out.xys.absgrad, counts)
        if groups:
            out.object_acc, out.background_acc = out.acc_tail, out.acc_head                 # :364-366
            return out
        opac_arg, raster = (out.opacities if antialiased else P["opacity_logits"]), F_.rasterize_gaussians_fused
    else:
        P, world_means, dcs = _world_scene_params(models, poses, idft)
        out = render(P, cam, sh_degree_to_use, block_width, with_depth=True, ops=ops,   # :363
                     split_counts=counts, caller_syncs=caller_syncs, rasterize_mode=rasterize_mode,
                     rolling_shutter=rolling_shutter, object_velocities=object_velocities)
        if getattr(out, "empty", False):        # nothing visible: the sub-model passes return their empty outputs too
            out.object_acc = torch.zeros(H, W, device=dev)
            out.background_acc = torch.zeros(H, W, device=dev)
            return out
        opac_arg, raster = out.opacities, ops.rasterize_gaussians

    def submodel_acc(lo: int, hi: int, which):                                          # :255-303
        if hi <= lo:
            return torch.zeros(H, W, device=dev)
        if fused:
            # colour is irrelevant for an accumulation-only pass; the full geometry tensors + id_range reuse the
            # main pass's binning (one-entry cache) instead of slicing and sorting again
            rgbs = _zero_colors(sum(counts), dev)
            _, acc = raster(out.xys, out.depths, out.radii, out.conics, out.num_tiles_hit, rgbs, opac_arg, H, W,
                            block_width, background=bg_zero, return_alpha=True, id_range=(lo, hi),
                            opacity_is_logit=not antialiased)
            return acc
        return _submodel_raster(models, world_means, dcs, out, range(*which), cam, sh_degree_to_use, block_width, bg_zero,
                                ops, caller_syncs, antialiased)[1]

    n_bg = counts[0]
    out.object_acc = submodel_acc(n_bg, sum(counts), (1, len(models)))                   # :364-365
    out.background_acc = submodel_acc(0, n_bg, (0, 1))                                   # :366
    return out


def _eval_finish(rgb: torch.Tensor, alpha: torch.Tensor, sky: Optional[torch.Tensor]):
    """``render_gaussian_attrs`` after its rasterization, eval mode (sgn_splatfacto.py:968-975) -> (rgb, alpha[H,W,1])."""
    alpha = alpha[..., None]                                                           # :968
    rgb = torch.clamp(rgb, max=1.0)                                                    # :969
    if sky is not None:
        rgb = rgb * alpha + sky * (1 - alpha)                                          # :972
    return rgb.clamp(0.0, 1.0), alpha                                                  # :974-975 (not self.training)


def _eval_nothing_visible(H: int, W: int, background: torch.Tensor, sky: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The reference's constant outputs when no Gaussian projects onto the image (sgn_splatfacto.py:878-886)."""
    dev = background.device
    out = {"rgb": background.repeat(H, W, 1), "accumulation": torch.zeros(H, W, 1, device=dev),
           "depth": torch.zeros(H, W, 1, device=dev)}
    if sky is not None:
        out["sky"] = sky
    return out


def render_eval(P: Dict[str, torch.Tensor], cam: Camera, background: torch.Tensor, sky: Optional[torch.Tensor] = None,
                sh_degree: int = 3, block_width: int = 16, fused: bool = True, ops=_hip_ops,
                rasterize_mode: str = "classic", rolling_shutter=None) -> Dict[str, torch.Tensor]:
    """``SplatfactoModel.get_outputs`` as ``get_outputs_for_camera`` reaches it: ``self.training == False`` under
    ``torch.no_grad()`` — the full SH degree whatever the step (sgn_splatfacto.py:937-938), a sky image looked up without
    jitter (``sky`` [H,W,3], e.g. ``sgn_rast.sky.sky_color(base, ..., jitter=None)``; None: ``use_sky_sphere=False``) and
    the final ``rgb.clamp(0, 1)`` (:974-975).  Returns the reference's keys: ``rgb`` [H,W,3], ``accumulation`` [H,W,1],
    ``depth`` [H,W,1] and ``sky`` when given.  ``fused=False`` is the call-site replay on the drop-in operators (or the
    oracle's, ``ops``); ``fused=True`` the fused front ends with the depth channel riding in the colour pass.
    ``rasterize_mode``, ``rolling_shutter``: as :func:`render` / :func:`render_fused` (the sky image is NOT rotated per
    line)."""
    antialiased_mode(rasterize_mode)
    _shutter.check(rolling_shutter)
    H, W = cam.height, cam.width
    with torch.no_grad():
        if fused:
            out = render_fused(P, cam, sh_degree, block_width, background=background, with_depth=True,
                               rasterize_mode=rasterize_mode, rolling_shutter=rolling_shutter)
            if bool(out.radii.sum() == 0):                                             # :878
                return _eval_nothing_visible(H, W, background, sky)
        else:
            out = render(P, cam, sh_degree, block_width, background=background, with_depth=True, ops=ops,
                         retain_xys_grad=False, rasterize_mode=rasterize_mode, rolling_shutter=rolling_shutter)
            if getattr(out, "empty", False):
                return _eval_nothing_visible(H, W, background, sky)
        rgb, alpha = _eval_finish(out.rgb, out.alpha, sky)
        res = {"rgb": rgb, "accumulation": alpha, "depth": out.depth}
        if sky is not None:
            res["sky"] = sky                                                           # :998-999
        return res


def render_scene_graph_eval(models, poses: torch.Tensor, idft: torch.Tensor, cam: Camera, background: torch.Tensor,
                            sky: Optional[torch.Tensor] = None, sh_degree: int = 3, block_width: int = 16,
                            fused: bool = True, ops=_hip_ops, layered: bool = True,
                            rasterize_mode: str = "classic") -> Dict[str, torch.Tensor]:
    """``SplatfactoSceneGraphModel.get_outputs`` in EVAL mode (``self.training == False`` under ``torch.no_grad()``:
    what the reference's render / eval scripts and the trainer's eval image go through) — :func:`render_eval`'s semantics
    for the scene, the two sub-model accumulations, and the two decomposition images of
    ``sgn_splatfacto_scene_graph.py:367-372``.  ``models[0]`` is the background, ``models[i>0]`` the objects annotated at
    this frame (``poses`` / ``idft`` rows as in :func:`render_scene_graph`); ``sky`` [H,W,3] is the sky image looked up
    without jitter, or None.  Returns the reference's keys and shapes: ``rgb`` [H,W,3], ``accumulation`` / ``depth`` /
    ``object_acc`` / ``background_acc`` [H,W,1], ``sky`` when given, ``background_rgb`` (the background over the sky) and
    ``object_rgb`` (the objects alone, no sky) [H,W,3].

    ``fused=False``: the literal replay — six rasterizations (rgb + alpha, depth, two accumulations, two images), the
    sub-model tensors aggregated with ``torch.cat`` as ``get_submodel_output`` does, on ``ops`` (the drop-in operators or
    the CPU oracle's).  ``fused=True``: the fused projection and SH, ONE layered rasterization
    (:func:`sgn_rast.layers.rasterize_layers`) and one finishing launch.  ``layered=False`` keeps the fused front ends
    but renders the way the training-side API allows — the main pass with the depth channel and the two group
    accumulations, two more ``id_range`` colour passes, torch expressions after them — for A/B runs and for the tests: the
    layered call returns the same bits.  ``rasterize_mode``: as :func:`render` / :func:`render_fused`, in every pass and
    layer."""
    antialiased = antialiased_mode(rasterize_mode)
    dev = models[0]["means"].device
    H, W = cam.height, cam.width
    # "prevent empty object" (:338-339): a model without points takes no part in the frame
    keep = [i for i, m in enumerate(models) if i == 0 or m["means"].shape[0] > 0]
    if len(keep) < len(models):
        models = [models[i] for i in keep]
        poses, idft = poses[keep], idft[keep]
    counts = [m["means"].shape[0] for m in models]
    n_bg, n_all = counts[0], sum(counts)
    no_objects = len(models) == 1
    zero1 = lambda: torch.zeros(H, W, 1, device=dev)

    def empty_objects(res):
        # no object at this frame (:263-267): the accumulation pass returns `empty`, the rgb pass {'rgb': empty,
        # 'depth': empty} — ONE-channel zeros, and the only case in which `object_depth` exists
        res["object_acc"], res["object_rgb"], res["object_depth"] = zero1(), zero1(), zero1()

    def nothing_visible():
        # :878-886 for the scene; the sub-model passes have nothing to composite either: zero layers (T = 1, C = 0)
        # through the same finish — as render_scene_graph does for its `empty` case
        res = _eval_nothing_visible(H, W, background, sky)
        blank = background.repeat(H, W, 1)
        res["background_acc"] = zero1()
        res["background_rgb"] = _eval_finish(blank, torch.zeros(H, W, device=dev), sky)[0]
        if no_objects:
            empty_objects(res)
        else:
            res["object_acc"] = zero1()
            res["object_rgb"] = _eval_finish(blank, torch.zeros(H, W, device=dev), None)[0]
        return res

    with torch.no_grad():
        if fused:
            from . import fused as F_, layers
            P, object_ids, idft_p = _fused_scene_params(models, idft)
            xys, depths, radii, conics, comp, num_tiles_hit, _cov3d = F_.project_gaussians_fused(
                P["means"], P["log_scales"], P["quats"], cam.viewmat[:3, :], cam.fx, cam.fy, cam.cx, cam.cy, H, W,
                block_width, object_ids=object_ids, poses=poses)
            opac, logit = P["opacity_logits"], True          # (one opacity tensor for every pass, as render_fused)
            if antialiased:
                opac, logit = F_.antialiased_opacities(P["opacity_logits"], comp), False
            _hip_ops.prefetch_binning(xys, depths, radii, conics, num_tiles_hit, opac, H, W, block_width,
                                      opacity_is_logit=logit)
            rgbs = F_.spherical_harmonics_fused(sh_degree, P["means"], cam.cam_pos, P["features_dc"],
                                                P["features_rest"], object_ids=object_ids, idft=idft_p, poses=poses)
            if bool(radii.sum() == 0):                                                 # :878
                return nothing_visible()
            if not layered:
                geo = (xys, depths, radii, conics, num_tiles_hit, rgbs, opac, H, W, block_width)
                img_all, alpha, D, acc_h, acc_t = F_.rasterize_gaussians_fused(
                    *geo, background=background, return_alpha=True, depth_channel=True, group_split=n_bg,
                    opacity_is_logit=logit)
                part = lambda lo, hi: (F_.rasterize_gaussians_fused(*geo, background=background, return_alpha=True,
                                                                    id_range=(lo, hi), opacity_is_logit=logit)[0]
                                       if hi > lo else background.repeat(H, W, 1))
                rgb, a = _eval_finish(img_all, alpha, sky)
                res = {"rgb": rgb, "accumulation": a, "depth": torch.where(a > 1e-3, D[..., None] / a, 10)}   # :995
                if sky is not None:
                    res["sky"] = sky
                res["background_acc"] = acc_h[..., None]
                res["background_rgb"] = _eval_finish(part(0, n_bg), acc_h, sky)[0]
                if no_objects:
                    empty_objects(res)
                else:
                    res["object_acc"] = acc_t[..., None]
                    res["object_rgb"] = _eval_finish(part(n_bg, n_all), acc_t, None)[0]
                return res
            img, Ts, D = layers.rasterize_layers(xys, depths, radii, conics, num_tiles_hit, rgbs, opac, H, W, block_width,
                                                 background, n_bg, opacity_is_logit=logit)
            rgb3, acc3, depth = layers.finish(img, Ts, D, sky)
            res = {"rgb": rgb3[0], "accumulation": acc3[0][..., None], "depth": depth[..., None]}
            if sky is not None:
                res["sky"] = sky
            res["background_acc"], res["background_rgb"] = acc3[1][..., None], rgb3[1]
            if no_objects:
                empty_objects(res)
            else:
                res["object_acc"], res["object_rgb"] = acc3[2][..., None], rgb3[2]
            return res
        Pw, world_means, dcs = _world_scene_params(models, poses, idft)
        out = render(Pw, cam, sh_degree, block_width, background=background, with_depth=True, ops=ops,   # :363
                     split_counts=counts, retain_xys_grad=False, rasterize_mode=rasterize_mode)
        if getattr(out, "empty", False):
            return nothing_visible()
        rgb, alpha = _eval_finish(out.rgb, out.alpha, sky)
        res = {"rgb": rgb, "accumulation": alpha, "depth": out.depth}
        if sky is not None:
            res["sky"] = sky
        sub = lambda which: _submodel_raster(models, world_means, dcs, out, range(*which), cam, sh_degree, block_width,
                                             background, ops, True, antialiased)
        objects, backgr = (1, len(models)), (0, 1)
        if not no_objects:
            res["object_acc"] = sub(objects)[1][..., None]                             # :364-365
        res["background_acc"] = sub(backgr)[1][..., None]                              # :366
        res["background_rgb"] = _eval_finish(*sub(backgr), sky)[0]                     # :369-370
        if no_objects:
            empty_objects(res)
        else:
            res["object_rgb"] = _eval_finish(*sub(objects), None)[0]                   # :371-372
        return res


def loss_weights(cam: Camera, seed: int = 7, device="cpu", dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    w_img = torch.rand(cam.height, cam.width, 3, generator=g)
    w_a = torch.rand(cam.height, cam.width, generator=g)
    return w_img.to(device=device, dtype=dtype), w_a.to(device=device, dtype=dtype)


def composite_sky(out: SimpleNamespace, cam: Camera, sky_base: torch.Tensor, c2w: torch.Tensor,
                  train: bool = True, fused: bool = False, sky_fn=None) -> None:
    """use_sky_sphere branch of the reference (sgn_splatfacto.py:875-876, 969-972): look the sky colour up in the
    cube map and blend it behind the splats, in place on ``out.rgb``.  ``fused`` does lookup + blend in one kernel
    (``sky.sky_blend``); ``sky_fn(base, H, W, fx, fy, cx, cy, c2w, jitter)`` lets the parity tests substitute the
    oracle's lookup."""
    from . import sky as _sky
    H, W = cam.height, cam.width
    jitter = torch.rand(2, H, W, device=sky_base.device) if train else None
    out.sky_jitter = jitter
    if fused:
        out.rgb, out.sky = _sky.sky_blend(sky_base, out.rgb, out.alpha, cam.fx, cam.fy, cam.cx, cam.cy, c2w, jitter)
        return
    fn = sky_fn or _sky.sky_color
    sky_capture = fn(sky_base, H, W, cam.fx, cam.fy, cam.cx, cam.cy, c2w, jitter)      # :876
    alpha = out.alpha[..., None]                                                       # :968
    rgb = torch.clamp(out.rgb, max=1.0)                                                # :969
    out.rgb = rgb * alpha + sky_capture * (1 - alpha)                                  # :972
    out.sky = sky_capture


def train_step(P: Dict[str, torch.Tensor], cam: Camera, w_img: torch.Tensor, w_a: torch.Tensor,
               sh_degree_to_use: int = 3, block_width: int = 16, with_depth: bool = False, ops=_hip_ops,
               reducer=None, fused: bool = False, sky: Optional[dict] = None, gt: Optional[torch.Tensor] = None,
               ssim_lambda: float = 0.2, loss_fn=None, caller_syncs: bool = False, zero_grad: bool = True,
               mask: Optional[torch.Tensor] = None, lidar_depth: Optional[torch.Tensor] = None,
               depth_loss_mult: float = 0.1, depth_loss_kind: str = "l1", rasterize_mode: str = "classic",
               absgrad: bool = False, densifier=None, step: int = 0, appearance=None, rolling_shutter=None,
               **fused_kw) -> SimpleNamespace:
    """One "train-step image": project fwd -> SH fwd -> rasterize(return_alpha) fwd -> scalar loss ->
    full backward to means / log-scales / raw quats / opacity logits / SH coefficients (the metric's definition,
    SURVEY.md §8d: the operator sequence; ``caller_syncs=True`` adds the two host syncs of the reference's own model
    code, sgn_splatfacto.py:878,944, as the scene-graph replay always does).  ``sky`` =
    {"base": cube map leaf [6,R,R,3], "c2w": [3,4]} adds the reference's sky-sphere branch.  ``gt`` [H,W,3] swaps the
    synthetic linear image loss for the reference's photometric loss (``sgn_splatfacto.py:1084-1087``: (1-l) L1 + l
    (1 - SSIM) on ``rgb.clamp(max=1)``), through ``sgn_rast.loss`` or the ``loss_fn(rgb, gt, l)`` the tests pass.
    ``mask`` (bool / uint8 [H,W] or [H,W,1]) is the batch's pixel mask of that loss (``:1081-1083``), see
    ``sgn_rast.loss.l1_ssim``; a ``loss_fn`` receives it as the keyword ``mask`` only when it is given.
    ``lidar_depth`` [H,W] float32 (``sgn_rast.lidar.splat_depth``; 0 = no return) adds the LiDAR depth term
    ``depth_loss_mult * lidar.depth_loss(*features.expected_depth(...), lidar_depth, depth_loss_kind, mask)``: the
    expected depth is composited over the list the RGB pass binned (nothing is binned again) and ``out.depth_loss`` holds
    the term's value; an empty view contributes nothing.  ``rasterize_mode="antialiased"`` multiplies the opacities by
    the projection's compensation factor (:func:`render` / :func:`render_fused`), in the LiDAR term's pass too.
    ``absgrad=True`` (``fused=True`` only; ``ValueError`` otherwise): the colour pass sums the absolute screen-space
    gradients, ``out.xys.absgrad`` [N,2] after the backward.  ``densifier`` (a :class:`sgn_rast.densify.Densifier`):
    its ``after_train(step, ...)`` runs behind the backward with this render's ``xys.grad`` — or, under
    ``DensifyConfig(absgrad=True)``, its ``xys.absgrad`` — radii and image size; a densifier that has a
    ``regularizer()`` (:class:`sgn_rast.mcmc.MCMCDensifier`) gets its value added to the loss.
    ``appearance=(grids, index)`` — a :class:`sgn_rast.appearance.BilateralGrids` module or its ``[num, L, Hg, Wg, 12]``
    tensor, and the image's (or sensor's) number — corrects ``out.rgb`` with ``appearance.slice_image`` after the sky
    composite and before the photometric loss, whose own clamp and mask then act on the corrected colour; the
    uncorrected image is kept as ``out.rgb_raw``, the grids' gradient lands in ``grids.grad`` (this step does not reset
    it).  It needs ``gt`` (``ValueError`` before the render otherwise).  Out of scope: ``train_step_views``, the
    scene-graph step and the data-parallel exchange of the grids' gradients do not take it.
    ``rolling_shutter`` (a :class:`sgn_rast.shutter.RollingShutter`): the render is the rolling sensor's
    (:func:`render` / :func:`render_fused`); the LiDAR term, absgrad and the densifier read the sheared ``out.xys`` /
    ``out.radii``.  Out of scope: ``train_step_views``, the per-line rotation of the sky lookup and of the SH view
    directions, learnable velocities, and the data-parallel exchange (the pass has nothing to exchange)."""
    antialiased = antialiased_mode(rasterize_mode)
    _shutter.check(rolling_shutter)
    if appearance is not None:
        from . import appearance as _appearance
        if gt is None:
            raise ValueError("appearance corrects the image the photometric loss compares: pass gt as well")
        app_grids, app_index = appearance
        if isinstance(app_grids, _appearance.BilateralGrids):
            app_grids = app_grids.grids
        if not isinstance(app_grids, torch.Tensor) or app_grids.dim() != 5 or app_grids.shape[-1] != 12 \
                or app_grids.dtype != torch.float32 or isinstance(app_index, bool) or not isinstance(app_index, int) \
                or not 0 <= app_index < app_grids.shape[0]:
            raise ValueError("appearance must be (grids [num, L, Hg, Wg, 12] float32 or BilateralGrids, index in range)")
    if absgrad and not fused:
        raise ValueError("absgrad is not supported on the drop-in operators (gsplat 0.1.x surface): use fused=True")
    if densifier is not None and densifier.cfg.absgrad and not absgrad:
        raise ValueError("DensifyConfig(absgrad=True) reads xys.absgrad: pass absgrad=True")
    if mask is not None:           # host-side errors first: before the render, let alone the loss, launches anything
        if gt is None:
            raise ValueError("mask applies to the photometric loss: pass gt as well")
        if loss_fn is None:
            from .loss import check_mask
            check_mask(mask, cam.height, cam.width)
    if lidar_depth is not None:
        from . import features, lidar
        lidar.check_target(lidar_depth, cam.height, cam.width)
        if depth_loss_kind not in lidar.KINDS:
            raise ValueError(f"depth_loss_kind must be one of {sorted(lidar.KINDS)}, got {depth_loss_kind!r}")
        if block_width != 16:
            raise ValueError("the LiDAR depth term exists for 16x16 tiles only (block_width=16)")
        if mask is not None:
            lidar.check_mask(mask, cam.height, cam.width)
    if zero_grad:                  # (False: the caller's loop owns the gradients — keeps and accumulates them, or resets them)
        for p in P.values():
            p.grad = None
        if sky is not None:
            sky["base"].grad = None
    if fused:
        out = render_fused(P, cam, sh_degree_to_use, block_width, with_depth=with_depth, rasterize_mode=rasterize_mode,
                           absgrad=absgrad, rolling_shutter=rolling_shutter, **fused_kw)
    else:
        out = render(P, cam, sh_degree_to_use, block_width, with_depth=with_depth, ops=ops,
                     caller_syncs=caller_syncs, rasterize_mode=rasterize_mode, rolling_shutter=rolling_shutter)
    if sky is not None:
        composite_sky(out, cam, sky["base"], sky["c2w"], train=sky.get("train", True), fused=fused,
                      sky_fn=sky.get("fn"))
    if appearance is not None:
        out.rgb_raw = out.rgb
        out.rgb = _appearance.slice_image(app_grids, app_index, out.rgb)
    n_pix = cam.height * cam.width
    if gt is not None:
        if loss_fn is not None:                                                        # tests: the oracle's loss
            rgb = out.rgb if sky is not None else torch.clamp(out.rgb, max=1.0)        # :969 (sky path clamps inside)
            photo = loss_fn(rgb, gt, ssim_lambda) if mask is None else loss_fn(rgb, gt, ssim_lambda, mask=mask)
        else:
            from .loss import photometric_loss
            photo = photometric_loss(out.rgb, gt, ssim_lambda, clamp_max=None if sky is not None else 1.0, mask=mask)
        loss = photo + (out.alpha * w_a).sum() / n_pix
    else:
        loss = ((out.rgb * w_img).sum() + (out.alpha * w_a).sum()) / n_pix
    if lidar_depth is not None:
        if getattr(out, "empty", False):
            out.depth_loss = torch.zeros((), device=loss.device)
        else:
            # the opacity tensor the RGB pass binned under: its list is reused
            logit = bool(fused) and not antialiased
            opac = P["opacity_logits"] if logit else out.opacities
            dsum, acc = features.expected_depth(out.xys, out.depths, out.radii, out.conics, out.num_tiles_hit, opac,
                                                cam.height, cam.width, block_width, opacity_is_logit=logit)
            term = lidar.depth_loss(dsum, acc, lidar_depth, depth_loss_kind, mask)
            loss = loss + depth_loss_mult * term
            out.depth_loss = term.detach()
    if hasattr(densifier, "regularizer"):     # sgn_rast.mcmc.MCMCDensifier: the opacity / scale regulariser
        loss = loss + densifier.regularizer()
    if loss.requires_grad:        # an empty view (the reference's constant outputs) has nothing to differentiate
        loss.backward()
    if reducer is not None:
        reducer.finish()
    if densifier is not None:     # (an empty view: no gradient, no absgrad — after_train counts it as "saw nothing")
        ran = loss.requires_grad
        densifier.after_train(step, out.xys.grad if ran else None, out.radii, (cam.height, cam.width),
                              absgrad=getattr(out.xys, "absgrad", None) if ran else None)
    out.loss = loss.detach()
    return out

"""GPU (-m gpu): the absgrad statistic (`rasterize_gaussians_fused(absgrad=True)` -> `xys.absgrad`, `sgn_raster_bwd_abs`,
csrc/raster_absgrad.hip) against the float64 restatement of the per-pixel reverse walk (tests/absgrad_fp64.py; the CPU
test test_absgrad_fp64.py holds it to the torch oracle and asserts that at most 2 % of the visible Gaussians of these
scenes are threshold-adjacent), on a 40x56 image — 3x4 tiles of 16 with ragged right and bottom edges — with ~300
Gaussians, ten of them over several tiles and a cluster of 60 over one tile, at thresholds that send this size through
every launch shape and both ways through a list."""
import numpy as np
import pytest
import torch

import absgrad_fp64 as A
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(adapt_bwd=16, batch_bwd=8)        # this size reaches the long-walk kernel and the LDS-staged walk


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _render(sc, absgrad, loss="weights", group_split=None, acc_in_loss=False, backward=True):
    """One colour pass over the scene's arrays (probabilities: the kernels see the reference's very opacities) and its
    backward -> (outputs, leaves [xys, conics, colors, opacities])."""
    from sgn_rast import fused, ops
    leaves = [_t(sc.xys).requires_grad_(True), _t(sc.conics).requires_grad_(True), _t(sc.colors).requires_grad_(True),
              _t(sc.opacities).requires_grad_(True)]
    ops.clear_binning_cache()
    out = fused.rasterize_gaussians_fused(leaves[0], _t(sc.depths), _t(sc.radii), leaves[1], _t(sc.num_tiles_hit),
                                          leaves[2], leaves[3], sc.H, sc.W, sc.block, background=_t(sc.background),
                                          return_alpha=True, opacity_is_logit=False, absgrad=absgrad,
                                          group_split=group_split)
    if backward:
        if loss == "rgb_sum":
            val = out[0].sum()
        else:
            val = (out[0] * _t(sc.w_img)).sum() + (out[1] * _t(sc.w_alpha)).sum()
        if acc_in_loss:
            val = val + (out[3] * _t(sc.w_alpha).flip(0)).sum()
        val.backward()
        torch.cuda.synchronize()
    return out, leaves


def _check_against_fp64(sc, ref, absgrad, tol, what):
    keep = torch.from_numpy(~ref.adjacent)
    got, exp = absgrad.cpu().double()[keep], torch.from_numpy(ref.absolute)[keep]
    rel = rel_l2(got, exp)
    print(f"[absgrad] {what}: rel-L2 {rel:.2e} over {int(keep.sum())} of {sc.n} Gaussians (bound {tol:.0e})")
    assert rel <= tol, (what, rel)
    # rows nothing touched stay exactly zero
    untouched = torch.from_numpy(~ref.visible & ~ref.adjacent)
    assert float(absgrad.cpu()[untouched].abs().max()) == 0.0


ROUTES = {
    "two-kernel": dict(block=16, tile_order=True),          # long-walk kernel + short-walk kernel
    "mode0-no-order": dict(block=16, tile_order=False),     # the in-kernel adaptive split, no launch order
    "mode0-block8": dict(block=8, tile_order=True),         # the in-kernel adaptive split, 8x8 tiles
}


@pytest.mark.parametrize("reduce_mode", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
def test_absgrad_equals_the_fp64_reference(route, reduce_mode):
    from sgn_rast import config
    r = ROUTES[route]
    sc, ref = A.reference(A.SEED, r["block"])
    with config.override(exact_exp=1, reduce_mode=reduce_mode, tile_order=r["tile_order"], **SMALL):
        _out, leaves = _render(sc, True)
    xys = leaves[0]
    assert xys.absgrad.shape == (sc.n, 2) and xys.absgrad.dtype is torch.float32 and not xys.absgrad.requires_grad
    _check_against_fp64(sc, ref, xys.absgrad, 1e-4, f"{route}, reduce_mode {reduce_mode}")
    # always: the absolute sum dominates the signed one
    assert bool((xys.absgrad >= xys.grad.abs() - 1e-6 * xys.absgrad).all())
    # ... and the signed gradient is the reference's signed sum, same tolerance
    keep = torch.from_numpy(~ref.adjacent)
    assert rel_l2(xys.grad.cpu()[keep], torch.from_numpy(ref.signed)[keep]) <= 1e-4


def test_absgrad_at_the_default_thresholds():
    """Default adapt_bwd / batch_bwd: only the scalar-chase walk and the short-walk kernel run at this size."""
    from sgn_rast import config
    sc, ref = A.reference(A.SEED, 16)
    with config.override(exact_exp=1):
        _out, leaves = _render(sc, True)
    _check_against_fp64(sc, ref, leaves[0].absgrad, 1e-4, "default thresholds")


def test_absgrad_with_the_hardware_exp():
    from sgn_rast import config
    sc, ref = A.reference(A.SEED, 16)
    with config.override(exact_exp=0, **SMALL):
        _out, leaves = _render(sc, True)
    _check_against_fp64(sc, ref, leaves[0].absgrad, 1e-3, "hardware exp")


@pytest.mark.parametrize("route", list(ROUTES))
def test_signed_outputs_do_not_move(route):
    from sgn_rast import config
    r = ROUTES[route]
    sc, _ref = A.reference(A.SEED, r["block"])
    with config.override(exact_exp=1, tile_order=r["tile_order"], **SMALL):
        out_a, with_abs = _render(sc, True)
        out_p, plain = _render(sc, False)
    assert torch.equal(out_a[0], out_p[0]) and torch.equal(out_a[1], out_p[1])        # the forward: bit-equal
    assert not hasattr(plain[0], "absgrad")
    for name, x, y in zip(("v_xy", "v_conic", "v_colors", "v_opacity"), with_abs, plain):
        rel = rel_l2(x.grad, y.grad)
        print(f"[absgrad] {route}: {name} with / without absgrad rel-L2 {rel:.2e}")
        assert rel < 1e-5, (name, rel)


def test_centred_isotropic_gaussian_cancels():
    from sgn_rast import config
    sc, ref = A.reference(A.SEED, 16, single=True, rgb_sum_loss=True)
    with config.override(exact_exp=1, **SMALL):
        _out, leaves = _render(sc, True, loss="rgb_sum")
    xys = leaves[0]
    print(f"[absgrad] centred Gaussian: grad {xys.grad.tolist()}, absgrad {xys.absgrad.tolist()}, "
          f"fp64 {ref.absolute.tolist()}")
    assert bool((xys.grad.abs() <= 1e-4 * xys.absgrad).all())
    assert rel_l2(xys.absgrad.cpu(), torch.from_numpy(ref.absolute)) <= 1e-4


def test_only_the_main_walk_contributes_with_groups():
    """A `group_split` render whose loss includes acc_head: one more (plain) reverse walk chained into the same
    workspace.  Its absgrad is the absgrad of the same render without the accumulation term; its signed gradients are
    those of the absgrad=False run."""
    from sgn_rast import config, ops
    sc, ref = A.reference(A.SEED, 16)
    split = 150
    with config.override(exact_exp=1, **SMALL):
        before = ops.group_stats["backward_passes"]
        _o, with_acc = _render(sc, True, group_split=split, acc_in_loss=True)
        assert ops.group_stats["backward_passes"] == before + 1
        _o, without_acc = _render(sc, True, group_split=split)
        assert ops.group_stats["backward_passes"] == before + 1
        _o, plain = _render(sc, False, group_split=split, acc_in_loss=True)
    a, b = with_acc[0].absgrad, without_acc[0].absgrad
    print(f"[absgrad] groups: absgrad with / without the accumulation term rel-L2 {rel_l2(a, b):.2e}")
    assert rel_l2(a, b) < 1e-5
    _check_against_fp64(sc, ref, a, 1e-4, "group_split, acc_head in the loss")
    for name, x, y in zip(("v_xy", "v_conic", "v_colors", "v_opacity"), with_acc, plain):
        assert rel_l2(x.grad, y.grad) < 1e-5, name
    # the accumulation term did reach the signed gradient
    assert rel_l2(with_acc[0].grad, without_acc[0].grad) > 1e-3


def test_second_backward_overwrites_and_empty_view_gives_zeros():
    from sgn_rast import config, fused, ops
    sc, _ref = A.reference(A.SEED, 16)
    with config.override(exact_exp=1, **SMALL):
        xys = _t(sc.xys).requires_grad_(True)
        ops.clear_binning_cache()
        img, alpha = fused.rasterize_gaussians_fused(
            xys, _t(sc.depths), _t(sc.radii), _t(sc.conics), _t(sc.num_tiles_hit), _t(sc.colors), _t(sc.opacities), sc.H,
            sc.W, 16, background=_t(sc.background), return_alpha=True, opacity_is_logit=False, absgrad=True)
        loss = (img * _t(sc.w_img)).sum() + (alpha * _t(sc.w_alpha)).sum()
        loss.backward(retain_graph=True)
        first, first_grad = xys.absgrad.clone(), xys.grad.clone()
        loss.backward()
        assert rel_l2(xys.grad, 2 * first_grad) < 1e-5           # autograd accumulates .grad ...
        assert rel_l2(xys.absgrad, first) < 1e-5                 # ... the statistic is assigned per backward
        # nothing visible: zeros, no error
        xys0 = _t(sc.xys).requires_grad_(True)
        zero_r, zero_n = torch.zeros_like(_t(sc.radii)), torch.zeros_like(_t(sc.num_tiles_hit))
        ops.clear_binning_cache()
        img, alpha = fused.rasterize_gaussians_fused(
            xys0, _t(sc.depths), zero_r, _t(sc.conics), zero_n, _t(sc.colors), _t(sc.opacities), sc.H, sc.W, 16,
            background=_t(sc.background), return_alpha=True, opacity_is_logit=False, absgrad=True)
        (img.sum() + alpha.sum()).backward()
        assert xys0.absgrad.shape == (sc.n, 2) and float(xys0.absgrad.abs().max()) == 0.0
        assert float(xys0.grad.abs().max()) == 0.0


def test_unsupported_call_shapes_raise():
    from sgn_rast import features, fused, scenes, views
    sc, _ref = A.reference(A.SEED, 16)
    geo = (_t(sc.xys), _t(sc.depths), _t(sc.radii), _t(sc.conics), _t(sc.num_tiles_hit))
    with pytest.raises(ValueError, match="absgrad is not supported"):
        fused.rasterize_gaussians_fused(*geo, _t(sc.colors), _t(sc.opacities), sc.H, sc.W, 16, id_range=(0, 100),
                                        opacity_is_logit=False, absgrad=True)
    with pytest.raises(ValueError, match="absgrad is not supported"):
        features.rasterize_features(*geo, _t(sc.colors), _t(sc.opacities), sc.H, sc.W, absgrad=True)
    cam = scenes.make_camera(sc.W, sc.H, 60.0, device=DEV)
    P = scenes.make_gaussians(50, cam, device=DEV)
    with pytest.raises(ValueError, match="absgrad is not supported"):
        views.render_views(P, [cam, cam], absgrad=True)


def test_train_step_feeds_the_densifier_absgrad():
    """`train_step(absgrad=True)` with `DensifyConfig(absgrad=True)`: Stats.xys_grad_norm is what a Stats.update fed
    `xys.absgrad` by hand leaves — bit for bit — and not what `xys.grad` would have given."""
    from sgn_rast import densify, scenes, step
    cam = scenes.make_camera(56, 40, 60.0, device=DEV)
    raw = scenes.make_gaussians(400, scenes.make_camera(56, 40, 60.0), seed=5, z_range=(1.0, 5.0), device=DEV)
    P = step.leaf_params(raw)
    w_img, w_a = step.loss_weights(cam, seed=2, device=DEV)
    d = densify.Densifier(P, {k: None for k in densify.PARAM_NAMES}, densify.DensifyConfig(absgrad=True))
    out = step.train_step(P, cam, w_img, w_a, fused=True, absgrad=True, densifier=d, step=0)
    torch.cuda.synchronize()
    assert out.xys.absgrad.shape == (400, 2) and float(out.xys.absgrad.abs().max()) > 0
    by_hand = densify.Stats()
    by_hand.update(out.xys.absgrad, out.radii, (cam.height, cam.width), step=0)
    assert torch.equal(d.stats.xys_grad_norm, by_hand.xys_grad_norm)
    assert torch.equal(d.stats.vis_counts, by_hand.vis_counts)
    signed = densify.Stats()
    signed.update(out.xys.grad, out.radii, (cam.height, cam.width), step=0)
    assert not torch.equal(d.stats.xys_grad_norm, signed.xys_grad_norm)
    assert bool((d.stats.xys_grad_norm >= signed.xys_grad_norm * (1 - 1e-5)).all())
    with pytest.raises(ValueError, match="absgrad"):
        step.train_step(P, cam, w_img, w_a, fused=True, densifier=d, step=1)


def test_scene_graph_parts_concatenate_to_the_whole():
    from sgn_rast import densify, scenes, step
    cam = scenes.make_camera(56, 40, 60.0)
    models, poses, idft = scenes.make_scene_graph(600, cam, n_objects=2, object_frac=0.3, z_range=(1.0, 5.0),
                                                  object_depth=(2.0, 4.0), object_extent=0.3)
    cam_d = scenes.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat.to(DEV), cam.cam_pos.to(DEV))
    Ms = [step.leaf_params({k: v.to(DEV) for k, v in m.items()}) for m in models]
    w_img, w_a = step.loss_weights(cam, seed=3, device=DEV)
    out = step.render_scene_graph(Ms, poses.to(DEV), idft.to(DEV), cam_d, fused=True, absgrad=True)
    ((out.rgb * w_img).sum() + (out.alpha * w_a).sum() + (out.object_acc * w_a).sum()).backward()
    torch.cuda.synchronize()
    parts = out.xys_absgrad_parts()
    assert [p.shape[0] for p in parts] == [m["means"].shape[0] for m in Ms]
    assert torch.equal(torch.cat(parts), out.xys.absgrad) and float(out.xys.absgrad.abs().max()) > 0
    # each part is what that sub-model's after_train reads
    sgd = densify.SceneGraphDensifier(Ms, {k: None for k in densify.PARAM_NAMES}, densify.DensifyConfig(absgrad=True))
    counts = [m["means"].shape[0] for m in Ms]
    sgd.after_train(0, range(len(Ms)), torch.split(out.xys.grad, counts), torch.split(out.radii, counts),
                    (cam.height, cam.width), absgrads=parts)
    for part, dens, radii in zip(parts, sgd.parts, torch.split(out.radii, counts)):
        by_hand = densify.Stats()
        by_hand.update(part, radii, (cam.height, cam.width), step=0)
        assert torch.equal(dens.stats.xys_grad_norm, by_hand.xys_grad_norm)

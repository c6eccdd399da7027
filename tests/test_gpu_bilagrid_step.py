"""GPU: ``step.train_step(appearance=(grids, index))`` on a small scene at 64 x 48, ``fused=True`` with ``gt``: identity
grids change nothing, bit for bit; a random grid gives the loss of the hand-composed ``render_fused`` ->
``slice_image`` -> ``photometric_loss`` bit for bit and its gradient for the grids to the tolerance of
tests/test_gpu_bilagrid.py (against the float64 definition on the gradient that reached the slice); the same with a
mask and with the sky branch; and masked-out pixels give the grids exactly nothing."""
import pytest
import torch

import bilagrid_fp64 as B

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 800
GRID = (4, 3, 2)                 # (Wg, Hg, L)


def _scene(seed=3):
    from sgn_rast import scenes, step
    cam = scenes.make_camera(W, H, 64.0, device="cuda")
    raw = scenes.make_gaussians(N, scenes.make_camera(W, H, 64.0), seed=seed, z_range=(1.0, 5.0), device="cuda")
    w_img, w_a = step.loss_weights(cam, seed=7, device="cuda")
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(4)).cuda()
    return cam, raw, w_img, w_a, gt


def _random_grids(num=3, seed=5):
    from sgn_rast import appearance
    m = appearance.BilateralGrids(num, GRID)
    with torch.no_grad():
        m.grids.add_(0.3 * torch.randn(m.grids.shape, generator=torch.Generator().manual_seed(seed)))
    return m.cuda()


def _sky():
    tex = torch.rand(6, 16, 16, 3, generator=torch.Generator().manual_seed(1)).cuda()
    return {"base": tex.requires_grad_(True), "c2w": torch.eye(4, device="cuda")[:3], "train": False}


def _right_half_masked():
    m = torch.ones(H, W, dtype=torch.bool)
    m[:, W // 2:] = False
    m[5:9, 3:11] = False
    return m.cuda()


def _by_hand(raw, cam, w_a, gt, grids, index, mask=None, sky=None):
    """The composition train_step stands for; also returns the raw image and the gradient that reached the slice."""
    from sgn_rast import appearance, step
    from sgn_rast.loss import photometric_loss
    P = step.leaf_params(raw)
    out = step.render_fused(P, cam, 3, 16)
    if sky is not None:
        step.composite_sky(out, cam, sky["base"], sky["c2w"], train=False, fused=True)
    raw_rgb = out.rgb
    rgb = appearance.slice_image(grids.grids, index, raw_rgb)
    rgb.retain_grad()
    photo = photometric_loss(rgb, gt, 0.2, clamp_max=None if sky is not None else 1.0, mask=mask)
    loss = photo + (out.alpha * w_a).sum() / (H * W)
    grids.grids.grad = None
    loss.backward()
    return loss.detach(), grids.grids.grad.clone(), raw_rgb.detach(), rgb.grad.clone(), P


def test_identity_grids_change_nothing():
    from sgn_rast import appearance, step
    cam, raw, w_img, w_a, gt = _scene()
    plain = step.train_step(step.leaf_params(raw), cam, w_img, w_a, fused=True, gt=gt)
    grids = appearance.BilateralGrids(2, GRID).cuda()
    got = step.train_step(step.leaf_params(raw), cam, w_img, w_a, fused=True, gt=gt, appearance=(grids, 0))
    assert torch.equal(got.loss, plain.loss)
    assert torch.equal(got.rgb.detach(), got.rgb_raw.detach()) and torch.equal(got.rgb_raw.detach(), plain.rgb.detach())
    assert not hasattr(plain, "rgb_raw")
    assert grids.grids.grad is not None and float(grids.grids.grad[1].abs().max()) == 0.0


@pytest.mark.parametrize("variant", ["plain", "mask", "sky", "mask+sky"])
def test_random_grid_equals_the_hand_composition(variant):
    from sgn_rast import step
    cam, raw, w_img, w_a, gt = _scene()
    mask = _right_half_masked() if "mask" in variant else None
    index = 1
    grids = _random_grids()
    sky = _sky() if "sky" in variant else None
    loss_h, grad_h, raw_rgb, v_rgb, P_h = _by_hand(raw, cam, w_a, gt, grids, index, mask, sky)
    sky_grad_h = sky["base"].grad.clone() if sky is not None else None

    grids.grids.grad = None
    P = step.leaf_params(raw)
    got = step.train_step(P, cam, w_img, w_a, fused=True, gt=gt, mask=mask, sky=sky, appearance=(grids, index))
    assert torch.equal(got.loss, loss_h)                                         # bit for bit
    assert torch.equal(got.rgb_raw.detach(), raw_rgb) and not torch.equal(got.rgb.detach(), raw_rgb)
    grad = grids.grids.grad
    assert float(grad[0].abs().max()) == 0.0 and float(grad[2].abs().max()) == 0.0

    # the tolerance of tests/test_gpu_bilagrid.py, on the gradient that reached the slice
    g_cpu = grids.grids.detach()[index].cpu()
    f64 = B.evaluate(g_cpu, raw_rgb, v_rgb)[2]
    f32 = B.evaluate(g_cpu, raw_rgb, v_rgb, torch.float32)[2]
    own = float((f32.double() - f64).abs().max())
    tol = max(8 * own, 4 * 2.0 ** -24 * float(f64.abs().max()))
    for what, g in (("train_step", grad), ("by hand", grad_h)):
        err = float((g[index].cpu().double() - f64).abs().max())
        print(f"[bilagrid step] {variant} {what}: max|hip-f64| {err:.3e}  max|f32-f64| {own:.3e}  tol {tol:.3e}")
        assert err <= tol, (what, err, tol)
    # the Gaussians' (and the sky's) gradients came through the slice in both
    for k in P:
        a, b = P[k].grad, P_h[k].grad
        assert float((a - b).norm()) <= 1e-5 * float(b.norm()) + 1e-12, k
    if sky is not None:
        assert float((sky["base"].grad - sky_grad_h).norm()) <= 1e-5 * float(sky_grad_h.norm())


def test_masked_out_pixels_give_the_grids_exactly_nothing():
    from sgn_rast import step
    cam, raw, w_img, w_a, gt = _scene()
    mask = _right_half_masked()
    grids = _random_grids()
    got = step.train_step(step.leaf_params(raw), cam, w_img, w_a, fused=True, gt=gt, mask=mask, appearance=(grids, 0))
    grad = grids.grids.grad.clone()
    # column Wg - 1 of the grid is reached only from pixels with gx > Wg - 2, i.e. j + 0.5 > W * 2 / 3: all masked out
    assert float(grad[0, :, :, GRID[0] - 1].abs().max()) == 0.0
    assert float(grad[0, :, :, 0].abs().max()) > 0.0
    # a ground truth changed only under the mask changes nothing
    gt2 = torch.where(mask[..., None], gt, 1.0 - gt)
    grids.grids.grad = None
    got2 = step.train_step(step.leaf_params(raw), cam, w_img, w_a, fused=True, gt=gt2, mask=mask, appearance=(grids, 0))
    assert torch.equal(got2.loss, got.loss)
    grad2 = grids.grids.grad
    assert float(grad2[0, :, :, GRID[0] - 1].abs().max()) == 0.0
    # (the kept pixels' sums go through float atomics, equal up to their order: both are held to the one float64 answer)
    _, _, raw_rgb, v_rgb, _ = _by_hand(raw, cam, w_a, gt2, grids, 0, mask)
    assert float(v_rgb[~mask].abs().max()) == 0.0
    g_cpu = grids.grids.detach()[0].cpu()
    f64 = B.evaluate(g_cpu, raw_rgb, v_rgb)[2]
    own = float((B.evaluate(g_cpu, raw_rgb, v_rgb, torch.float32)[2].double() - f64).abs().max())
    tol = max(8 * own, 4 * 2.0 ** -24 * float(f64.abs().max()))
    for g in (grad, grad2):
        assert float((g[0].cpu().double() - f64).abs().max()) <= tol


def test_appearance_needs_gt_before_anything_is_rendered():
    from sgn_rast import step
    cam, raw, w_img, w_a, _ = _scene()
    P = step.leaf_params(raw)
    with pytest.raises(ValueError, match="pass gt as well"):
        step.train_step(P, cam, w_img, w_a, fused=True, appearance=(_random_grids(), 0))
    assert all(p.grad is None for p in P.values())

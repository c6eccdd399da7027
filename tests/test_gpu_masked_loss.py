"""Masked L1 + SSIM loss and the image metrics (csrc/loss.hip masked instantiations via sgn_l1_ssim_masked_fwd/bwd)
against the unchanged oracle applied to the reference's literal expressions (sgn_splatfacto.py:1081-1087, 1135-1151):
``O.l1_ssim_losses(torch.clamp(p, max=1) * m, gt * m)`` with autograd, and ``10 log10(1 / mean((gt m - p m)^2))`` in
fp64.  Tolerances are the ones tests/test_gpu_loss.py uses for the same kernels and reductions.  The content here is white
noise with sigma^2 >> C2 in every window; the smooth, near-converged regime is held per pixel against fp64 in
tests/test_gpu_loss_per_pixel.py."""
import math

import pytest
import torch

from oracle import torch_oracle as O
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

SIZES = [(11, 11), (16, 16), (37, 53), (128, 96), (200, 333), (1280, 1920)]
KINDS = ["bernoulli", "hood", "single"]


def _images(h, w, seed, noise=0.15):
    """tests/test_gpu_loss.py::_images."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(h, w, 3, generator=g)
    pred = (gt + noise * torch.randn(h, w, 3, generator=g)).clamp(0, 1.2)
    return pred, gt


def _mask(kind, h, w, seed=1):
    """bool [H,W], True = keep.  bernoulli: i.i.d. 70 % kept, every window straddles an edge.  hood: the bottom third
    and a rectangle are masked out — at the larger sizes whole 26x26 patches are masked, and neither edge falls on a
    16-pixel tile boundary.  single: one kept pixel."""
    if kind == "bernoulli":
        return torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) < 0.7
    if kind == "hood":
        m = torch.ones(h, w, dtype=torch.bool)
        m[h - h // 3:, :] = False
        m[h // 5: h // 5 + max(1, h // 4), w // 3: w // 3 + max(1, w // 4)] = False
        return m
    m = torch.zeros(h, w, dtype=torch.bool)
    m[h // 2, w // 2] = True
    return m


def _reference(pred, gt, m, clamp=True):
    """(Ll1, ssim, gradient of 0.8 Ll1 + 0.2 (1 - ssim)) of the reference's expressions on the CPU oracle."""
    p = pred.clone().requires_grad_(True)
    mf = m.reshape(m.shape[0], m.shape[1], 1).float()
    rgb = torch.clamp(p, max=1.0) if clamp else p
    l1, s = O.l1_ssim_losses(rgb * mf, gt * mf)
    (0.8 * l1 + 0.2 * (1 - s)).backward()
    return l1.detach(), s.detach(), p.grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w", SIZES)
def test_masked_forward_backward(h, w, kind):
    from sgn_rast import loss
    pred, gt = _images(h, w, h * 1000 + w, noise=0.3)
    assert float((pred > 1).float().mean()) > 0.02          # the clamp is exercised (test_fused_clamp_equals_...)
    m = _mask(kind, h, w)
    l1_ref, s_ref, g_ref = _reference(pred, gt, m)
    p_hip = pred.cuda().requires_grad_(True)
    l1, s = loss.l1_ssim(p_hip, gt.cuda(), clamp_max=1.0, mask=m.cuda())
    (0.8 * l1 + 0.2 * (1 - s)).backward()
    l1, s, grad = l1.detach(), s.detach(), p_hip.grad.cpu()
    e_l1, e_s, e_g = abs(float(l1) - float(l1_ref)), abs(float(s) - float(s_ref)), rel_l2(grad, g_ref)
    print(f"[masked loss] {h}x{w} {kind}: kept {float(m.float().mean()):.4f}  Ll1 {float(l1):.8f} (err {e_l1:.2e})  "
          f"ssim {float(s):.8f} (err {e_s:.2e})  grad rel-L2 {e_g:.2e}")
    assert e_l1 < 1e-6 * max(1.0, abs(float(l1_ref)))
    assert e_s < 2e-6
    assert e_g < 2e-5
    assert float(grad[~m].abs().max()) == 0.0               # an exact zero, L1 sign term included
    assert float(grad[pred > 1].abs().max()) == 0.0


@pytest.mark.parametrize("h,w", [(37, 53), (200, 333)])
def test_all_ones_mask_is_the_unmasked_call_bit_for_bit(h, w):
    from sgn_rast import loss
    pred, gt = _images(h, w, 3 * h + w, noise=0.3)
    ones = torch.ones(h, w, dtype=torch.bool, device="cuda")
    res = []
    for mask in (None, ones):
        p = pred.cuda().requires_grad_(True)
        l1, s = loss.l1_ssim(p, gt.cuda(), clamp_max=1.0, mask=mask)
        (0.8 * l1 + 0.2 * (1 - s)).backward()
        q = pred.cuda().requires_grad_(True)
        ph = loss.photometric_loss(q, gt.cuda(), 0.2, clamp_max=1.0, mask=mask)
        ph.backward()
        res.append((l1.detach(), s.detach(), p.grad, ph.detach(), q.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("h,w", [(16, 16), (128, 96)])
def test_all_zeros_mask(h, w):
    from sgn_rast import loss
    pred, gt = _images(h, w, 7 * h + w, noise=0.3)
    zeros = torch.zeros(h, w, dtype=torch.bool, device="cuda")
    p = pred.cuda().requires_grad_(True)
    l1, s = loss.l1_ssim(p, gt.cuda(), clamp_max=1.0, mask=zeros)
    (0.8 * l1 + 0.2 * (1 - s)).backward()
    l1, s = l1.detach(), s.detach()
    assert float(l1) == 0.0
    assert abs(float(s) - 1.0) < 2e-6
    assert float(p.grad.abs().max()) == 0.0
    psnr, ssim = loss.image_metrics(pred.cuda(), gt.cuda(), mask=zeros)
    assert float(psnr) == math.inf and abs(float(ssim) - 1.0) < 2e-6
    same = gt.cuda()
    assert float(loss.image_metrics(same, same.clone())[0]) == math.inf       # identical images, no mask


def test_mask_dtypes_shapes_and_inputs_left_alone():
    from sgn_rast import loss
    h, w = 61, 47
    pred, gt = _images(h, w, 11, noise=0.3)
    m = _mask("bernoulli", h, w).cuda()
    wide = torch.zeros(h, 2 * w, dtype=torch.bool, device="cuda")
    wide[:, ::2] = m
    strided = wide[:, ::2]
    assert not strided.is_contiguous() and torch.equal(strided, m)
    forms = [m, m.to(torch.uint8), m[..., None], m[..., None].to(torch.uint8), m.to(torch.uint8) * 255, strided,
             m.t().contiguous().t()]
    res = []
    for mask in forms:
        p, g = pred.cuda().requires_grad_(True), gt.cuda()
        p0, g0, mask0 = p.detach().clone(), g.clone(), mask.clone()
        l1, s = loss.l1_ssim(p, g, clamp_max=1.0, mask=mask)
        (0.8 * l1 + 0.2 * (1 - s)).backward()
        assert torch.equal(p.detach(), p0) and torch.equal(g, g0) and torch.equal(mask, mask0)   # nothing in place
        assert p.grad.shape == p.shape
        res.append((l1.detach(), s.detach(), p.grad))
    for r in res[1:]:
        for a, b in zip(res[0], r):
            assert torch.equal(a, b)
    assert float(res[0][2][~m].abs().max()) == 0.0
    with pytest.raises(TypeError):
        loss.l1_ssim(pred.cuda(), gt.cuda(), mask=m.float())
    with pytest.raises(ValueError):
        loss.photometric_loss(pred.cuda(), gt.cuda(), mask=m[:-1])


@pytest.mark.parametrize("kind", [None, "bernoulli", "hood"])
@pytest.mark.parametrize("h,w", [(37, 53), (200, 333), (1280, 1920)])
def test_image_metrics(h, w, kind):
    from sgn_rast import loss
    pred, gt = _images(h, w, 5 * h + w)
    m = torch.ones(h, w, dtype=torch.bool) if kind is None else _mask(kind, h, w)
    mf = m[..., None].float()
    mse_ref = float(((gt * mf - pred * mf).double() ** 2).mean())
    psnr_ref = 10.0 * math.log10(1.0 / mse_ref)
    s_ref = float(O.l1_ssim_losses(pred * mf, gt * mf)[1])
    p = pred.cuda().requires_grad_(True)                     # a graph-carrying input must not leak into the metrics
    mask = None if kind is None else m.cuda()
    psnr, ssim = loss.image_metrics(p, gt.cuda(), mask=mask)
    mse = loss._metrics_out4(p, gt.cuda(), mask)[3]
    for t in (psnr, ssim, mse):
        assert t.is_cuda and t.dim() == 0 and not t.requires_grad and t.grad_fn is None
    e_mse, e_psnr, e_s = abs(float(mse) - mse_ref) / mse_ref, abs(float(psnr) - psnr_ref), abs(float(ssim) - s_ref)
    print(f"[image metrics] {h}x{w} {kind}: mse {float(mse):.9e} (rel err {e_mse:.2e})  psnr {float(psnr):.6f} dB "
          f"(err {e_psnr:.2e})  ssim {float(ssim):.8f} (err {e_s:.2e})")
    assert e_mse < 1e-6
    assert e_psnr < 1e-5
    assert e_s < 2e-6


# ------------------------------------------------------------------------------------------------------ in the step
def _oracle_photometric(rgb, gt, lam, mask=None):
    """The reference's masked loss on the oracle: the `loss_fn` of step.train_step (rgb arrives clamped, :969)."""
    mf = 1.0 if mask is None else mask.reshape(rgb.shape[0], rgb.shape[1], 1).float()
    l1, s = O.l1_ssim_losses(rgb * mf, gt * mf)
    return (1 - lam) * l1 + lam * (1 - s)


@pytest.mark.parametrize("fused", [False, True])
def test_masked_loss_in_train_step(fused):
    """step.train_step(gt=, mask=) on the HIP path against the oracle rasterizer + oracle loss on the masked images."""
    import oracle_ops
    from sgn_rast import scenes, step
    cam, raw = scenes.make_scene("c1", seed=2, n_override=1500)
    gt = torch.rand(cam.height, cam.width, 3, generator=torch.Generator().manual_seed(4))
    m = _mask("hood", cam.height, cam.width) & _mask("bernoulli", cam.height, cam.width, seed=9)
    w_img, w_a = step.loss_weights(cam, seed=7)
    Pc = step.leaf_params(raw)
    exp = step.train_step(Pc, cam, w_img, w_a, ops=oracle_ops, gt=gt, mask=m, loss_fn=_oracle_photometric)
    cam_d, _ = scenes.make_scene("c1", seed=2, n_override=1500, device="cuda")
    Pd = step.leaf_params({k: v.cuda() for k, v in raw.items()})
    got = step.train_step(Pd, cam_d, w_img.cuda(), w_a.cuda(), gt=gt.cuda(), mask=m.cuda(), fused=fused)
    e_loss = abs(float(got.loss) - float(exp.loss))
    rels = {k: rel_l2(Pd[k].grad.cpu(), Pc[k].grad) for k in Pd}
    print(f"[masked step] fused={fused}: loss {float(got.loss):.8f} (err {e_loss:.2e})  "
          + "  ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    assert e_loss < 1e-5
    for k, v in rels.items():
        assert v < 5e-4, k


def test_masked_loss_in_train_step_views():
    """Two views, the second without a mask: gradients of the batched step against the two single-view masked fused
    steps averaged."""
    from sgn_rast import loss, scenes, step, views
    cam0, raw = scenes.make_scene("c1", seed=2, n_override=1500, device="cuda")
    cam1, _ = scenes.make_scene("c1", seed=2, yaw=0.15, n_override=1500, device="cuda")
    cams = [cam0, cam1]
    g = torch.Generator().manual_seed(4)
    gts = [torch.rand(cam0.height, cam0.width, 3, generator=g).cuda() for _ in cams]
    masks = [_mask("hood", cam0.height, cam0.width).cuda(), None]
    Pb = step.leaf_params(raw)
    out = views.train_step_views(Pb, cams, gts, masks=masks)
    acc = {k: torch.zeros_like(v) for k, v in raw.items()}
    total = 0.0
    for v, cam in enumerate(cams):
        P = step.leaf_params(raw)
        o = step.render_fused(P, cam)
        val = loss.photometric_loss(o.rgb, gts[v], 0.2, clamp_max=1.0, mask=masks[v]) / len(cams)
        val.backward()
        total += float(val)
        for k in acc:
            acc[k] += P[k].grad
    rels = {k: rel_l2(Pb[k].grad, acc[k]) for k in acc}
    print(f"[masked views] loss {float(out.loss):.8f} vs {total:.8f}  " + "  ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    # view for view the batched forward is the single-view one bit for bit: only the order of the two-term sum differs
    assert abs(float(out.loss) - total) < 1e-6
    for k, v in rels.items():
        assert v <= 1e-5, k
    # the mask reached view 0: without it the gradients differ
    Pn = step.leaf_params(raw)
    views.train_step_views(Pn, cams, gts)
    assert rel_l2(Pn["features_dc"].grad, Pb["features_dc"].grad) > 1e-3

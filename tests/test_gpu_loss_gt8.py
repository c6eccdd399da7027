"""uint8 ground truth in the fused L1 + SSIM loss (csrc/loss.hip byte instantiations via sgn_l1_ssim_gt8_fwd/bwd).

The reference is always the existing float path on ``gt8.cpu().float() / 255.0`` — the quotient formed ON THE CPU (a true
division; torch on the device multiplies by a reciprocal) and then moved to the device: the value the reference caches
(sgn_dataset.py:77) and get_gt_img forms.  The byte path must give the same bits, value for value, so every comparison
of the loss functions here is ``torch.equal``.  The ground truth holds every byte value 0..255 (the first 256 elements
are arange(256)): a dequantisation by u * (1 / 255) is off in the last bit for 126 of them and cannot pass."""
import ctypes

import pytest
import torch

from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

SIZES = [(11, 11), (16, 16), (37, 53), (200, 333), (1280, 1920)]     # smallest legal; one tile; 159-byte rows, partial
KINDS = [None, "bernoulli", "hood"]                                  # edge tiles; several tiles; 64-bit indexing


def _mask(kind, h, w, seed=1):
    """tests/test_gpu_masked_loss.py::_mask, bool [H,W], True = keep."""
    if kind == "bernoulli":
        return torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) < 0.7
    m = torch.ones(h, w, dtype=torch.bool)
    m[h - h // 3:, :] = False
    m[h // 5: h // 5 + max(1, h // 4), w // 3: w // 3 + max(1, w // 4)] = False
    return m


_CASES: dict = {}


def _case(h, w):
    """(pred, gt8, gt float) on the device, made once per size and never written to."""
    if (h, w) not in _CASES:
        g = torch.Generator().manual_seed(h * 1000 + w)
        gt8 = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g)
        gt8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
        gtf = gt8.float() / 255.0                                     # on the CPU: the correctly rounded quotient
        pred = (gtf + 0.3 * torch.randn(h, w, 3, generator=g)).clamp(0, 1.2)
        assert float((pred > 1).float().mean()) > 0.02               # clamp_max=1.0 is exercised
        assert len(torch.unique(gt8)) == 256
        _CASES[(h, w)] = (pred.cuda(), gt8.cuda(), gtf.cuda())
    return _CASES[(h, w)]


def _run(pred, gt, mask):
    from sgn_rast import loss
    p = pred.clone().requires_grad_(True)
    l1, s = loss.l1_ssim(p, gt, clamp_max=1.0, mask=mask)
    (0.8 * l1 + 0.2 * (1 - s)).backward()
    q = pred.clone().requires_grad_(True)
    ph = loss.photometric_loss(q, gt, 0.2, clamp_max=1.0, mask=mask)
    ph.backward()
    psnr, ssim = loss.image_metrics(pred, gt, mask=mask)
    mse = loss._metrics_out4(pred, gt, mask)[3]
    return dict(Ll1=l1.detach(), ssim=s.detach(), v_pred=p.grad, photometric=ph.detach(), v_pred_photometric=q.grad,
                psnr=psnr, metric_ssim=ssim, mse=mse)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w", SIZES)
def test_bytes_equal_the_cpu_quotient_bit_for_bit(h, w, kind):
    pred, gt8, gtf = _case(h, w)
    mask = None if kind is None else _mask(kind, h, w).cuda()
    ref, got = _run(pred, gtf, mask), _run(pred, gt8, mask)
    print(f"[gt8 loss] {h}x{w} {kind}: Ll1 {float(got['Ll1']):.8f} / {float(ref['Ll1']):.8f}  ssim "
          f"{float(got['ssim']):.8f} / {float(ref['ssim']):.8f}  psnr {float(got['psnr']):.5f} / {float(ref['psnr']):.5f}  "
          f"max |v_pred diff| {float((got['v_pred'] - ref['v_pred']).abs().max()):.1e}")
    assert float(ref["Ll1"]) < 0.5                                  # (read as 0..255, Ll1 would be ~127)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert torch.equal(got[k], ref[k]), k
    assert float(got["v_pred"].abs().max()) > 0.0
    if mask is not None:
        assert float(got["v_pred"][~mask].abs().max()) == 0.0


def test_the_byte_tensor_is_what_the_backward_keeps():
    """A quarter of the saved memory: the node holds the uint8 tensor itself, and neither input is modified."""
    from sgn_rast import loss
    pred, gt8, _ = _case(37, 53)
    p, g0 = pred.clone().requires_grad_(True), gt8.clone()
    out = loss.photometric_loss(p, g0, 0.2, clamp_max=1.0)
    saved = [t for t in out.grad_fn.saved_tensors if t is not None]
    assert any(t.dtype == torch.uint8 and t.data_ptr() == g0.data_ptr() for t in saved)
    assert not any(t.dtype == torch.float32 and t.shape == g0.shape and t.data_ptr() != p.data_ptr() for t in saved)
    out.backward()
    assert torch.equal(g0, gt8) and torch.equal(p.detach(), pred)


def test_a_strided_byte_gt():
    from sgn_rast import loss
    pred, gt8, _ = _case(37, 53)
    wide = torch.zeros(37, 53, 4, dtype=torch.uint8, device="cuda")
    wide[..., :3] = gt8
    view = wide[..., :3]
    assert not view.is_contiguous()
    a, b = loss.photometric_loss(pred, view, 0.2, clamp_max=1.0), loss.photometric_loss(pred, gt8, 0.2, clamp_max=1.0)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ dtypes
def test_integer_pred_is_a_type_error():
    from sgn_rast import loss
    pred, gt8, gtf = _case(16, 16)
    for bad in (gt8, (pred * 255).to(torch.int32)):
        for gt in (gt8, gtf):
            with pytest.raises(TypeError):
                loss.l1_ssim(bad, gt)
            with pytest.raises(TypeError):
                loss.photometric_loss(bad, gt, 0.2, clamp_max=1.0)
            with pytest.raises(TypeError):
                loss.image_metrics(bad, gt)


def test_float_gt_keeps_its_bits():
    """A float ground truth still goes to the unmasked entry: the public call equals a direct call of sgn_l1_ssim_fwd
    (whose kernels compile to the code they had), and a float64 one is still converted with .float()."""
    from sgn_rast import _lib as L
    from sgn_rast import loss
    h, w = 37, 53
    pred, _, gtf = _case(h, w)
    lib = L.load()
    out3 = torch.empty(3, dtype=torch.float32, device="cuda")
    ws = L.workspace(lib.sgn_l1_ssim_workspace_bytes(h, w, 0), pred.device)
    L.check(lib.sgn_l1_ssim_fwd(h, w, L.ptr(pred), L.ptr(gtf), 1.0, 1.0, 0.2, L.ptr(out3), 0, L.ptr(ws), ws.numel(),
                                L.stream_ptr()), "sgn_l1_ssim_fwd")
    l1, s = loss.l1_ssim(pred, gtf, clamp_max=1.0)
    ph = loss.photometric_loss(pred, gtf, 0.2, clamp_max=1.0)
    assert torch.equal(l1, out3[0]) and torch.equal(s, out3[1]) and torch.equal(ph, out3[2])
    l1d, sd = loss.l1_ssim(pred, gtf.double(), clamp_max=1.0)
    assert torch.equal(l1d, l1) and torch.equal(sd, s)
    half = gtf.half()
    l1h, _ = loss.l1_ssim(pred, half, clamp_max=1.0)
    assert torch.equal(l1h, loss.l1_ssim(pred, half.float(), clamp_max=1.0)[0])


# ------------------------------------------------------------------------------------------------------ in the step
GRAD_REL_L2 = 5e-4      # tests/test_gpu_masked_loss.py::test_masked_loss_in_train_step, the same scene: the raster
                        # backward accumulates with float atomics, so two runs of one input differ by their order


def _gt_for(cam, seed):
    gt8 = torch.randint(0, 256, (cam.height, cam.width, 3), dtype=torch.uint8,
                        generator=torch.Generator().manual_seed(seed))
    gt8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    return gt8.cuda(), (gt8.float() / 255.0).cuda()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_train_step_takes_a_byte_gt(fused, masked):
    from sgn_rast import scenes, step
    cam, raw = scenes.make_scene("c1", seed=2, n_override=1500, device="cuda")
    gt8, gtf = _gt_for(cam, 4)
    m = (_mask("hood", cam.height, cam.width) & _mask("bernoulli", cam.height, cam.width, seed=9)).cuda() if masked else None
    w_img, w_a = step.loss_weights(cam, seed=7)
    w_img, w_a = w_img.cuda(), w_a.cuda()
    Pf, Pb = step.leaf_params(raw), step.leaf_params(raw)
    ref = step.train_step(Pf, cam, w_img, w_a, gt=gtf, mask=m, fused=fused)
    got = step.train_step(Pb, cam, w_img, w_a, gt=gt8, mask=m, fused=fused)
    rels = {k: rel_l2(Pb[k].grad, Pf[k].grad) for k in Pf}
    print(f"[gt8 step] fused={fused} masked={masked}: loss {float(got.loss):.8f} / {float(ref.loss):.8f}  "
          + "  ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    assert torch.equal(got.loss.detach(), ref.loss.detach())
    for k, v in rels.items():
        assert v < GRAD_REL_L2, k


def test_train_step_passes_the_tensor_to_a_loss_fn_as_given():
    from sgn_rast import loss, scenes, step
    cam, raw = scenes.make_scene("c1", seed=2, n_override=1500, device="cuda")
    gt8, _ = _gt_for(cam, 4)
    w_img, w_a = step.loss_weights(cam, seed=7)
    seen = []

    def loss_fn(rgb, gt, lam):
        seen.append(gt)
        return loss.photometric_loss(rgb, gt, lam)

    step.train_step(step.leaf_params(raw), cam, w_img.cuda(), w_a.cuda(), gt=gt8, loss_fn=loss_fn)
    assert len(seen) == 1 and seen[0] is gt8


def test_train_step_views_takes_byte_gts():
    """Two views, the first with a mask."""
    from sgn_rast import scenes, step, views
    cam0, raw = scenes.make_scene("c1", seed=2, n_override=1500, device="cuda")
    cam1, _ = scenes.make_scene("c1", seed=2, yaw=0.15, n_override=1500, device="cuda")
    cams = [cam0, cam1]
    pairs = [_gt_for(cam0, 4), _gt_for(cam1, 5)]
    masks = [_mask("hood", cam0.height, cam0.width).cuda(), None]
    Pf, Pb = step.leaf_params(raw), step.leaf_params(raw)
    ref = views.train_step_views(Pf, cams, [p[1] for p in pairs], masks=masks)
    got = views.train_step_views(Pb, cams, [p[0] for p in pairs], masks=masks)
    rels = {k: rel_l2(Pb[k].grad, Pf[k].grad) for k in Pf}
    print(f"[gt8 views] loss {float(got.loss):.8f} / {float(ref.loss):.8f}  "
          + "  ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    assert torch.equal(got.loss.detach(), ref.loss.detach())
    for k, v in rels.items():
        assert v < GRAD_REL_L2, k

"""GPU (-m gpu): the fused L1 + SSIM loss (csrc/loss.hip through sgn_rast.loss) pixel by pixel against fp64, on
street-like images: smooth content, a flat sky band, exact 0.0 and 1.0 blocks, exact ties, and a prediction within
eps in {0.15, 1e-2, 1e-3, 1e-4} of the ground truth (tests/loss_fp64.py; tests/test_loss_fp64.py shows on the CPU that
the content reaches its targets, that the fp64 reference agrees with a closed-form gradient and that the rule below
rejects wrong gradients).

In that regime sigma^2 = E[x^2] - mu^2 cancels, 1/B2 approaches 1/C2 ~ 1100 and the backward's three maps are each
thousands in size and cancel to a small gradient.  The fp32 oracle is itself 1e-4 .. 1e-3 from the truth there, so fp64
is the truth and the budget is the fp32 oracle's own error on the same input, times F (loss_fp64.F, at most 8):

  gradient of ssim alone   max |g_hip - g64| <= F max |g32 - g64|, over the interior and over the border band (within
                           10 of an edge, where fewer than 121 windows contribute) separately, each with its own max
  ssim                     |ssim_hip - ssim64| <= F mean |S32 - S64| (the oracle's per-pixel map error: cannot cancel)
  Ll1                      |Ll1_hip - Ll1_64| <= (log2(3HW) + 4) 2^-24 Ll1_64
  gradient of Ll1 alone    sign(pred - gt) / (3HW) to 1 ulp where non-zero; an exact 0.0 at ties, masked-out pixels and
                           values above clamp_max
  gradient of ssim         an exact 0.0 at masked-out pixels and values above clamp_max
  (each yardstick floored at 2^-24 of the quantity's scale)

Variants: unmasked; clamp_max = 1 (with a block of pred in 1.0 .. 1.2); the hood and bernoulli masks of
tests/test_gpu_masked_loss.py with the clamp, whose edges cross the sky band.  Shapes: one output pixel, one output
row, one column, exactly one 16x16 tile of valid region plus one pixel (26x27), one pixel into further tiles (27x43),
37x53, 64x80 and, at eps = 1e-2, 128x96.

MEASURED (MI355X, kernel error / fp32-oracle error, worst over the shapes):
                 eps 0.15   1e-2   1e-3   1e-4      (columns), worst over the eight shapes
  g_int   plain      2.44   2.27   1.81   1.20
          clamp      4.64   2.27   1.84   1.66
          hood       2.92   1.94   1.57   1.20
          bernoulli  1.48   1.44   1.38   3.04
  g_band  plain      3.40   1.99   3.11   2.78
          clamp      3.07   2.79   3.81   2.97
          hood       2.22   2.78   2.21   1.93
          bernoulli  1.69   1.74   1.52   1.50
  ssim    plain      1.09   1.00   1.41   2.35
          clamp      1.67   0.85   3.47   0.76
          hood       0.99   0.26   1.29   0.38
          bernoulli  0.31   0.47   0.53   0.83
  Ll1 (over its derived bound, not over the oracle): at most 0.146
  image_metrics at 64x80, eps 1e-3 / 1e-4: mse at most 0.08 of its bound, PSNR at most 0.73, ssim at most 0.36 x oracle
Worst per quantity: g_int 4.64 (37x53, eps 0.15, clamp), g_band 3.81 and ssim 3.47 (both 11x11, eps 1e-3, clamp).

F = 8.  Twice the worst ratio rounded up is 10, above the ceiling of 8 this budget may not exceed, so F stands at the
ceiling: the margin over the worst case is 1.7x, not 2x, and at every other case at least 2.1x (the kernels add in a
fixed order, so the ratios repeat run for run).  The 4.64 is a finding about the FORWARD: the kernel's three stored maps
pushed through an fp64 backward give 4.7 on that case, the same maps formed by fp32 torch expressions give 0.95, and an
fp32 torch restatement of the whole formulation reaches at most 2.0 in the interior (3.7 in the band) over all cases.
The backward filter and the border guards add nothing measurable.  DESIGN.md (loss section) has the breakdown; the
kernel is unchanged.
"""
import math

import pytest
import torch

import loss_fp64 as LF

pytestmark = pytest.mark.gpu

CASES = [(h, w, e, v) for (h, w, e) in LF.CASES for v in LF.VARIANTS]


@pytest.fixture(scope="module")
def loss():
    from sgn_rast import _lib, loss as M
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return M


def _run(loss, c):
    """(g_ssim, g_l1, ssim, Ll1) of the kernels on the case: one forward, each output backpropagated alone."""
    p = c.pred.cuda().requires_grad_(True)
    mask = None if c.mask is None else c.mask.cuda()
    l1, s = loss.l1_ssim(p, c.gt.cuda(), clamp_max=c.clamp_max, mask=mask)
    g_s, = torch.autograd.grad(s, p, retain_graph=True)
    g_l1, = torch.autograd.grad(l1, p)
    return g_s.cpu(), g_l1.cpu(), float(s.detach()), float(l1.detach())


@pytest.mark.parametrize("h,w,eps,variant", CASES, ids=[f"{h}x{w}-{e:g}-{v}" for h, w, e, v in CASES])
def test_loss_per_pixel(loss, h, w, eps, variant):
    c = LF.case(h, w, eps, variant)
    g_s, g_l1, s, l1 = _run(loss, c)
    r = LF.ratios(c, g_s, s, l1)
    print(f"\nLOSS_PER_PIXEL {h}x{w} eps {eps:g} {variant}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    LF.accept(c, g_s, g_l1, s, l1)


@pytest.mark.parametrize("kind", [None, "hood", "bernoulli"])
@pytest.mark.parametrize("eps", [1e-3, 1e-4])
def test_image_metrics_near_convergence(loss, eps, kind):
    """image_metrics at 60 .. 80 dB: mse within the summation bound of an fp32 sum of 3HW non-negative terms, PSNR
    within 10 / ln 10 times that relative bound, ssim by the yardstick above."""
    h, w = 64, 80
    c = LF.case(h, w, eps, "plain")
    m = None if kind is None else LF.mask_of(kind, h, w)
    r32, r64 = (LF.reference(c.pred, c.gt, m, None, dt) for dt in (torch.float32, torch.float64))
    mf = 1.0 if m is None else m[..., None].double()
    mse_ref = float((((c.gt.double() - c.pred.double()) * mf) ** 2).mean())
    psnr_ref = 10.0 * math.log10(1.0 / mse_ref)
    mask = None if m is None else m.cuda()
    psnr, ssim = loss.image_metrics(c.pred.cuda(), c.gt.cuda(), mask=mask)
    mse = float(loss._metrics_out4(c.pred.cuda(), c.gt.cuda(), mask)[3])
    bound = LF.sum_bound(3 * h * w)
    e_mse, e_psnr = abs(mse - mse_ref) / mse_ref, abs(float(psnr) - psnr_ref)
    s_yard = max(float((r32.S.double() - r64.S).abs().mean()), LF.U * abs(float(r64.ssim)))
    e_s = abs(float(ssim) - float(r64.ssim)) / s_yard
    print(f"\nLOSS_METRICS {h}x{w} eps {eps:g} {kind}: psnr {psnr_ref:.4f} dB  mse err/bound {e_mse / bound:.3g}  "
          f"psnr err/bound {e_psnr / (10 / math.log(10) * bound):.3g}  ssim {e_s:.3g}")
    assert 55.0 < psnr_ref < 85.0
    assert e_mse <= bound
    assert e_psnr <= 10.0 / math.log(10.0) * bound
    assert e_s <= LF.F

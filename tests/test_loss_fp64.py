"""CPU: the fp64 yardstick of the loss tests (tests/loss_fp64.py) is itself checked — the closed-form gradient against
fp64 autograd, the content against its targets, and the acceptance rule against three deliberately wrong gradients.
tests/test_gpu_loss_per_pixel.py applies the same rule to csrc/loss.hip."""
import pytest
import torch

import loss_fp64 as LF
from oracle import torch_oracle as O

ALL_SHAPES = LF.SHAPES + [LF.BIG]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("variant", LF.VARIANTS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids)
def test_analytic_gradient_equals_fp64_autograd(shape, variant):
    h, w = shape
    for eps in ((1e-2,) if shape == LF.BIG else (0.15, 1e-4)):
        c = LF.case(h, w, eps, variant)
        got = LF.analytic_ssim_grad(c.pred, c.gt, c.mask, c.clamp_max)
        want = c.r64.g_ssim
        scale = float(want.abs().max())
        assert scale > 0
        band = LF.band_mask(h, w)
        e_band = float((got - want)[band].abs().max())
        assert e_band <= 1e-10 * scale, (eps, "band", e_band / scale)
        if bool((~band).any()):
            e_int = float((got - want)[~band].abs().max())
            assert e_int <= 1e-10 * scale, (eps, "interior", e_int / scale)
        z = LF.zero_pixels(c)
        if bool(z.any()):
            assert float(got[z].abs().max()) == 0.0 and float(want[z].abs().max()) == 0.0


def test_reference_at_fp32_is_the_oracle_bit_for_bit():
    """`reference(dtype=float32)` is what the budget calls "the fp32 oracle": the same numbers as
    oracle/torch_oracle.py:l1_ssim_losses with autograd."""
    c = LF.case(37, 53, 1e-3, "plain")
    p = c.pred.clone().requires_grad_(True)
    l1, s = O.l1_ssim_losses(p, c.gt)
    g, = torch.autograd.grad(s, p)
    assert torch.equal(l1.detach(), c.r32.Ll1) and torch.equal(s.detach(), c.r32.ssim) and torch.equal(g, c.r32.g_ssim)
    assert torch.equal(LF.window(torch.float32), O.ssim_window())


def test_masks_are_the_masked_loss_tests_masks():
    from tests.test_gpu_masked_loss import _mask
    for h, w in ALL_SHAPES:
        for kind in ("hood", "bernoulli"):
            assert torch.equal(LF.mask_of(kind, h, w), _mask(kind, h, w))


@pytest.mark.parametrize("h,w,eps", LF.CASES, ids=[f"{h}x{w}-{e:g}" for h, w, e in LF.CASES])
def test_street_pair_reaches_its_targets(h, w, eps):
    L = LF.layout(h, w)
    plain, clamp = LF.case(h, w, eps, "plain"), LF.case(h, w, eps, "clamp")
    pred, gt = plain.pred, plain.gt
    assert pred.dtype == torch.float32 and pred.shape == (h, w, 3) and float(pred.min()) >= 0.0
    # the tie block is bit-equal, and it is not the only place the images agree or differ
    r0, r1, c0, c1 = L.tie
    assert r1 > r0 and c1 > c0 and torch.equal(pred[r0:r1, c0:c1], gt[r0:r1, c0:c1])
    assert not torch.equal(pred, gt)
    # exact 0.0 and exact 1.0 blocks, no edge on a 16-pixel tile boundary
    for (r0, r1, c0, c1), value in ((L.black, 0.0), (L.white, 1.0)):
        assert r1 > r0 and c1 > c0 and bool((gt[r0:r1, c0:c1] == value).all())
        assert all(v % 16 for v in (r0, r1, c0, c1)), (r0, r1, c0, c1)
    assert all(v % 16 for v in L.tie)
    # sky: rows [0, h // 4) are the constant; windows that straddle its lower edge exist (top row flat, window textured)
    assert L.hs >= 1 and bool((gt[:L.hs] == torch.tensor([0.55, 0.7, 0.9])).all())
    x, y = pred.double().permute(2, 0, 1)[None], gt.double().permute(2, 0, 1)[None]
    win = LF.window(torch.float64)
    filt = lambda t: torch.nn.functional.conv2d(
        torch.nn.functional.conv2d(t, win.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3),
        win.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)
    var1 = (filt(x * x) - filt(x) ** 2)[0]
    var2 = (filt(y * y) - filt(y) ** 2)[0]
    straddle = var2[:, :L.hs]                                  # output rows < hs start in the sky, all reach below it
    assert straddle.numel() > 0 and float(straddle.max()) > 1e-4
    # flat windows: an image needs 11 flat rows and columns in BOTH images; with a dimension of 11 every window holds
    # the whole height or width (sky, texture and blocks at once), so no window can be flat there
    flat = int(((var1 + var2) < 1e-6).sum())
    if min(h, w) >= 26:
        assert flat > 0
    # the clamp cases: at least 2 % of the values above 1
    assert float((clamp.pred > 1).float().mean()) >= 0.02
    assert bool((clamp.pred == 1.0).any())
    # the fp32 oracle's own error, per quantity: finite and non-zero
    for c in (plain, clamp, LF.case(h, w, eps, "hood"), LF.case(h, w, eps, "bernoulli")):
        e_S = float((c.r32.S.double() - c.r64.S).abs().max())
        e_s = abs(float(c.r32.ssim) - float(c.r64.ssim))
        e_g = float((c.r32.g_ssim.double() - c.r64.g_ssim).abs().max()) / float(c.r64.g_ssim.abs().max())
        print(f"[oracle32 vs fp64] {h}x{w} eps {eps:g} {c.variant}: |ssim32-ssim64| {e_s:.2e}  max|S32-S64| {e_S:.2e}  "
              f"grad max|g32-g64|/max|g64| {e_g:.2e}  flat windows {flat}")
        for v in (e_S, e_g):
            assert v > 0 and v == v and v != float("inf")


def test_hood_edges_cross_the_sky_band():
    for h, w in ALL_SHAPES:
        m, hs = LF.mask_of("hood", h, w), h // 4
        cols = slice(w // 3, w // 3 + max(1, w // 4))
        if h >= 26:                                            # (at h = 11 the band is two rows and h // 5 == h // 4)
            assert not bool(m[hs - 1, cols].any()) and not bool(m[hs, cols].any())      # masked on both sides of the edge
            assert bool(m[:hs].any()) and not bool(m[:hs].all())                        # the band is kept in part


@pytest.mark.parametrize("eps", LF.EPS)
@pytest.mark.parametrize("shape", [(37, 53), (64, 80)], ids=_ids)
def test_acceptance_rejects_wrong_gradients(shape, eps):
    """The budget is sharp: the fp32 oracle passes its own rule, and three fp32 gradients that are wrong in the ways a
    kernel goes wrong are each rejected, at every eps.  No faulty GPU code is run."""
    h, w = shape
    c = LF.case(h, w, eps, "plain")
    ok = c.r32
    LF.accept(c, ok.g_ssim, ok.g_l1, ok.ssim, ok.Ll1)                      # the oracle itself: ratio 1 by construction
    # 1. C2 = 1e-3 instead of 9e-4
    bad = LF.reference(c.pred, c.gt, dtype=torch.float32, C2=1e-3)
    with pytest.raises(AssertionError, match="oracle's"):
        LF.accept(c, bad.g_ssim, ok.g_l1, ok.ssim, ok.Ll1)
    # 2. the valid-region guard off by one: the last output row contributes nothing (to image rows h - 11 .. h - 1:
    # one interior row and the bottom band)
    bad = LF.reference(c.pred, c.gt, dtype=torch.float32, drop_last_row=True)
    with pytest.raises(AssertionError, match="g_(int|band)"):
        LF.accept(c, bad.g_ssim, ok.g_l1, ok.ssim, ok.Ll1)
    # 3. sign(0) = +1 at ties
    ties = c.pred == c.gt
    assert bool(ties.any())
    g_l1 = torch.where(ties, torch.full_like(ok.g_l1, 1.0 / (3 * h * w)), ok.g_l1)
    with pytest.raises(AssertionError, match="ties"):
        LF.accept(c, ok.g_ssim, g_l1, ok.ssim, ok.Ll1)

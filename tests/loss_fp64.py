"""Street-like image pairs, an fp64 reference of the L1 + SSIM loss and the per-pixel acceptance rule built on it.
Plain torch on the CPU; nothing here touches the GPU (tests/test_loss_fp64.py runs all of it without one).

Why: the other loss tests feed white noise, where every 11x11 window has sigma^2 ~ 0.08 >> C2 = 9e-4 and
sigma^2 = E[x^2] - mu^2 never cancels.  Training images have a flat sky, a dark road, saturated highlights and, late in
the fit, a prediction within 1e-2 .. 1e-4 of the ground truth.  There the fp32 oracle is itself 2e-4 .. 1e-3 from the
truth per pixel, so the yardstick has to be fp64 and the budget has to be the fp32 oracle's own error on the same input.

* street_pair      the content (layout below)
* reference        the reference's literal expressions at a dtype: Ll1, ssim, the per-pixel map, the two gradients
* analytic_ssim_grad   closed-form fp64 gradient of ssim, a direct sum over the windows that contain a pixel (unfold /
                   fold, centred moments): the fp64 reference does not rest on conv2d autograd alone
* case             one cached (content, fp32 reference, fp64 reference) per (h, w, eps, variant), shared by all tests
* ratios / accept  kernel error over oracle32 error per quantity, and the asserts on them

Layout of street_pair (hs = h // 4; "big" = the dimension is >= 26, otherwise blocks shrink to a third of it):
  rows [0, hs)                         sky: the constant (0.55, 0.7, 0.9)
  rows [hs+2, hs+2+bh) x cols [1, 1+bw)    exact 0.0 (bh, bw = 13 when big); pred there is max(0, eps randn): half ties
  rows [hs+3, hs+3+wh) x cols [w-2-ww, w-2) exact 1.0 (5 x 7 when big)
  rows [max(hs-3,1), hs+1+bh) x cols [2, 1+bw)  pred = gt bit for bit: sky ties, two textured rows, and a 12x12 area of
                                       pred = gt = 0 inside the black block, i.e. 2x2 windows that are exactly flat
  rows [h-2-h//5, h-2) x cols [w//3, w//3 + w//3)  (clamp cases) pred = 1.0 .. 1.2, first row exactly 1.0
None of the block edges is a multiple of 16 at the shapes in SHAPES (test_loss_fp64.py asserts it).
"""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as Fn

U = 2.0 ** -24
WIN, HALO = 11, 10
EPS = (0.15, 1e-2, 1e-3, 1e-4)
SHAPES = [(11, 11), (11, 64), (64, 11), (26, 27), (27, 43), (37, 53), (64, 80)]
BIG = (128, 96)                                   # at eps = 1e-2 only
VARIANTS = ("plain", "clamp", "hood", "bernoulli")
CASES = [(h, w, e) for (h, w) in SHAPES for e in EPS] + [(BIG[0], BIG[1], 1e-2)]

# The kernel may be F times the fp32 oracle's own error against fp64 (gradient per pixel, SSIM value).  The rule is twice
# the worst ratio measured on the MI355X, rounded up, and never more than 8.  The worst measured ratio is 4.64, so the
# rule asks for 10 and F stands at its ceiling (tests/test_gpu_loss_per_pixel.py and DESIGN.md have every ratio).
F = 8


def _span(n, big, small_div=3):
    return big if n >= 26 else max(2, n // small_div)


def layout(h, w):
    """The blocks of street_pair as (r0, r1, c0, c1), clipped to the image."""
    hs = h // 4
    bh, bw = _span(h, 13), _span(w, 13)
    wh, ww = _span(h, 5, 5), _span(w, 7, 4)
    clip = lambda r0, r1, c0, c1: (max(r0, 0), min(r1, h), max(c0, 0), min(c1, w))
    return SimpleNamespace(
        hs=hs,
        black=clip(hs + 2, hs + 2 + bh, 1, 1 + bw),
        white=clip(hs + 3, hs + 3 + wh, w - 2 - ww, w - 2),
        tie=clip(max(hs - 3, 1), hs + 1 + bh, 2, 1 + bw),
        hot=clip(h - 2 - max(1, h // 5), h - 2, w // 3, w // 3 + max(1, w // 3)))


def street_pair(h, w, eps, seed, clamp=False):
    """(pred, gt) fp32 [H,W,3]; see the module docstring.  clamp: add the block of pred in 1.0 .. 1.2."""
    g = torch.Generator().manual_seed(seed)
    L = layout(h, w)
    grid = torch.rand(1, 3, h // 8 + 2, w // 8 + 2, generator=g)
    gt = Fn.interpolate(grid, size=(h, w), mode="bicubic", align_corners=False)[0].permute(1, 2, 0).clamp(0, 1)
    gt = gt.contiguous()
    gt[:L.hs] = torch.tensor([0.55, 0.7, 0.9])
    r0, r1, c0, c1 = L.black
    gt[r0:r1, c0:c1] = 0.0
    r0, r1, c0, c1 = L.white
    gt[r0:r1, c0:c1] = 1.0
    pred = (gt + eps * torch.randn(h, w, 3, generator=g)).clamp(min=0.0)
    r0, r1, c0, c1 = L.tie
    pred[r0:r1, c0:c1] = gt[r0:r1, c0:c1]
    if clamp:
        r0, r1, c0, c1 = L.hot
        pred[r0:r1, c0:c1] = 1.0 + 0.2 * torch.rand(r1 - r0, c1 - c0, 3, generator=g)
        pred[r0, c0:c1] = 1.0                     # exactly at the clamp: the gradient passes
    return pred, gt


def mask_of(kind, h, w, seed=1):
    """tests/test_gpu_masked_loss.py::_mask, restated (test_loss_fp64.py holds the two equal).  bool [H,W], True = keep.
    hood's rectangle starts at row h // 5 < h // 4 and is h // 4 tall, so it crosses the lower edge of the sky band;
    bernoulli's edges are everywhere."""
    if kind == "bernoulli":
        return torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) < 0.7
    assert kind == "hood"
    m = torch.ones(h, w, dtype=torch.bool)
    m[h - h // 3:, :] = False
    m[h // 5: h // 5 + max(1, h // 4), w // 3: w // 3 + max(1, w // 4)] = False
    return m


def window(dtype):
    """The 11 taps: built in fp32 (pytorch_msssim._fspecial_gauss_1d, csrc/loss.hip:make_window), then cast, so that the
    fp64 side filters with the same 11 numbers as the kernel."""
    coords = torch.arange(WIN, dtype=torch.float32) - WIN // 2
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def _inputs(p, gt, mask, clamp_max, dtype):
    y = gt.to(dtype)
    x = p if clamp_max is None else torch.clamp(p, max=clamp_max)
    if mask is not None:
        mf = mask.reshape(mask.shape[0], mask.shape[1], 1).to(dtype)
        x, y = x * mf, y * mf
    return x, y


def ssim_map(X, Y, dtype, C2=0.03 ** 2, C1=0.01 ** 2):
    """pytorch_msssim's expressions (oracle/torch_oracle.py:ssim) on [1,3,H,W] -> the map [1,3,H-10,W-10]."""
    win = window(dtype)

    def filt(t):
        t = Fn.conv2d(t, win.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3)
        return Fn.conv2d(t, win.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)

    mu1, mu2 = filt(X), filt(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq = filt(X * X) - mu1_sq
    sigma2_sq = filt(Y * Y) - mu2_sq
    sigma12 = filt(X * Y) - mu1_mu2
    cs_map = (2 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2)
    return ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map


def reference(pred, gt, mask=None, clamp_max=None, dtype=torch.float64, C2=0.03 ** 2, drop_last_row=False):
    """The reference's literal expressions (sgn_splatfacto.py:1081-1087: clamp, mask, |gt - rgb|.mean(), SSIM(gt, rgb)) at
    `dtype`.  Returns Ll1, ssim, S (the per-pixel map [3,Ho,Wo]) and g_l1 / g_ssim, the gradients of each term alone with
    respect to pred, by autograd.  `C2` and `drop_last_row` exist only to build deliberately wrong gradients."""
    p = pred.to(dtype).clone().requires_grad_(True)
    x, y = _inputs(p, gt, mask, clamp_max, dtype)
    Ll1 = torch.abs(y - x).mean()
    S = ssim_map(y.permute(2, 0, 1)[None, ...], x.permute(2, 0, 1)[None, ...], dtype, C2=C2)
    if drop_last_row:
        ssim = torch.flatten(S[:, :, :-1, :], 2).sum(-1).div(S.shape[2] * S.shape[3]).mean()
    else:
        ssim = torch.flatten(S, 2).mean(-1).mean()
    g_l1, = torch.autograd.grad(Ll1, p, retain_graph=True)
    g_ssim, = torch.autograd.grad(ssim, p)
    return SimpleNamespace(Ll1=Ll1.detach(), ssim=ssim.detach(), S=S.detach()[0], g_l1=g_l1, g_ssim=g_ssim)


def analytic_ssim_grad(pred, gt, mask=None, clamp_max=None):
    """d ssim / d pred in fp64 without autograd and without conv2d: every window's 121 samples are laid out by unfold,
    the moments are direct weighted sums, and with the centred identities (exact for any weights)
        d sigma12 / d x_k = w_k (y_k - mu2),   d sigma1^2 / d x_k = 2 w_k (x_k - mu1),   d mu1 / d x_k = w_k
    the derivative of S = (A1 / B1)(A2 / B2) per window sample is
        w_k [ (2 mu2 / B1 - 2 mu1 A1 / B1^2) A2 / B2 + (A1 / B1)(2 (y_k - mu2) / B2 - 2 A2 (x_k - mu1) / B2^2) ].
    fold adds each sample's term back onto its pixel: at most 121 windows, fewer within 10 of an edge."""
    dt = torch.float64
    h, w = pred.shape[0], pred.shape[1]
    ho, wo = h - HALO, w - HALO
    p = pred.to(dt)
    x, y = _inputs(p, gt, mask, clamp_max, dt)
    g = window(dt)
    wk = torch.outer(g, g).reshape(1, WIN * WIN, 1)
    xs = Fn.unfold(x.permute(2, 0, 1)[:, None], WIN)           # [3, 121, Ho*Wo]
    ys = Fn.unfold(y.permute(2, 0, 1)[:, None], WIN)
    mu1, mu2 = (wk * xs).sum(1, keepdim=True), (wk * ys).sum(1, keepdim=True)
    dx, dy = xs - mu1, ys - mu2
    # the 11 fp32 taps sum to 1 only to ~1e-7, and the reference's sigma^2 = E[x^2] - mu^2 sees that: with W = sum w,
    # E[x^2] - mu^2 = sum w (x - mu)^2 + mu^2 (1 - W)
    rest = 1.0 - wk.sum()
    s1 = (wk * dx * dx).sum(1, keepdim=True) + mu1 * mu1 * rest
    s2 = (wk * dy * dy).sum(1, keepdim=True) + mu2 * mu2 * rest
    s12 = (wk * dx * dy).sum(1, keepdim=True) + mu1 * mu2 * rest
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    per = wk * ((2 * mu2 / B1 - 2 * mu1 * A1 / B1 ** 2) * (A2 / B2)
                + (A1 / B1) * (2 * dy / B2 - 2 * A2 * dx / B2 ** 2))
    grad = Fn.fold(per, (h, w), WIN)[:, 0].permute(1, 2, 0) / (3.0 * ho * wo)
    if clamp_max is not None:
        grad = grad * (p <= clamp_max).to(dt)
    if mask is not None:
        grad = grad * mask.reshape(h, w, 1).to(dt)
    return grad


def band_mask(h, w):
    """bool [H,W]: the pixels within 10 of any edge — those that fewer than 121 windows contain."""
    b = torch.ones(h, w, dtype=torch.bool)
    if h > 2 * HALO and w > 2 * HALO:
        b[HALO:h - HALO, HALO:w - HALO] = False
    return b


@functools.lru_cache(maxsize=None)
def case(h, w, eps, variant):
    """One cached case: content, mask, clamp, the fp32 oracle and the fp64 truth.  Nothing returned may be modified."""
    clamp = variant != "plain"                    # the masked calls clamp too, as the training step does
    pred, gt = street_pair(h, w, eps, h * 1000 + w, clamp=clamp)
    mask = mask_of(variant, h, w) if variant in ("hood", "bernoulli") else None
    cmax = 1.0 if clamp else None
    return SimpleNamespace(h=h, w=w, eps=eps, variant=variant, pred=pred, gt=gt, mask=mask, clamp_max=cmax,
                           r32=reference(pred, gt, mask, cmax, torch.float32),
                           r64=reference(pred, gt, mask, cmax, torch.float64))


def sum_bound(n):
    """Relative bound of an fp32 sum of n non-negative terms, tree or serial in blocks, plus the forming of each term
    and the final scale: (log2 n + 4) 2^-24."""
    return (math.log2(n) + 4.0) * U


def ratios(c, g_ssim, ssim, Ll1):
    """Kernel error over yardstick per quantity for the case `c`.  g_ssim fp32 [H,W,3]; ssim, Ll1 floats.
    g_int / g_band: max |g - g64| over the interior / the border band, over the fp32 oracle's max |g32 - g64| in the same
    region, floored at 2^-24 of max |g64| (an oracle that happens to be exact cannot divide by zero).
    ssim: |ssim - ssim64| over the oracle's mean absolute per-pixel map error (which cannot cancel), floored at 2^-24.
    Ll1: |Ll1 - Ll1_64| over the derived summation bound — that one must stay below 1, not F."""
    r32, r64 = c.r32, c.r64
    band = band_mask(c.h, c.w)
    g64 = r64.g_ssim
    floor = U * float(g64.abs().max())
    e_k = (g_ssim.double() - g64).abs()
    e_o = (r32.g_ssim.double() - g64).abs()
    out = {}
    for name, region in (("g_int", ~band), ("g_band", band)):
        if bool(region.any()):
            out[name] = float(e_k[region].max()) / max(float(e_o[region].max()), floor)
    s_yard = max(float((r32.S.double() - r64.S).abs().mean()), U * abs(float(r64.ssim)))
    out["ssim"] = abs(float(ssim) - float(r64.ssim)) / s_yard
    l1_64 = float(r64.Ll1)
    out["Ll1"] = abs(float(Ll1) - l1_64) / max(sum_bound(3 * c.h * c.w) * l1_64, 1e-300)
    return out


def zero_pixels(c):
    """bool [H,W,3]: where both gradients must be an exact 0.0 — masked-out pixels and values above clamp_max."""
    z = torch.zeros(c.h, c.w, 3, dtype=torch.bool)
    if c.clamp_max is not None:
        z |= c.pred > c.clamp_max
    if c.mask is not None:
        z |= ~c.mask.reshape(c.h, c.w, 1)
    return z


def check_l1_grad(c, g_l1):
    """The gradient of Ll1 alone: sign(x - y) / (3HW) to 1 ulp wherever that is non-zero, an exact 0.0 at every tie,
    every masked-out pixel and every pixel above clamp_max."""
    x, y = _inputs(c.pred, c.gt, c.mask, c.clamp_max, torch.float32)
    sgn = torch.sign(x - y)
    sgn[zero_pixels(c)] = 0.0
    want = sgn.double() / (3.0 * c.h * c.w)
    zero = sgn == 0
    nz_bad = int((g_l1[zero] != 0).sum())
    assert nz_bad == 0, f"{nz_bad} of {int(zero.sum())} ties / masked / clamped values have a non-zero L1 gradient"
    ulp = 2.0 ** (math.floor(math.log2(1.0 / (3.0 * c.h * c.w))) - 23)
    err = (g_l1.double() - want).abs()[~zero]
    assert err.numel() == 0 or float(err.max()) <= ulp, f"L1 gradient off by {float(err.max()):.3g} (ulp {ulp:.3g})"


def accept(c, g_ssim, g_l1, ssim, Ll1, factor=None):
    """The acceptance rule of tests/test_gpu_loss_per_pixel.py; returns the ratios.  Raises AssertionError."""
    factor = F if factor is None else factor
    r = ratios(c, g_ssim, ssim, Ll1)
    tag = f"{c.h}x{c.w} eps {c.eps:g} {c.variant}"
    assert all(math.isfinite(v) for v in r.values()), (tag, r)
    for k in ("g_int", "g_band", "ssim"):
        if k in r:
            assert r[k] <= factor, f"{tag}: {k} error is {r[k]:.3g} x the fp32 oracle's (budget {factor})"
    assert r["Ll1"] <= 1.0, f"{tag}: Ll1 error is {r['Ll1']:.3g} x the summation bound"
    z = zero_pixels(c)
    if bool(z.any()):
        assert float(g_ssim[z].abs().max()) == 0.0, f"{tag}: ssim gradient non-zero at a masked or clamped value"
    check_l1_grad(c, g_l1)
    return r

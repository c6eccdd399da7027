"""GPU (-m gpu): the feature rasterizer (`sgn_rast.features`, csrc/raster_features.hip) and the semantic cross-entropy
(csrc/semantic_loss.hip).

Forward: every channel BIT-EQUAL to the same channel of `ops.rasterize_gaussians` with D = K — the multi-pass
yardstick, ceil(K / 3) passes of the 3-channel kernels over one binning — and `1 - final_Ts` bit-equal to its alpha, with
the hardware exp and the portable one, a non-zero background, for every chunk layout (K = 1, 2, 4: exact widths; 5: a
padded chunk; 16: the widest; 17, 20, 33, 64: several walks, a narrow or padded last one), on partial tiles, on walks
that stop early, and on an empty list.
Backward: `v_xy`, `v_conic`, `v_features`, `v_opacity` against fp64 autograd through the channel-generic torch oracle
(tests/test_features_oracle.py pins it) and against the yardstick, rel-L2 <= 1e-4 (the project's gradient bar: fp32
atomics in arbitrary order and a 1-ulp exp / rcp against a double-accumulating reference).  The scenes' opacities stay
<= 0.98, so autograd's clamp and the kernels' `alpha_clamp_bwd` agree (tests/test_gpu_parity.py); where the clamp acts
the yardstick, which honours the same setting, is the reference.
Semantic cross-entropy: loss and gradient per element against the fp64 definition (tests/semantic_fp64.py) within 8x the
error of torch's own fp32 `F.cross_entropy` on the same input, each yardstick floored at 2^-24 of the quantity's scale
(the rule of tests/test_gpu_loss_per_pixel.py)."""
import pytest
import torch

import semantic_fp64 as SF
from helpers import rel_l2, small_scene
from sgn_rast import features as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_BAR = 1e-4

SCENES = {
    # name: (n, W, H, z_range)
    "base": (3000, 128, 128, (1.0, 5.0)),
    "edges": (3000, 200, 120, (1.0, 5.0)),          # partial tiles on the right and bottom edges
    "opaque": (3000, 128, 128, (1.0, 1.3)),         # near-opaque, close: every walk stops early
    "empty": (64, 128, 128, (1.0, 5.0)),            # everything behind the camera: nothing is listed
    "grad": (1500, 96, 80, (1.0, 5.0)),
}
_GEO = {}


def _geo(kind):
    """Projected geometry on the device, once per scene, left unchanged."""
    if kind not in _GEO:
        from sgn_rast import ops
        n, W, H, z = SCENES[kind]
        cam, P = small_scene(n=n, w=W, h=H, focal=float(W), z_range=z)
        if kind == "opaque":
            P["opacity_logits"].fill_(3.8)           # 0.978: three or four entries saturate a pixel
            P["log_scales"] += 1.0
        if kind == "empty":
            P["means"][:, 2] = -P["means"][:, 2]
        P = {k: v.to(DEV) for k, v in P.items()}
        with torch.no_grad():
            scales = P["log_scales"].exp()
            quats = P["quats"] / P["quats"].norm(dim=-1, keepdim=True)
            xys, depths, radii, conics, _c, nth, _cov = ops.project_gaussians(
                P["means"], scales, 1.0, quats, cam.viewmat.to(DEV), cam.fx, cam.fy, cam.cx, cam.cy, H, W, 16)
            opac = torch.sigmoid(P["opacity_logits"])
        _GEO[kind] = dict(geo=(xys, depths, radii, conics, nth), opac=opac, logits=P["opacity_logits"], H=H, W=W, n=n,
                          cam=cam, P=P)
    return _GEO[kind]


def _features(n, K, seed=0):
    g = torch.Generator().manual_seed(100 * K + seed)
    return torch.randn(n, K, generator=g), torch.rand(K, generator=g) + 0.1


def _check_forward(kind, K, exact):
    from sgn_rast import _lib as L, ops
    S = _geo(kind)
    feats, bg = _features(S["n"], K)
    feats, bg = feats.to(DEV), bg.to(DEV)
    with L.options(exact_exp=exact), torch.no_grad():
        out, alpha = F.rasterize_features(*S["geo"], feats, S["opac"], S["H"], S["W"], background=bg, return_alpha=True)
        ref, ref_alpha = ops.rasterize_gaussians(*S["geo"], feats, S["opac"], S["H"], S["W"], 16, bg, True)
    torch.cuda.synchronize()
    assert out.shape == (S["H"], S["W"], K) and alpha.shape == (S["H"], S["W"])
    assert torch.equal(alpha, ref_alpha), float((alpha - ref_alpha).abs().max())
    for c in range(K):
        assert torch.equal(out[..., c], ref[..., c]), (c, float((out[..., c] - ref[..., c]).abs().max()))
    return out, alpha, bg


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4, 5, 16, 17, 20, 33, 64])
def test_forward_equals_the_multi_pass_form_bit_for_bit(K, exact):
    out, alpha, _ = _check_forward("base", K, exact)
    assert float(alpha.max()) > 0.5 and float(out.abs().max()) > 0.5         # not a comparison of blank images


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("K", [5, 20])
@pytest.mark.parametrize("kind", ["edges", "opaque", "empty"])
def test_forward_scenes(kind, K, exact):
    out, alpha, bg = _check_forward(kind, K, exact)
    if kind == "opaque":      # walks stopped early: saturated pixels, with listed entries left behind them
        assert float((alpha > 0.995).float().mean()) > 0.2
    if kind == "empty":       # the background, T = 1
        assert torch.equal(out, bg.expand_as(out)) and float(alpha.abs().max()) == 0.0


def test_forward_over_a_list_that_carries_quadrant_masks():
    from sgn_rast import ops
    saved = ops.quadrant_masks
    ops.quadrant_masks = "on"
    try:
        ops.clear_binning_cache()
        before = ops.quadrant_mask_stats["binnings_with_masks"]
        _check_forward("base", 20, 0)
        assert ops.quadrant_mask_stats["binnings_with_masks"] == before + 1
    finally:
        ops.quadrant_masks = saved
        ops.clear_binning_cache()


def test_default_background_is_zero_and_bad_arguments_are_refused():
    S = _geo("base")
    feats, _ = _features(S["n"], 4)
    feats = feats.to(DEV)
    with torch.no_grad():
        a = F.rasterize_features(*S["geo"], feats, S["opac"], S["H"], S["W"])
        b = F.rasterize_features(*S["geo"], feats, S["opac"], S["H"], S["W"], background=torch.zeros(4, device=DEV))
    assert isinstance(a, torch.Tensor) and torch.equal(a, b)
    with pytest.raises(ValueError):
        F.rasterize_features(*S["geo"], feats, S["opac"], S["H"], S["W"], block_width=8)
    with pytest.raises(ValueError):
        F.rasterize_features(*S["geo"], feats[:, :0], S["opac"], S["H"], S["W"])
    with pytest.raises(ValueError):
        F.rasterize_features(*S["geo"], torch.zeros(S["n"], 65, device=DEV), S["opac"], S["H"], S["W"])


# ------------------------------------------------------------------ backward
def _weights(S, K):
    """Seeded image and alpha weights, as step.loss_weights builds them (K channels instead of three)."""
    g = torch.Generator().manual_seed(7)
    return torch.rand(S["H"], S["W"], K, generator=g), torch.rand(S["H"], S["W"], generator=g)


def _leaves(S, feats, dev, dtype, opac=None):
    xys, _d, _r, conics, _n = S["geo"]
    opac = S["opac"] if opac is None else opac
    return [t.detach().to(device=dev, dtype=dtype).clone().requires_grad_(True) for t in (xys, conics, feats, opac)]


def _grads(fn, S, K, dev=DEV, dtype=torch.float32, opac=None, **kw):
    feats, bg = _features(S["n"], K)
    w_img, w_a = _weights(S, K)
    t = _leaves(S, feats, dev, dtype, opac)
    _x, depths, radii, _c, nth = S["geo"]
    img, alpha = fn(t[0], depths.to(dev).to(dtype), radii.to(dev), t[1], nth.to(dev), t[2], t[3], S["H"], S["W"], 16,
                    bg.to(device=dev, dtype=dtype), True, **kw)
    ((img * w_img.to(device=dev, dtype=dtype)).sum() + (alpha * w_a.to(device=dev, dtype=dtype)).sum()).backward()
    return [x.grad.detach().cpu().double() for x in t]


_ORACLE = {}


def _oracle_grads(K):
    """fp64 autograd through the channel-generic torch oracle on the CPU; once per K."""
    if K not in _ORACLE:
        from oracle import torch_oracle as O
        _ORACLE[K] = _grads(O.rasterize_gaussians, _geo("grad"), K, dev="cpu", dtype=torch.float64)
    return _ORACLE[K]


NAMES = ("v_xy", "v_conic", "v_features", "v_opacity")


def _assert_grads(got, exp, what):
    errs = {n: rel_l2(a, b) for n, a, b in zip(NAMES, got, exp)}
    print(f"\nFEATURE_GRADS {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    for n, a, b in zip(NAMES, got, exp):
        assert a.shape == b.shape, (what, n)
        assert float(b.norm()) > 0, (what, n)
        assert errs[n] <= GRAD_BAR, (what, n, errs[n])


@pytest.mark.parametrize("K", [1, 5, 17, 20])
def test_backward_equals_autograd_through_the_oracle(K):
    _assert_grads(_grads(F.rasterize_features, _geo("grad"), K), _oracle_grads(K), f"K={K} vs oracle")


def test_backward_equals_the_multi_pass_form():
    from sgn_rast import ops
    S = _geo("grad")
    _assert_grads(_grads(F.rasterize_features, S, 20), _grads(ops.rasterize_gaussians, S, 20), "K=20 vs multi-pass")


def test_backward_under_the_upstream_clamp_variant():
    """`alpha_clamp_bwd` is read at call time.  On the oracle's scene (opacities <= 0.98: the clamp does not act) the variant
    still equals autograd; on a scene where it acts (opacities ~0.9999) the result equals the yardstick's under the same
    variant and differs from the default's."""
    from sgn_rast import ops
    S = _geo("grad")
    hot = S["logits"].clone()
    hot[:200] = 9.0
    hot = torch.sigmoid(hot)
    with ops.upstream_variant(alpha_clamp_bwd=0.999):
        _assert_grads(_grads(F.rasterize_features, S, 5), _oracle_grads(5), "K=5 vs oracle, clamp 0.999")
        got = _grads(F.rasterize_features, S, 5, opac=hot)
        ref = _grads(ops.rasterize_gaussians, S, 5, opac=hot)
    _assert_grads(got, ref, "K=5 vs multi-pass, clamp 0.999, opaque entries")
    default = _grads(F.rasterize_features, S, 5, opac=hot)
    assert rel_l2(default[3], got[3]) > 1e-3          # the setting reached the kernel


def test_backward_with_fused_opacity_logits():
    S = _geo("grad")

    def outside(xys, depths, radii, conics, nth, feats, logits, H, W, bw, bg, ra):
        return F.rasterize_features(xys, depths, radii, conics, nth, feats, torch.sigmoid(logits), H, W, bw, bg, ra)
    got = _grads(F.rasterize_features, S, 5, opac=S["logits"], opacity_is_logit=True)
    exp = _grads(outside, S, 5, opac=S["logits"])
    _assert_grads(got, exp, "K=5 logits inside vs torch.sigmoid outside")


def test_nothing_visible_gives_zero_gradients():
    S = _geo("empty")
    got = _grads(F.rasterize_features, S, 5)
    for g in got:
        assert float(g.abs().max()) == 0.0


# ------------------------------------------------------------------ expected depth
def _depth_grads(S, fused_projection, feature_form):
    from sgn_rast import fused, ops
    cam, P, H, W = S["cam"], S["P"], S["H"], S["W"]
    g = torch.Generator().manual_seed(11)
    w = torch.rand(H, W, generator=g).to(DEV)
    V = cam.viewmat.to(DEV)
    means = P["means"].detach().clone().requires_grad_(True)
    log_scales = P["log_scales"].detach().clone().requires_grad_(True)
    quats = P["quats"].detach().clone().requires_grad_(True)
    if fused_projection:
        xys, depths, radii, conics, _c, nth, _cov = fused.project_gaussians_fused(
            means, log_scales, quats, V[:3, :], cam.fx, cam.fy, cam.cx, cam.cy, H, W, 16)
        if feature_form:
            depth, _a = F.expected_depth(xys, depths, radii, conics, nth, P["opacity_logits"], H, W, opacity_is_logit=True)
        else:
            depth = fused.rasterize_gaussians_fused(xys, depths, radii, conics, nth, depths[:, None].repeat(1, 3),
                                                    P["opacity_logits"], H, W, 16,
                                                    background=torch.zeros(3, device=DEV))[..., 0]
    else:
        xys, depths, radii, conics, _c, nth, _cov = ops.project_gaussians(
            means, log_scales.exp(), 1.0, quats / quats.norm(dim=-1, keepdim=True), V, cam.fx, cam.fy, cam.cx, cam.cy,
            H, W, 16)
        opac = torch.sigmoid(P["opacity_logits"])
        if feature_form:
            depth, _a = F.expected_depth(xys, depths, radii, conics, nth, opac, H, W)
        else:
            depth = ops.rasterize_gaussians(xys, depths, radii, conics, nth, depths[:, None].repeat(1, 3), opac, H, W, 16,
                                            background=torch.zeros(3, device=DEV))[..., 0]
    (depth * w).sum().backward()
    return depth.detach(), [t.grad.detach().cpu().double() for t in (means, log_scales, quats)]


@pytest.mark.parametrize("fused_projection", [False, True], ids=["drop-in", "fused"])
def test_expected_depth_reaches_the_means_through_the_projection(fused_projection):
    from sgn_rast import ops
    S = _geo("grad")
    ops.clear_binning_cache()
    ref_img, ref = _depth_grads(S, fused_projection, feature_form=False)
    ops.clear_binning_cache()
    img, got = _depth_grads(S, fused_projection, feature_form=True)
    assert float(ref_img.max()) > 0.5
    assert float((img - ref_img).abs().max()) <= 1e-5 * float(ref_img.max())
    for name, a, b in zip(("means", "log_scales", "quats"), got, ref):
        e = rel_l2(a, b)
        print(f"\nEXPECTED_DEPTH {'fused' if fused_projection else 'drop-in'} {name}: {e:.3g}")
        assert float(b.norm()) > 0 and e <= GRAD_BAR, (name, e)


# ------------------------------------------------------------------ binning reuse
@pytest.mark.usefixtures("library_defaults")
@pytest.mark.parametrize("fused_rgb", [False, True], ids=["drop-in", "fused"])
def test_feature_pass_after_the_rgb_pass_bins_nothing(fused_rgb):
    from sgn_rast import fused, ops
    S = _geo("base")
    feats, _ = _features(S["n"], 20)
    feats = feats.to(DEV)
    rgb = torch.rand(S["n"], 3, device=DEV)
    ops.clear_binning_cache()
    b0 = ops.binning_stats["binnings"]
    with torch.no_grad():
        if fused_rgb:
            fused.rasterize_gaussians_fused(*S["geo"], rgb, S["logits"], S["H"], S["W"], 16)
            assert ops.binning_stats["binnings"] == b0 + 1
            F.rasterize_features(*S["geo"], feats, S["logits"], S["H"], S["W"], opacity_is_logit=True)
        else:
            ops.rasterize_gaussians(*S["geo"], rgb, S["opac"], S["H"], S["W"], 16)
            assert ops.binning_stats["binnings"] == b0 + 1
            F.rasterize_features(*S["geo"], feats, S["opac"], S["H"], S["W"])
    assert ops.binning_stats["binnings"] == b0 + 1            # the feature pass found the RGB pass's list
    ops.clear_binning_cache()
    with torch.no_grad():
        F.rasterize_features(*S["geo"], feats, S["opac"], S["H"], S["W"])
    assert ops.binning_stats["binnings"] == b0 + 2            # ... and bins for itself when there is none


# ------------------------------------------------------------------ semantic cross-entropy
def _within_8x(got, torch32, ref, scale, what):
    floor = 2.0 ** -24 * scale
    err = (got.double() - ref).abs()
    bound = 8.0 * torch.clamp((torch32.double() - ref).abs(), min=floor)
    worst = float((err / bound).max())
    print(f"\nSEMANTIC_CE {what}: worst err/bound {worst:.3g}  max err {float(err.max()):.3g}  floor {floor:.3g}")
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("K", [3, 19, 64])
def test_semantic_cross_entropy_against_the_fp64_definition(K):
    logits, labels, mask = SF.case(K)
    ref_loss, ref_grad = SF.cross_entropy_fp64(logits, labels, 255, mask)
    t_loss, t_grad = SF.torch_cross_entropy(logits.to(DEV), labels.to(DEV), 255, mask.to(DEV))
    x = logits.to(DEV).requires_grad_(True)
    loss = F.semantic_cross_entropy(x, labels.to(DEV)[..., None], ignore_index=255, mask=mask.to(DEV))
    (loss * 1.0).backward()
    assert loss.shape == () and x.grad.shape == x.shape
    _within_8x(loss.detach().cpu().reshape(1), t_loss.cpu().reshape(1), ref_loss.reshape(1), abs(float(ref_loss)),
               f"K={K} loss")
    _within_8x(x.grad.cpu(), t_grad.cpu(), ref_grad, float(ref_grad.abs().max()), f"K={K} gradient")
    dropped = ~SF.counted_pixels(labels, K, 255, mask)
    assert int(dropped.sum()) > 500 and float(x.grad.cpu()[dropped].abs().max()) == 0.0
    # neither option: every pixel counts
    x2 = logits.to(DEV).requires_grad_(True)
    lab2 = labels.clamp(max=K - 1)
    loss2 = F.semantic_cross_entropy(x2, lab2.to(DEV))
    loss2.backward()
    r2_loss, r2_grad = SF.cross_entropy_fp64(logits, lab2)
    t2_loss, t2_grad = SF.torch_cross_entropy(logits.to(DEV), lab2.to(DEV))
    _within_8x(loss2.detach().cpu().reshape(1), t2_loss.cpu().reshape(1), r2_loss.reshape(1), abs(float(r2_loss)),
               f"K={K} loss, plain")
    _within_8x(x2.grad.cpu(), t2_grad.cpu(), r2_grad, float(r2_grad.abs().max()), f"K={K} gradient, plain")


def test_semantic_cross_entropy_of_an_all_ignored_image():
    logits, labels, mask = SF.case(19, all_ignored=True)
    x = logits.to(DEV).requires_grad_(True)
    loss = F.semantic_cross_entropy(x, labels.to(DEV), ignore_index=255, mask=mask.to(DEV))
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(x.grad.abs().max()) == 0.0 and bool(torch.isfinite(x.grad).all())


def test_semantic_argmax_is_the_byte_class_map():
    logits, _l, _m = SF.case(19)
    got = F.semantic_argmax(logits.to(DEV))
    assert got.dtype is torch.uint8 and got.shape == logits.shape[:2]
    assert torch.equal(got.cpu().long(), logits.argmax(dim=-1))

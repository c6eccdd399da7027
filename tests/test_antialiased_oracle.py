"""CPU: the antialiased rasterize mode (`rasterize_mode="antialiased"`, the reference's dead config field made real:
opacity = sigmoid(logit) * the projection's compensation factor) on the reference arithmetic of `oracle/torch_oracle.py`
— the step layer's plumbing, the property the mode exists for (accumulation independent of the render resolution), and
the host-side errors."""
import pytest
import torch

W, H, FOCAL = 160, 96, 140.0


def _scene():
    from sgn_rast import scenes
    cam = scenes.make_camera(W, H, FOCAL)
    return cam, scenes.make_gaussians(3500, cam, seed=4, z_range=(2.0, 8.0))


@pytest.fixture(scope="module")
def renders(torch_oracle):
    """mode -> (render at 160x96, render at 80x48) of the same Gaussians on the oracle; computed once, left unchanged."""
    from sgn_rast import scenes, step
    cam, raw = _scene()
    half = scenes.make_camera(W // 2, H // 2, FOCAL / 2)
    with torch.no_grad():
        return {mode: tuple(step.render(raw, c, rasterize_mode=mode, ops=torch_oracle, with_depth=True)
                            for c in (cam, half)) for mode in ("classic", "antialiased")}


def _by_hand(P, cam, TO, antialiased):
    """`step.render`'s composition written out from the oracle's operators (sgn_splatfacto.py:857-996)."""
    Hh, Ww = cam.height, cam.width
    bg = torch.zeros(3)
    scales = torch.exp(P["log_scales"])
    colors = torch.cat((P["features_dc"], P["features_rest"]), dim=1)
    quats = P["quats"] / P["quats"].norm(dim=-1, keepdim=True)
    xys, depths, radii, conics, comp, nth, _ = TO.project_gaussians(
        P["means"], scales, 1, quats, cam.viewmat[:3, :], cam.fx, cam.fy, cam.cx, cam.cy, Hh, Ww, 16)
    viewdirs = P["means"].detach() - cam.cam_pos
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    rgbs = torch.clamp(TO.spherical_harmonics(3, viewdirs, colors) + 0.5, min=0.0)
    opac = torch.sigmoid(P["opacity_logits"])
    if antialiased:
        opac = torch.sigmoid(P["opacity_logits"]) * comp[:, None]
    rgb, alpha = TO.rasterize_gaussians(xys, depths, radii, conics, nth, rgbs, opac, Hh, Ww, 16, background=bg,
                                        return_alpha=True)
    dimg = TO.rasterize_gaussians(xys, depths, radii, conics, nth, depths[:, None].repeat(1, 3), opac, Hh, Ww, 16,
                                  torch.zeros(3))[..., 0:1]
    return rgb, alpha, torch.where(alpha[..., None] > 1e-3, dimg / alpha[..., None], 10), opac


def test_render_is_the_hand_written_composition(torch_oracle, renders):
    cam, raw = _scene()
    from sgn_rast import step
    with torch.no_grad():
        for mode in ("classic", "antialiased"):
            out = renders[mode][0]
            rgb, alpha, depth, opac = _by_hand(raw, cam, torch_oracle, mode == "antialiased")
            assert torch.equal(out.rgb, rgb) and torch.equal(out.alpha, alpha) and torch.equal(out.depth, depth), mode
            assert torch.equal(out.opacities, opac) and out.opacities.shape == raw["opacity_logits"].shape
        today = step.render(raw, cam, ops=torch_oracle, with_depth=True)        # no argument: the classic mode
    for k in ("rgb", "alpha", "depth", "opacities", "xys", "radii"):
        assert torch.equal(getattr(today, k), getattr(renders["classic"][0], k)), k
    assert float((renders["classic"][0].rgb - renders["antialiased"][0].rgb).abs().mean()) > 1e-2


def test_gradient_flows_through_the_factor(torch_oracle):
    """Autograd through the projection's compensation output: detaching the factor changes the covariance's gradients
    and leaves the logits' alone."""
    from sgn_rast import step
    cam, raw = _scene()
    w_img, w_a = step.loss_weights(cam, seed=7)
    P = step.leaf_params(raw)
    step.train_step(P, cam, w_img, w_a, ops=torch_oracle, rasterize_mode="antialiased")

    class Detached:                              # the oracle's namespace with the factor cut out of the graph
        spherical_harmonics = staticmethod(torch_oracle.spherical_harmonics)
        rasterize_gaussians = staticmethod(torch_oracle.rasterize_gaussians)

        @staticmethod
        def project_gaussians(*a, **k):
            out = list(torch_oracle.project_gaussians(*a, **k))
            out[4] = out[4].detach()
            return tuple(out)

    Q = step.leaf_params(raw)
    step.train_step(Q, cam, w_img, w_a, ops=Detached, rasterize_mode="antialiased")
    rel = lambda k: float((P[k].grad - Q[k].grad).norm() / P[k].grad.norm())
    assert rel("log_scales") > 0.05 and rel("quats") > 0.05
    assert torch.equal(P["opacity_logits"].grad, Q["opacity_logits"].grad)


def test_accumulation_is_consistent_across_resolutions(renders):
    """The property the mode exists for: at half the resolution the 0.3 px blur inflates every small Gaussian; the
    classic mode renders the scene denser, the antialiased one does not."""
    ratio = {mode: float(half.alpha.mean()) / float(full.alpha.mean()) for mode, (full, half) in renders.items()}
    print("mean accumulation 80x48 / 160x96:", ratio)
    assert abs(ratio["antialiased"] - 1.0) < 0.02, ratio
    assert ratio["classic"] > 1.10, ratio


def test_unknown_mode_is_a_value_error_everywhere(torch_oracle):
    from sgn_rast import scenes, step, views
    cam, raw = _scene()
    models, poses, idft = scenes.make_scene_graph(200, cam, n_objects=2, object_frac=0.25, z_range=(2.0, 8.0))
    w_img, w_a = step.loss_weights(cam, seed=7)
    bg = torch.zeros(3)
    calls = [
        lambda m: step.render(raw, cam, ops=torch_oracle, rasterize_mode=m),
        lambda m: step.render_fused(raw, cam, rasterize_mode=m),
        lambda m: step.render_scene_graph(models, poses, idft, cam, ops=torch_oracle, rasterize_mode=m),
        lambda m: step.render_scene_graph(models, poses, idft, cam, fused=True, rasterize_mode=m),
        lambda m: step.render_eval(raw, cam, bg, rasterize_mode=m),
        lambda m: step.render_eval(raw, cam, bg, fused=False, ops=torch_oracle, rasterize_mode=m),
        lambda m: step.render_scene_graph_eval(models, poses, idft, cam, bg, rasterize_mode=m),
        lambda m: step.render_scene_graph_eval(models, poses, idft, cam, bg, fused=False, ops=torch_oracle,
                                               rasterize_mode=m),
        lambda m: step.train_step(step.leaf_params(raw), cam, w_img, w_a, ops=torch_oracle, rasterize_mode=m),
        lambda m: step.train_step(step.leaf_params(raw), cam, w_img, w_a, fused=True, rasterize_mode=m),
        lambda m: views.render_views(raw, [cam, cam], rasterize_mode=m),
        lambda m: views.train_step_views(raw, [cam, cam], [torch.zeros(H, W, 3)] * 2, rasterize_mode=m),
    ]
    for call in calls:
        for bad in ("Antialiased", "aa", "", None):
            with pytest.raises(ValueError, match="rasterize_mode"):
                call(bad)


def test_batched_views_refuse_the_mode_on_the_host():
    """CPU tensors, no GPU: the refusal comes before any device work (the classic mode would fail on the device check)."""
    from sgn_rast import views
    cam, raw = _scene()
    with pytest.raises(NotImplementedError, match="batched views"):
        views.render_views(raw, [cam, cam], rasterize_mode="antialiased")
    with pytest.raises(NotImplementedError, match="batched views"):
        views.train_step_views(raw, [cam, cam], [torch.zeros(H, W, 3)] * 2, rasterize_mode="antialiased")

"""GPU: batched views (sgn_rast.views.render_views) against the single-view fused path, view by view — forward bit for
bit, gradients as the sum of the single-view backward passes — plus run-to-run determinism of the summed parts,
densification statistics, one host wait per batched forward, and a short multi-view fit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LEAVES = ("means", "log_scales", "quats", "opacity_logits", "features_dc", "features_rest")


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _cam(w, h, focal, yaw=0.0, t=(0.0, 0.0, 0.0)):
    """A yawed camera whose centre sits at ``t`` (world -> camera: R^T (x - t))."""
    from sgn_rast import scenes
    c = scenes.make_camera(w, h, focal, yaw=yaw)
    R_w2c = c.viewmat[:3, :3]
    tt = torch.tensor(t, dtype=torch.float32)
    c.viewmat[:3, 3] = -(R_w2c @ tt)
    c.cam_pos = tt.clone()
    return c


def _to_dev(cam):
    cam.viewmat, cam.cam_pos = cam.viewmat.to(DEV), cam.cam_pos.to(DEV)
    return cam


def _scene(kind, n, w=1920, h=1280, focal=2000.0, seed=0):
    from sgn_rast import scenes, step
    base = scenes.make_camera(w, h, focal)
    if kind == "street":
        raw = scenes.make_street_gaussians(n, base, seed=seed)
    else:
        raw = scenes.make_gaussians(n, base, seed=seed, z_range=(2.0, 60.0))
    return {k: v.to(DEV) for k, v in raw.items()}


def _leaves(raw):
    from sgn_rast import step
    return step.leaf_params(raw)


def _single(raw, cams, with_depth=False, grads=True, weights=None):
    """render_fused per camera; with `grads`, the sum over the views of each leaf's gradient of the same loss."""
    from sgn_rast import step
    outs, acc = [], {k: torch.zeros_like(v) for k, v in raw.items()}
    for b, cam in enumerate(cams):
        P = _leaves(raw)
        o = step.render_fused(P, cam, with_depth=with_depth)
        outs.append(o)
        if grads:
            w_img, w_a = weights[b]
            ((o.rgb * w_img).sum() + (o.alpha * w_a).sum()).backward()
            for k in acc:
                acc[k] += P[k].grad
    return outs, acc


def _weights(cams, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(c.height, c.width, 3, generator=g).to(DEV), torch.rand(c.height, c.width, generator=g).to(DEV))
            for c in cams]


def _batched(raw, cams, with_depth=False, weights=None):
    from sgn_rast import views
    P = _leaves(raw)
    out = views.render_views(P, cams, with_depth=with_depth)
    if weights is not None:
        loss = sum((out.rgb[b] * weights[b][0]).sum() + (out.alpha[b] * weights[b][1]).sum() for b in range(len(cams)))
        loss.backward()
    return out, P


def _assert_views_equal(out, singles, with_depth=False):
    for b, o in enumerate(singles):
        for name in ("rgb", "alpha", "xys", "depths", "radii", "conics", "num_tiles_hit") + (("depth",) if with_depth else ()):
            got, exp = getattr(out, name)[b], getattr(o, name)
            assert torch.equal(got.detach(), exp.detach()), (b, name, float((got.double() - exp.double()).abs().max()))


CAM_SETS = {
    "yawed": lambda: [_cam(1920, 1280, 2000.0, yaw=y, t=(0.3 * y, 0.0, 0.5 * y)) for y in (0.0, 0.15, -0.2, 0.35)],
    "with_empty_and_twin": lambda: [_cam(1920, 1280, 2000.0), _cam(1920, 1280, 2000.0, yaw=math.pi),
                                    _cam(1920, 1280, 2000.0), _cam(1920, 1280, 2000.0, yaw=0.1, t=(1.0, 0.2, -1.0))],
    "side_1920x886": lambda: [_cam(1920, 886, 1400.0, yaw=y) for y in (-0.9, 0.0, 0.9)],
}


def test_one_view_equals_render_fused():
    raw = _scene("c2", 50_000)
    cams = [_to_dev(_cam(1920, 1280, 2000.0, yaw=0.1))]
    w = _weights(cams)
    singles, exp = _single(raw, cams, with_depth=True, weights=w)
    out, P = _batched(raw, cams, with_depth=True, weights=w)
    _assert_views_equal(out, singles, with_depth=True)
    for k in LEAVES:
        assert rel_l2(P[k].grad, exp[k]) <= 1e-6, k


@pytest.mark.parametrize("kind", ["c2", "street"])
@pytest.mark.parametrize("cams_name,B", [("yawed", 2), ("yawed", 3), ("yawed", 4), ("with_empty_and_twin", 4),
                                         ("side_1920x886", 3)])
def test_forward_is_bit_identical_per_view(kind, cams_name, B):
    cams = [_to_dev(c) for c in CAM_SETS[cams_name]()[:B]]
    raw = _scene(kind, 200_000, w=cams[0].width, h=cams[0].height, focal=cams[0].fx)
    singles, _ = _single(raw, cams, grads=False)
    out, _ = _batched(raw, cams)
    _assert_views_equal(out, singles)
    if cams_name == "with_empty_and_twin":
        assert int(out.num_tiles_hit[1].sum()) == 0
        assert torch.equal(out.rgb[1], torch.zeros_like(out.rgb[1]))       # pure background (zeros)
        assert torch.equal(out.rgb[0], out.rgb[2])                          # the same camera twice


def test_eight_views_and_edge_straddlers():
    """B = 8, and Gaussians centred on / just past the bottom and right edges (H not a multiple of 16)."""
    from sgn_rast import scenes
    cams = [_to_dev(_cam(1000, 700, 900.0, yaw=0.05 * b, t=(0.1 * b, 0.0, 0.0))) for b in range(8)]
    raw = _scene("c2", 60_000, w=1000, h=700, focal=900.0, seed=5)
    g = torch.Generator().manual_seed(9)
    m = raw["means"].clone().cpu()
    k = 4000
    z = torch.rand(k, generator=g) * 20 + 3
    u = torch.where(torch.rand(k, generator=g) < 0.5, torch.full((k,), 1000.0), torch.rand(k, generator=g) * 1000)
    v = torch.where(u >= 1000.0, torch.rand(k, generator=g) * 700, torch.full((k,), 700.0))
    u = u + (torch.rand(k, generator=g) - 0.5) * 12
    v = v + (torch.rand(k, generator=g) - 0.5) * 12
    m[:k] = torch.stack([(u - 500.0) / 900.0 * z, (v - 350.0) / 900.0 * z, z], -1)
    raw["means"] = m.to(DEV)
    singles, _ = _single(raw, cams, grads=False)
    out, _ = _batched(raw, cams)
    _assert_views_equal(out, singles)


def test_no_view_leaks_into_its_neighbours_tiles():
    """Every Gaussian is visible from camera 0 only (cameras 1-3 look away): views 1-3 are pure background, exactly."""
    cams = [_to_dev(_cam(640, 480, 600.0, yaw=y)) for y in (0.0, math.pi / 2, math.pi, -math.pi / 2)]
    raw = _scene("c2", 30_000, w=640, h=480, focal=600.0, seed=2)
    raw["means"][:, 2] = raw["means"][:, 2].clamp(min=8.0)
    singles, _ = _single(raw, cams, grads=False)
    out, _ = _batched(raw, cams)
    _assert_views_equal(out, singles)
    assert int(out.num_tiles_hit[0].sum()) > 0
    for b in (1, 2, 3):
        assert int(out.num_tiles_hit[b].sum()) == 0
        assert torch.equal(out.alpha[b], torch.zeros_like(out.alpha[b]))


@pytest.mark.parametrize("kind", ["c2", "street"])
def test_gradients_are_sums_of_single_view_gradients(kind):
    cams = [_to_dev(c) for c in CAM_SETS["yawed"]()]
    raw = _scene(kind, 200_000)
    w = _weights(cams)
    _, exp = _single(raw, cams, weights=w)
    out, P = _batched(raw, cams, weights=w)
    for k in LEAVES:
        assert rel_l2(P[k].grad, exp[k]) <= 1e-5, (k, rel_l2(P[k].grad, exp[k]))


def test_projection_sh_and_opacity_sums_are_deterministic():
    """The per-view sums inside the projection, SH and opacity reductions have a fixed order: given the same per-row
    gradients, the leaf gradients come out bit-identical on every run."""
    from sgn_rast import views
    cams = [_to_dev(c) for c in CAM_SETS["yawed"]()]
    raw = _scene("c2", 200_000)
    P = _leaves(raw)
    out = views.render_views(P, cams)
    g = torch.Generator().manual_seed(1)
    v_xys = torch.randn(out.xys.shape, generator=g).to(DEV)
    v_con = torch.randn(out.conics.shape, generator=g).to(DEV)
    v_rgb = torch.randn(out.rgbs.shape, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        grads = torch.autograd.grad([out.xys, out.conics, out.rgbs], [P["means"], P["log_scales"], P["quats"],
                                                                      P["features_dc"], P["features_rest"]],
                                    [v_xys, v_con, v_rgb], retain_graph=True)
        runs.append(grads)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # the opacity part: the batched unpack sums d/d logit over the views in ascending order
    w = _weights(cams)
    opac = []
    for _ in range(2):
        o, P2 = _batched(raw, cams, weights=w)
        opac.append(P2["opacity_logits"].grad)
    assert rel_l2(opac[0], opac[1]) <= 1e-6       # (the raster backward's atomics remain: equal to rounding)


def test_at_size_one_million_three_views():
    cams = [_to_dev(_cam(1920, 1280, 2000.0, yaw=y, t=(0.2 * y, 0.0, 0.0))) for y in (-0.25, 0.0, 0.25)]
    raw = _scene("c2", 1_000_000, seed=7)
    w = _weights(cams)
    singles, exp = _single(raw, cams, weights=w)
    out, P = _batched(raw, cams, weights=w)
    _assert_views_equal(out, singles)
    for k in LEAVES:
        assert rel_l2(P[k].grad, exp[k]) <= 1e-5, (k, rel_l2(P[k].grad, exp[k]))


def test_densification_statistics_match_sequential_views():
    from sgn_rast import densify
    cams = [_to_dev(c) for c in CAM_SETS["yawed"]()]
    raw = _scene("c2", 100_000)
    w = _weights(cams)
    seq = densify.Stats()
    for b, cam in enumerate(cams):
        from sgn_rast import step
        P = _leaves(raw)
        o = step.render_fused(P, cam)
        ((o.rgb * w[b][0]).sum() + (o.alpha * w[b][1]).sum()).backward()
        seq.update(o.xys.grad, o.radii, (cam.height, cam.width))
    out, _ = _batched(raw, cams, weights=w)
    bat = densify.Stats()
    for b, cam in enumerate(cams):
        bat.update(out.xys.grad[b], out.radii[b], (cam.height, cam.width))
    assert torch.equal(bat.vis_counts, seq.vis_counts)
    assert torch.equal(bat.max_2Dsize, seq.max_2Dsize)
    assert rel_l2(bat.xys_grad_norm, seq.xys_grad_norm) <= 1e-6


def test_one_host_wait_per_batched_forward(library_defaults):
    from sgn_rast import _lib as L
    from sgn_rast import views
    cams = [_to_dev(c) for c in CAM_SETS["yawed"]()]
    raw = _scene("c2", 100_000)
    P = _leaves(raw)
    with torch.no_grad():
        views.render_views(P, cams)               # sizes the list's capacity for this shape
        torch.cuda.synchronize()
        lib = L.load()
        import ctypes
        n = ctypes.c_int64(0)
        lib.sgn_timing_host_wait_us(1, ctypes.byref(n))
        misses = views.stats["capacity_misses"]
        views.render_views(P, cams)
        lib.sgn_timing_host_wait_us(0, ctypes.byref(n))
    assert views.stats["capacity_misses"] == misses
    assert n.value == 1


def test_short_fit_follows_sequential_accumulation():
    """50 steps of 4 views: render_views + train-step loss against sequential render_fused with gradient accumulation
    (mean of the per-view photometric losses), same Adam: final PSNR within 0.01 dB."""
    from sgn_rast import loss as LS
    from sgn_rast import step, views
    cams = [_to_dev(_cam(320, 240, 300.0, yaw=y)) for y in (-0.1, 0.0, 0.1, 0.2)]
    raw = _scene("c2", 20_000, w=320, h=240, focal=300.0, seed=11)
    tgt = _scene("c2", 20_000, w=320, h=240, focal=300.0, seed=12)
    with torch.no_grad():
        gts = [step.render_fused(_leaves(tgt), c).rgb.clamp(max=1.0).detach() for c in cams]

    def fit(batched):
        P = _leaves(raw)
        opt = torch.optim.Adam(list(P.values()), lr=1e-3)
        for _ in range(50):
            opt.zero_grad(set_to_none=True)
            if batched:
                views.train_step_views(P, cams, gts, zero_grad=False)
            else:
                for b, c in enumerate(cams):
                    o = step.render_fused(P, c)
                    (LS.photometric_loss(o.rgb, gts[b], 0.2, clamp_max=1.0) / len(cams)).backward()
            opt.step()
        with torch.no_grad():
            mse = sum(float(((step.render_fused(P, c).rgb.clamp(max=1.0) - g) ** 2).mean()) for c, g in zip(cams, gts))
        return -10 * math.log10(mse / len(cams))

    a, b = fit(True), fit(False)
    assert abs(a - b) <= 0.01, (a, b)

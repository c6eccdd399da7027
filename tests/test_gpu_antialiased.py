"""GPU (-m gpu): the antialiased rasterize mode (`rasterize_mode="antialiased"`: opacity = sigmoid(logit) * the
projection's compensation factor) — the kernel pair of csrc/antialias.hip per element against float64, and the mode
through every layer that takes it (fused front end, train step, scene graph, eval renders, LiDAR term, empty view)
against the reference composition on the CPU oracle.  Tolerances are those of the classic mode's tests, named where used."""
import pytest
import torch

import test_gpu_eval_render as TE
import test_gpu_fused as TF
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
AA = "antialiased"
U = 2.0 ** -24            # half an fp32 ulp of 1


# ---------------------------------------------------------------- the kernel pair

def _pair_inputs(n, clamp8=False):
    """Logits: seeded normal x 4 and {-20, -8, 0, 8, 20}; compensation: seeded uniform(0, 1) and {0, 1e-6, 1} (every
    combination of the special values in the first 15 rows where n allows); v_o: seeded normal."""
    g = torch.Generator().manual_seed(100 + n)
    logits = torch.randn(n, generator=g) * 4
    comp = torch.rand(n, generator=g)
    v_o = torch.randn(n, generator=g)
    if n >= 15:
        sl, sc = torch.tensor([-20.0, -8.0, 0.0, 8.0, 20.0]), torch.tensor([0.0, 1e-6, 1.0])
        logits[:15], comp[:15] = sl.repeat_interleave(3), sc.repeat(5)
    if n >= 32:
        comp[20:32:3] = 0.0                        # culled rows among ordinary logits
    if clamp8:
        logits = logits.clamp(-8.0, 8.0)
    return logits, comp, v_o


def _pair64(logits, comp, v_o):
    l, c, v = logits.double(), comp.double(), v_o.double()
    s = 1.0 / (1.0 + torch.exp(-l))
    return s * c, v * c * s * (1.0 - s), v * s


def _run_pair(logits, comp, v_o, two_d):
    from sgn_rast import fused
    l = (logits[:, None] if two_d else logits).to(DEV).requires_grad_(True)
    c = comp.to(DEV).requires_grad_(True)
    o = fused.antialiased_opacities(l, c)
    assert o.shape == (logits.shape[0],) and o.dtype == torch.float32
    assert type(o.grad_fn).__name__ == "_AntialiasedOpacitiesBackward"           # the kernel ran
    o.backward(v_o.to(DEV))
    assert l.grad.shape == l.shape and c.grad.shape == c.shape
    return o.detach().cpu(), l.grad.reshape(-1).cpu(), c.grad.cpu()


@pytest.mark.parametrize("two_d", [False, True], ids=["logits[N]", "logits[N,1]"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_kernel_pair_per_element_against_float64(n, two_d):
    """|o - o64| <= 8 * 2^-24 * o64 (two ulp for expf, one rounding each for the add, the divide and the multiply, a
    twofold margin); v_c the same; v_l, logits within [-8, 8]: <= 8 * 2^-24 * |v_o c| (s (1 - s) <= 1/4 and its
    absolute error is at most about 4.5 * 2^-24).  Rows with c = 0: exact zeros in o and v_l."""
    logits, comp, v_o = _pair_inputs(n)
    o, v_l, v_c = _run_pair(logits, comp, v_o, two_d)
    o64, _, v_c64 = _pair64(logits, comp, v_o)
    e_o = float(((o.double() - o64).abs() / o64.clamp(min=1e-300)).max())
    e_c = float(((v_c.double() - v_c64).abs() / v_c64.abs().clamp(min=1e-300)).max())
    assert bool(((o.double() - o64).abs() <= 8 * U * o64).all()), e_o / U
    assert bool(((v_c.double() - v_c64).abs() <= 8 * U * v_c64.abs()).all()), e_c / U
    culled = comp == 0
    assert bool((o[culled] == 0).all()) and bool((v_l[culled] == 0).all())
    assert bool(torch.isfinite(v_l).all())
    # the logits' gradient, on logits within [-8, 8]
    logits8, comp, v_o = _pair_inputs(n, clamp8=True)
    o8, v_l, v_c8 = _run_pair(logits8, comp, v_o, two_d)
    _, v_l64, _ = _pair64(logits8, comp, v_o)
    scale = (v_o.double() * comp.double()).abs()
    e_l = float(((v_l.double() - v_l64).abs() / scale.clamp(min=1e-300))[scale > 0].max()) if bool((scale > 0).any()) else 0.0
    print(f"[aa pair] n={n} 2d={two_d}: o {e_o / U:.2f}  v_c {e_c / U:.2f}  v_l {e_l / U:.2f}  (units of 2^-24; bound 8)")
    assert bool(((v_l.double() - v_l64).abs() <= 8 * U * scale).all()), e_l / U
    assert bool((v_l[comp == 0] == 0).all())


@pytest.mark.parametrize("n", [257, 1000])
def test_an_unwanted_gradient_leaves_the_other_unchanged(n):
    """A NULL output pointer at the C entry, and `requires_grad=False` at the autograd node."""
    from sgn_rast import _lib as L, fused
    logits, comp, v_o = (t.to(DEV) for t in _pair_inputs(n))
    lib = L.load()
    both = [torch.full((n,), 7.0, device=DEV) for _ in range(2)]
    only_l, only_c = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
    call = lambda vl, vc: L.check(lib.sgn_aa_opacity_bwd(n, L.ptr(logits), L.ptr(comp), L.ptr(v_o), L.ptr(vl), L.ptr(vc),
                                                         L.stream_ptr()), "sgn_aa_opacity_bwd")
    call(both[0], both[1])
    call(only_l, None)
    call(None, only_c)
    call(None, None)
    torch.cuda.synchronize()
    assert torch.equal(only_l, both[0]) and torch.equal(only_c, both[1])
    assert not bool((both[0] == 7.0).all()) and not bool((both[1] == 7.0).all())
    for want_l, want_c in ((True, False), (False, True)):
        l, c = logits.clone().requires_grad_(want_l), comp.clone().requires_grad_(want_c)
        fused.antialiased_opacities(l, c).backward(v_o)
        assert (l.grad is None) == (not want_l) and (c.grad is None) == (not want_c)
        assert torch.equal(l.grad if want_l else c.grad, both[0] if want_l else both[1])
    with torch.no_grad():
        assert fused.antialiased_opacities(logits, comp).grad_fn is None


# ---------------------------------------------------------------- through the fused front end

def _aa_scene():
    from sgn_rast import scenes
    cam = scenes.make_camera(160, 96, 140.0)
    return cam, scenes.make_gaussians(3500, cam, seed=4, z_range=(2.0, 8.0))


def _to_dev(cam):
    cam.viewmat, cam.cam_pos = cam.viewmat.to(DEV), cam.cam_pos.to(DEV)
    return cam


def test_compensation_of_ones_is_the_classic_fused_path():
    from sgn_rast import fused, ops, step
    cam, raw = _aa_scene()
    cam = _to_dev(cam)
    w_img, w_a = step.loss_weights(cam, seed=7, device=DEV)
    res = []
    for ones in (False, True):
        P = step.leaf_params({k: v.to(DEV) for k, v in raw.items()})
        xys, depths, radii, conics, _c, nth, _ = fused.project_gaussians_fused(
            P["means"], P["log_scales"], P["quats"], cam.viewmat[:3, :], cam.fx, cam.fy, cam.cx, cam.cy, cam.height,
            cam.width, 16)
        rgbs = fused.spherical_harmonics_fused(3, P["means"], cam.cam_pos, P["features_dc"], P["features_rest"])
        ops.clear_binning_cache()
        kw = dict(compensation=torch.ones(raw["means"].shape[0], device=DEV)) if ones else {}
        img, alpha = fused.rasterize_gaussians_fused(xys, depths, radii, conics, nth, rgbs, P["opacity_logits"], cam.height,
                                                     cam.width, 16, torch.zeros(3, device=DEV), True, **kw)
        ((img * w_img).sum() + (alpha * w_a).sum()).backward()
        res.append((img.detach(), alpha.detach(), P["opacity_logits"].grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].mean()) > 0.3 and float(res[0][2].abs().sum()) > 0
    assert rel_l2(res[1][2], res[0][2]) < 1e-5               # (tests/test_gpu_fused.py's same-path figure)


class _FactorDetached:
    """An operator namespace with the projection's compensation output cut out of the autograd graph."""

    def __init__(self, ops):
        self.spherical_harmonics, self.rasterize_gaussians, self._project = (
            ops.spherical_harmonics, ops.rasterize_gaussians, ops.project_gaussians)

    def project_gaussians(self, *a, **k):
        out = list(self._project(*a, **k))
        out[4] = out[4].detach()
        return tuple(out)


def _oracle_step(raw, object_ids, poses, idft, cam, w_img, w_a, TO, mode=AA, ops=None):
    """tests/test_gpu_fused.py's expected side: the reference composition on the CPU oracle, autograd through the glue."""
    from sgn_rast import step
    Pc, comp = TF._composite_params(raw, object_ids, poses, idft, TO)
    exp = step.render(comp, cam, 3, 16, with_depth=True, ops=ops or TO, rasterize_mode=mode)
    loss = ((exp.rgb * w_img).sum() + (exp.alpha * w_a).sum()) / (cam.height * cam.width)
    loss.backward()
    return Pc, exp, loss


@pytest.mark.parametrize("with_objects", [False, True])
def test_fused_train_step_matches_reference_composition(torch_oracle, with_objects):
    """`test_gpu_fused.py::test_fused_train_step_matches_reference_composition` in antialiased mode, its tolerances
    unchanged; and, on the oracle alone, that the mode and the gradient through the factor are large enough here for
    those tolerances to notice a build without them."""
    from sgn_rast import step
    cam, raw, object_ids, poses, idft = TF._scene_graph_scene(local_objects=with_objects)
    if not with_objects:
        object_ids = torch.zeros_like(object_ids)
    w_img, w_a = step.loss_weights(cam, seed=7)
    Pc, exp, loss = _oracle_step(raw, object_ids, poses, idft, cam, w_img, w_a, torch_oracle)
    # (a) the mode changes the image, (b) the factor's own gradient matters — oracle against oracle
    _, classic, _ = _oracle_step(raw, object_ids, poses, idft, cam, w_img, w_a, torch_oracle, mode="classic")
    Pn, _, _ = _oracle_step(raw, object_ids, poses, idft, cam, w_img, w_a, torch_oracle,
                            ops=_FactorDetached(torch_oracle))
    d_img = float((exp.rgb.detach() - classic.rgb.detach()).abs().mean())
    d_ls, d_q = rel_l2(Pn["log_scales"].grad, Pc["log_scales"].grad), rel_l2(Pn["quats"].grad, Pc["quats"].grad)
    print(f"[aa step] objects={with_objects}: oracle classic-vs-aa rgb {d_img:.4f}; factor detached: log_scales "
          f"{d_ls:.4f} quats {d_q:.4f}")
    assert d_img > 1e-2
    assert d_ls > 0.05 and d_q > 0.05
    assert torch.equal(Pn["opacity_logits"].grad, Pc["opacity_logits"].grad)
    # fused HIP path on raw parameters
    cam = _to_dev(cam)
    Pd = step.leaf_params({k: v.to(DEV) for k, v in raw.items()})
    got = step.train_step(Pd, cam, w_img.to(DEV), w_a.to(DEV), with_depth=True, fused=True, rasterize_mode=AA,
                          object_ids=object_ids.to(DEV), poses=poses.to(DEV), idft=idft.to(DEV))
    vis = exp.radii > 0
    assert float((got.radii.cpu() != exp.radii).float().mean()) < 2e-3
    assert float((got.xys.detach().cpu() - exp.xys.detach())[vis].abs().max()) < 2e-3
    for name in ("rgb", "alpha"):
        err = (getattr(got, name).detach().cpu() - getattr(exp, name).detach()).abs()
        print(f"[aa step] {name}: mean {float(err.mean()):.2e}  >1e-3: {float((err > 1e-3).float().mean()):.2e}")
        assert float(err.mean()) < 2e-5 and float((err > 1e-3).float().mean()) < 5e-3, (name, float(err.mean()))
    assert abs(float(got.loss) - float(loss.detach())) < 1e-4
    rels = {k: rel_l2(Pd[k].grad.cpu(), Pc[k].grad) for k in Pd}
    print("[aa step] grads:", "  ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    for k, v in rels.items():
        assert v < 2e-3, k
    assert got.opacities.shape == (raw["means"].shape[0],) and got.opacities.requires_grad


def test_unfused_hip_equals_fused_hip():
    """`test_gpu_fused.py::test_fused_equals_unfused_hip_path` in antialiased mode, its tolerances unchanged."""
    from sgn_rast import scenes, step
    cam, raw = scenes.make_scene("c1", n_override=6000)
    cam = _to_dev(cam)
    w_img, w_a = step.loss_weights(cam, seed=7, device=DEV)
    Pa = step.leaf_params({k: v.to(DEV) for k, v in raw.items()})
    Pb = step.leaf_params({k: v.to(DEV) for k, v in raw.items()})
    Pc = step.leaf_params({k: v.to(DEV) for k, v in raw.items()})
    a = step.train_step(Pa, cam, w_img, w_a, with_depth=True, rasterize_mode=AA)
    b = step.train_step(Pb, cam, w_img, w_a, with_depth=True, fused=True, rasterize_mode=AA)
    c = step.train_step(Pc, cam, w_img, w_a, with_depth=True, fused=True)
    assert float((a.radii != b.radii).float().mean()) < 1e-3
    assert float((a.rgb - b.rgb).abs().mean()) < 1e-6 and float((a.alpha - b.alpha).abs().mean()) < 1e-6
    assert float((a.depth - b.depth).abs().mean()) < 1e-3
    for k in Pa:
        assert rel_l2(Pb[k].grad, Pa[k].grad) < 1e-3, k
    assert not torch.equal(b.alpha, c.alpha) and not torch.equal(b.rgb, c.rgb)        # (the mode is on)
    # the depth channel in the colour pass and the second pass over the same opacities agree, as in classic mode
    Pd = step.leaf_params({k: v.to(DEV) for k, v in raw.items()})
    d = step.train_step(Pd, cam, w_img, w_a, with_depth=True, fused=True, rasterize_mode=AA, depth_channel=False)
    assert torch.equal(d.rgb, b.rgb) and float((d.depth - b.depth).abs().mean()) < 1e-3


# ---------------------------------------------------------------- scene graph

def test_scene_graph_replay_fused_vs_dropin_vs_oracle(torch_oracle):
    """`test_gpu_fused.py::test_scene_graph_replay_fused_vs_dropin_vs_oracle` in antialiased mode (its scene, loss and
    tolerances), the fused form with the group accumulations and with the two id-range passes."""
    from sgn_rast import scenes, step
    cam = scenes.make_camera(160, 96, 140.0)
    models, poses, idft = scenes.make_scene_graph(4000, cam, n_objects=3, object_frac=0.25, z_range=(2.0, 8.0))
    poses[1:, 11] = torch.tensor([4.0, 5.0, 6.0])
    poses[1:, 9] = torch.tensor([-1.0, 0.2, 1.0]); poses[1:, 10] = 0.0
    w_img, w_a = step.loss_weights(cam, seed=7)

    def run(dev, mode=AA, **kw):
        cam_d = scenes.make_camera(160, 96, 140.0)
        cam_d.viewmat, cam_d.cam_pos = cam_d.viewmat.to(dev), cam_d.cam_pos.to(dev)
        leaves = [step.leaf_params({k: v.to(dev) for k, v in m.items()}) for m in models]
        out = step.render_scene_graph(leaves, poses.to(dev), idft.to(dev), cam_d, rasterize_mode=mode, **kw)
        loss = ((out.rgb * w_img.to(dev)).sum() + (out.alpha * w_a.to(dev)).sum() +
                (out.object_acc * w_a.to(dev)).sum()) / (cam.height * cam.width)
        loss.backward()
        return out, leaves, float(loss)

    exp, Le, le = run("cpu", ops=torch_oracle)
    classic, _, _ = run("cpu", mode="classic", ops=torch_oracle)
    assert float((exp.object_acc - classic.object_acc).abs().mean()) > 1e-3          # (the sub-model passes take the mode)
    assert float((exp.alpha - classic.alpha).abs().mean()) > 1e-2
    for name, kw in (("drop-in", {}), ("fused groups", dict(fused=True, groups=True)),
                     ("fused id-range", dict(fused=True, groups=False))):
        got, Lg, lg = run(DEV, **kw)
        assert abs(lg - le) < 1e-4, name
        for k in ("rgb", "alpha", "object_acc", "background_acc"):
            err = (getattr(got, k).detach().cpu() - getattr(exp, k).detach()).abs()
            assert float(err.mean()) < 2e-5 and float((err > 1e-3).float().mean()) < 5e-3, (name, k, float(err.mean()))
        rels = [rel_l2(mg[k].grad.cpu(), me[k].grad) for mg, me in zip(Lg, Le) for k in mg]
        print(f"[aa graph] {name}: loss err {abs(lg - le):.2e}  worst grad rel-L2 {max(rels):.2e}")
        for mg, me in zip(Lg, Le):
            for k in mg:
                assert rel_l2(mg[k].grad.cpu(), me[k].grad) < 2e-3, (name, k)
    assert float(exp.object_acc.max()) > 0.5 and float(exp.background_acc.max()) > 0.5


# ---------------------------------------------------------------- eval renders

@pytest.fixture(scope="module")
def eval_graph():
    """tests/test_gpu_eval_render.py's scene on the CPU, with its oracle replays in antialiased mode (computed once)."""
    from oracle import torch_oracle as TO
    from sgn_rast import scenes, step
    cam = scenes.make_camera(TE.W, TE.H, TE.FOCAL)
    models, poses, idft = scenes.make_scene_graph(6000, cam, n_objects=4, object_frac=0.2, fourier_dim=5, seed=3,
                                                  z_range=(1.5, 9.0), object_depth=(3.0, 7.0), object_extent=0.4)
    sky = torch.rand(TE.H, TE.W, 3, generator=torch.Generator().manual_seed(2))
    bg = torch.tensor([0.1, 0.2, 0.3])
    want_graph = step.render_scene_graph_eval(models, poses, idft, cam, bg, sky=sky, fused=False, ops=TO, rasterize_mode=AA)
    want_single = step.render_eval(models[0], cam, bg, sky=sky, fused=False, ops=TO, rasterize_mode=AA)
    classic = step.render_scene_graph_eval(models, poses, idft, cam, bg, sky=sky, fused=False, ops=TO)
    return models, poses, idft, sky, bg, want_graph, want_single, classic


def test_eval_renders(eval_graph):
    """Layered and un-layered bit-equal, as in classic mode; both, and `render_eval`, within
    tests/test_gpu_eval_render.py's tolerances of the oracle replay."""
    from sgn_rast import layers, ops, step
    models, poses, idft, sky, bg, want_graph, want_single, classic = eval_graph
    assert float((want_graph["accumulation"] - classic["accumulation"]).abs().mean()) > 1e-2
    assert float((want_graph["object_acc"] - classic["object_acc"]).abs().mean()) > 1e-3
    Ms = [{k: v.to(DEV) for k, v in m.items()} for m in models]
    p, w, sky_d, bg_d = poses.to(DEV), idft.to(DEV), sky.to(DEV), bg.to(DEV)
    ops.clear_binning_cache()
    calls = layers.stats["calls"]
    one = step.render_scene_graph_eval(Ms, p, w, TE._cam(), bg_d, sky=sky_d, fused=True, rasterize_mode=AA)
    assert layers.stats["calls"] == calls + 1
    multi = step.render_scene_graph_eval(Ms, p, w, TE._cam(), bg_d, sky=sky_d, fused=True, layered=False, rasterize_mode=AA)
    six = step.render_scene_graph_eval(Ms, p, w, TE._cam(), bg_d, sky=sky_d, fused=False, rasterize_mode=AA)
    assert set(one) == set(multi) == set(six) == set(want_graph) == TE.KEYS
    for k in TE.KEYS:
        assert torch.equal(one[k], multi[k]), (k, float((one[k] - multi[k]).abs().max()))
        for name, got in (("layered", one), ("drop-in", six)):
            if k == "depth":
                TE._close_depth(got[k].cpu(), want_graph[k])
            else:
                TE._close(got[k].cpu(), want_graph[k], (name, k))
    for fused in (True, False):
        a = step.render_eval(Ms[0], TE._cam(), bg_d, sky=sky_d, fused=fused, rasterize_mode=AA)
        assert set(a) == set(want_single)
        for k in ("rgb", "accumulation"):
            TE._close(a[k].cpu(), want_single[k], (fused, k))
        TE._close_depth(a["depth"].cpu(), want_single["depth"])


# ---------------------------------------------------------------- LiDAR term, empty view

@pytest.mark.parametrize("fused", [False, True])
def test_lidar_term_takes_the_compensated_opacities(fused):
    import test_gpu_lidar_depth as TL
    from sgn_rast import features, lidar, ops, step
    cam, raw, gt, target = TL._e2e_scene()
    w_img, w_a = (t.to(DEV) for t in step.loss_weights(cam, seed=7))
    P = step.leaf_params(raw)
    ops.clear_binning_cache()
    b0 = ops.binning_stats["binnings"]
    got = step.train_step(P, cam, w_img, w_a, gt=gt, fused=fused, lidar_depth=target, rasterize_mode=AA)
    assert ops.binning_stats["binnings"] == b0 + 1          # one opacity tensor for every pass: one binning
    with torch.no_grad():
        dsum, acc = features.expected_depth(got.xys, got.depths, got.radii, got.conics, got.num_tiles_hit, got.opacities,
                                            cam.height, cam.width, 16, opacity_is_logit=False)
        by_hand = lidar.depth_loss(dsum, acc, target, "l1", None)
    assert torch.equal(got.depth_loss, by_hand)
    Q = step.leaf_params(raw)
    classic = step.train_step(Q, cam, w_img, w_a, gt=gt, fused=fused, lidar_depth=target)
    assert float(got.depth_loss) > 0 and float(got.depth_loss) != float(classic.depth_loss)
    # the term's gradient reaches the covariance through the factor as well: without the term the gradients differ
    R = step.leaf_params(raw)
    step.train_step(R, cam, w_img, w_a, gt=gt, fused=fused, rasterize_mode=AA)
    assert rel_l2(R["log_scales"].grad, P["log_scales"].grad) > 1e-3


@pytest.mark.parametrize("fused", [False, True])
def test_empty_view(fused):
    """A camera that sees nothing: the reference's constant outputs (sgn_splatfacto.py:878-886) in both modes, the leaf
    gradients of the classic mode."""
    from sgn_rast import scenes, step
    cam = scenes.make_camera(64, 48, 64.0, device=DEV)
    raw = scenes.make_gaussians(300, cam, seed=0, z_range=(1.0, 4.0))
    raw["means"][:, 2] = -5.0                                    # everything behind the camera
    raw = {k: v.to(DEV) for k, v in raw.items()}
    w_img, w_a = (t.to(DEV) for t in step.loss_weights(cam))
    outs, grads = {}, {}
    for mode in ("classic", AA):
        P = step.leaf_params(raw)
        outs[mode] = o = step.train_step(P, cam, w_img, w_a, with_depth=True, fused=fused, caller_syncs=True,
                                         rasterize_mode=mode)
        grads[mode] = {k: p.grad for k, p in P.items()}
        torch.cuda.synchronize()
        assert int(o.radii.sum()) == 0 and float(o.loss) == 0.0
        assert o.rgb.shape == (48, 64, 3) and float(o.rgb.abs().max()) == 0.0 and float(o.alpha.abs().max()) == 0.0
    for k in raw:
        a, b = grads["classic"][k], grads[AA][k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert torch.equal(a, b) and float(a.abs().max()) == 0.0, k
    if fused:
        assert float(outs[AA].opacities.abs().max()) == 0.0       # culled rows: c = 0, o = 0

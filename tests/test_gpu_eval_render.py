"""GPU (-m gpu): `sgn_rast.step.render_scene_graph_eval` / `render_eval` on the HIP kernels — the one-call layered form
(`fused=True`) against the six-pass call-site replay (`fused=False`), against the multi-call form of the same fused
front ends (bit for bit), and against the frozen eval-mode run of the reference's own model
(tests/golden/literal_scene_graph_eval.npz)."""
import pytest
import torch

import test_literal_eval_golden as TE
import test_literal_golden as TG

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, FOCAL = 328, 200, 260.0
KEYS = set(TE.KEYS)


def _cam(w=W, h=H, f=FOCAL):
    from sgn_rast import scenes
    return scenes.make_camera(w, h, f, device=DEV)


@pytest.fixture(scope="module")
def graph():
    """Four objects with Fourier dimension 5 in front of a background, a sky image, a non-zero background colour."""
    from sgn_rast import scenes
    cam = scenes.make_camera(W, H, FOCAL)
    models, poses, idft = scenes.make_scene_graph(6000, cam, n_objects=4, object_frac=0.2, fourier_dim=5, seed=3,
                                                  z_range=(1.5, 9.0), object_depth=(3.0, 7.0), object_extent=0.4)
    sky = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(2))
    to = lambda m: {k: v.to(DEV) for k, v in m.items()}
    return [to(m) for m in models], poses.to(DEV), idft.to(DEV), sky.to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _close(got, want, name):
    """Forward tolerance of tests/test_gpu_fused.py::test_scene_graph_replay_fused_vs_dropin_vs_oracle: the fused
    projection / SH differ from the drop-in operators' in the last bits, a pixel at a 1/255 or 1e-4 threshold may flip."""
    err = (got.float() - want.float()).abs()
    assert float(err.mean()) < 2e-5 and float((err > 1e-3).float().mean()) < 5e-3, (name, float(err.mean()))


def _close_depth(got, want):
    derr = (got - want).abs() / want.abs().clamp(min=1)          # as tests/test_gpu_literal_golden.py
    assert float(derr.mean()) < 1e-5, float(derr.mean())


@pytest.mark.parametrize("with_sky", [True, False])
def test_layered_eval_equals_the_six_pass_replay(graph, with_sky):
    from sgn_rast import layers, ops, step
    models, poses, idft, sky, bg = graph
    sky = sky if with_sky else None
    ops.clear_binning_cache()
    calls = layers.stats["calls"]
    one = step.render_scene_graph_eval(models, poses, idft, _cam(), bg, sky=sky, fused=True)
    assert layers.stats["calls"] == calls + 1                    # ONE layered rasterization
    six = step.render_scene_graph_eval(models, poses, idft, _cam(), bg, sky=sky, fused=False)
    multi = step.render_scene_graph_eval(models, poses, idft, _cam(), bg, sky=sky, fused=True, layered=False)
    torch.cuda.synchronize()
    want_keys = KEYS if with_sky else KEYS - {"sky"}
    assert set(one) == set(six) == set(multi) == want_keys
    for k in want_keys:
        assert one[k].shape == six[k].shape == ((H, W, 3) if k in ("rgb", "sky", "background_rgb", "object_rgb")
                                                else (H, W, 1)), k
        assert not one[k].requires_grad
        # the same fused projection / SH through the existing forward, three id-range calls and eager torch: every
        # operation after the SH is shared, so the layered call must return the same bits
        assert torch.equal(one[k], multi[k]), (k, float((one[k] - multi[k]).abs().max()))
        if k == "depth":
            _close_depth(one[k], six[k])
        else:
            _close(one[k], six[k], k)
    for k in ("accumulation", "object_acc", "background_acc", "object_rgb", "background_rgb"):
        assert float(one[k].max()) > 0.2, k
    assert float(one["rgb"].max()) <= 1.0 and float(one["rgb"].min()) >= 0.0


def test_eval_with_an_empty_object_list(graph):
    """No object at the frame — by an empty list and by objects without points (sgn_splatfacto_scene_graph.py:263-267,
    :338-339): one-channel zeros and `object_depth`; the background outputs are the scene's."""
    from sgn_rast import step
    models, poses, idft, sky, bg = graph
    pointless = [models[0]] + [{k: v[:0] for k, v in m.items()} for m in models[1:]]
    for ms, p, w in ((models[:1], poses[:1], idft[:1]), (pointless, poses, idft)):
        one = step.render_scene_graph_eval(ms, p, w, _cam(), bg, sky=sky, fused=True)
        six = step.render_scene_graph_eval(ms, p, w, _cam(), bg, sky=sky, fused=False)
        assert set(one) == set(six) == KEYS | {"object_depth"}
        for k in ("object_acc", "object_rgb", "object_depth"):
            assert one[k].shape == six[k].shape == (H, W, 1) and float(one[k].abs().max()) == 0, k
        assert torch.equal(one["background_acc"], one["accumulation"])
        assert torch.equal(one["background_rgb"], one["rgb"])
        for k in ("rgb", "accumulation", "background_rgb", "background_acc"):
            _close(one[k], six[k], k)
        _close_depth(one["depth"], six["depth"])


def test_eval_with_nothing_visible(graph):
    """Everything behind the camera: the constant outputs of sgn_splatfacto.py:878-886, empty layers."""
    from sgn_rast import step
    models, poses, idft, sky, bg = graph
    flip = torch.tensor([1.0, 1.0, -1.0], device=DEV)
    hidden = [dict(m, means=m["means"] * flip - torch.tensor([0.0, 0.0, 50.0], device=DEV)) for m in models]
    p = poses.clone()
    p[1:, 9:12] = torch.tensor([0.0, 0.0, -80.0], device=DEV)
    for fused in (True, False):
        out = step.render_scene_graph_eval(hidden, p, idft, _cam(), bg, sky=sky, fused=fused)
        assert set(out) == KEYS
        assert torch.equal(out["rgb"], bg.repeat(H, W, 1)) and torch.equal(out["object_rgb"], bg.repeat(H, W, 1))
        assert torch.equal(out["background_rgb"], sky.clamp(0, 1))
        for k in ("accumulation", "depth", "object_acc", "background_acc"):
            assert out[k].shape == (H, W, 1) and float(out[k].abs().max()) == 0, (fused, k)


def _close_golden(got, want, name):
    """Tolerance of tests/test_gpu_literal_golden.py (HIP against the oracle's arithmetic)."""
    err = (got.detach().cpu().float() - want.float()).abs()
    assert float(err.mean()) < 2e-6 and float((err > 1e-4).float().mean()) < 2e-3, (name, float(err.mean()))


@pytest.mark.parametrize("fused", [True, False])
def test_eval_on_hip_matches_the_frozen_literal_eval_run(fused):
    from sgn_rast import ops, step
    G = TE.load()
    cam, models = TG.graph_scene()
    Ms = [{k: v.to(DEV) for k, v in m.items()} for m in models]
    ops.clear_binning_cache()
    out = step.render_scene_graph_eval(Ms, G["poses"].to(DEV), G["idft"].to(DEV), _cam(TG.W, TG.H, TG.FOCAL),
                                       torch.zeros(3, device=DEV), sky=G["sky"].to(DEV), fused=fused)
    torch.cuda.synchronize()
    assert set(out) == KEYS
    for k in TE.KEYS:
        assert tuple(out[k].shape) == tuple(G[k].shape), k
        if k == "depth":
            _close_depth(out[k].cpu(), G[k])
        else:
            _close_golden(out[k], G[k], k)
    # ... and the record without objects at the frame
    want = {k[len("empty_"):]: v for k, v in G.items() if k.startswith("empty_")}
    out = step.render_scene_graph_eval(Ms[:1], G["poses"][:1].to(DEV), G["idft"][:1].to(DEV),
                                       _cam(TG.W, TG.H, TG.FOCAL), torch.zeros(3, device=DEV),
                                       sky=want["sky"].to(DEV), fused=fused)
    assert set(out) == set(want)
    for k, w in want.items():
        assert tuple(out[k].shape) == tuple(w.shape), k
        if k == "depth":
            _close_depth(out[k].cpu(), w)
        else:
            _close_golden(out[k], w, k)


def test_single_model_eval(graph):
    """`render_eval`: the all-layer alone through the existing forward, with the eval semantics."""
    from sgn_rast import step
    models, _poses, _idft, sky, bg = graph
    a = step.render_eval(models[0], _cam(), bg, sky=sky, fused=True)
    b = step.render_eval(models[0], _cam(), bg, sky=sky, fused=False)
    assert set(a) == set(b) == {"rgb", "accumulation", "depth", "sky"}
    for k in ("rgb", "accumulation"):
        _close(a[k], b[k], k)
    _close_depth(a["depth"], b["depth"])
    assert a["accumulation"].shape == (H, W, 1) and a["depth"].shape == (H, W, 1) and float(a["rgb"].max()) <= 1.0
    assert set(step.render_eval(models[0], _cam(), bg, fused=True)) == {"rgb", "accumulation", "depth"}

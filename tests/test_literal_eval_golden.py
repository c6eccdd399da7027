"""CPU: `sgn_rast.step.render_scene_graph_eval(fused=False)` on the oracle ops against the FROZEN eval-mode run of the
reference's own scene-graph model (tests/golden/literal_scene_graph_eval.npz, written by
tests/golden/make_literal_eval.py from the reference checkout).  Needs no checkout; where one exists,
`test_eval_golden_is_current` re-runs the reference and compares.

Tolerance: the one tests/test_literal_golden.py uses for forward outputs — bit equality (`torch.equal`): the replay
hands the same operators the same tensors in the same order."""
import os

import numpy as np
import pytest
import torch

import test_literal_golden as TG

GOLDEN = TG.GOLDEN
KEYS = ("rgb", "accumulation", "depth", "sky", "object_acc", "background_acc", "background_rgb", "object_rgb")


def load():
    z = np.load(os.path.join(GOLDEN, "literal_scene_graph_eval.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _replay(G, models, poses, idft, sky, **kw):
    import oracle_ops
    from sgn_rast import step
    cam, _ = TG.graph_scene()
    return step.render_scene_graph_eval(models, poses, idft, cam, torch.zeros(3), sky=sky, fused=False, ops=oracle_ops,
                                        **kw)


def test_eval_replay_equals_the_frozen_literal_eval_run():
    G = load()
    _, models = TG.graph_scene()
    out = _replay(G, models, G["poses"], G["idft"], G["sky"])
    assert set(out) == set(KEYS)
    for k in KEYS:
        assert out[k].shape == G[k].shape and out[k].dtype == G[k].dtype, (k, out[k].shape, G[k].shape)
        assert torch.equal(out[k], G[k]), (k, float((out[k] - G[k]).abs().max()))
    assert not any(t.requires_grad for t in out.values())
    # the fixture is not blank, and the decomposition is a decomposition: both layers show up in the frame
    assert float(G["object_acc"].max()) > 0.2 and float(G["background_acc"].max()) > 0.2
    assert float(G["object_rgb"].max()) > 0.05 and float(G["rgb"].min()) >= 0 and float(G["rgb"].max()) <= 1


def test_eval_uses_the_full_sh_degree_whatever_the_step():
    """The fixture was frozen at step 0: training mode would evaluate degree 0 there (sgn_splatfacto.py:936-938)."""
    G = load()
    _, models = TG.graph_scene()
    low = _replay(G, models, G["poses"], G["idft"], G["sky"], sh_degree=0)
    assert not torch.equal(low["rgb"], G["rgb"])


def test_eval_replay_with_an_empty_object_list():
    """No object annotated at the frame (sgn_splatfacto_scene_graph.py:263-267): one-channel zeros for the object
    outputs, `object_depth` appears, the background outputs are the scene's."""
    G = load()
    _, models = TG.graph_scene()
    want = {k[len("empty_"):]: v for k, v in G.items() if k.startswith("empty_")}
    assert set(want) == set(KEYS) | {"object_depth"}
    for bg_only in (models[:1], [models[0]] + [{k: v[:0] for k, v in m.items()} for m in models[1:]]):
        n = len(bg_only)
        out = _replay(G, bg_only, G["poses"][:n], G["idft"][:n], want["sky"])
        assert set(out) == set(want)
        for k, w in want.items():
            assert out[k].shape == w.shape, (k, out[k].shape, w.shape)
            assert torch.equal(out[k], w), k
    assert want["object_rgb"].shape == (TG.H, TG.W, 1) and float(want["object_rgb"].abs().max()) == 0
    assert torch.equal(want["background_acc"], want["accumulation"])


def test_eval_replay_with_nothing_visible():
    """Every Gaussian behind the camera: the constant outputs of sgn_splatfacto.py:878-886 and empty layers."""
    G = load()
    _, models = TG.graph_scene()
    hidden = [dict(m, means=m["means"] * torch.tensor([1.0, 1.0, -1.0]) - torch.tensor([0.0, 0.0, 50.0]))
              for m in models]
    poses = G["poses"].clone()
    poses[1:, 9:12] = torch.tensor([0.0, 0.0, -80.0])
    bg = torch.tensor([0.25, 0.5, 0.75])
    import oracle_ops
    from sgn_rast import step
    cam, _ = TG.graph_scene()
    out = step.render_scene_graph_eval(hidden, poses, G["idft"], cam, bg, sky=G["sky"], fused=False, ops=oracle_ops)
    assert set(out) == set(KEYS)
    assert torch.equal(out["rgb"], bg.repeat(TG.H, TG.W, 1))
    for k in ("accumulation", "depth", "object_acc", "background_acc"):
        assert out[k].shape == (TG.H, TG.W, 1) and float(out[k].abs().max()) == 0, k
    assert torch.equal(out["background_rgb"], G["sky"].clamp(0, 1)) and out["object_rgb"].shape == (TG.H, TG.W, 3)
    assert torch.equal(out["object_rgb"], bg.repeat(TG.H, TG.W, 1))


def test_single_model_eval_replay():
    """`render_eval`: the scene-graph replay with the background alone returns the same rgb / accumulation / depth."""
    import oracle_ops
    from sgn_rast import step
    G = load()
    cam, models = TG.graph_scene()
    sky = G["empty_sky"]
    out = step.render_eval(models[0], cam, torch.zeros(3), sky=sky, fused=False, ops=oracle_ops)
    assert set(out) == {"rgb", "accumulation", "depth", "sky"}
    for k in ("rgb", "accumulation", "depth"):
        assert torch.equal(out[k], G["empty_" + k]), k
    plain = step.render_eval(models[0], cam, torch.zeros(3), fused=False, ops=oracle_ops)
    assert set(plain) == {"rgb", "accumulation", "depth"} and float(plain["rgb"].max()) <= 1.0


def test_eval_golden_is_current():
    import refhost
    if not refhost.available():
        pytest.skip("needs the reference checkout")
    if refhost._loaded and "oracle" not in refhost._loaded:
        pytest.skip("the reference modules are bound to another backend in this process")
    import sys
    sys.path.insert(0, GOLDEN)
    import make_literal_eval
    now = make_literal_eval.scene_graph_eval(refhost.load("oracle"))
    G = load()
    assert set(G) == set(now)
    for k in G:
        b = torch.from_numpy(np.asarray(now[k]))
        assert G[k].shape == b.shape and G[k].dtype == b.dtype and torch.equal(G[k], b), k
    assert os.path.getsize(os.path.join(GOLDEN, "literal_scene_graph_eval.npz")) <= os.path.getsize(
        os.path.join(GOLDEN, "literal_scene_graph.npz"))

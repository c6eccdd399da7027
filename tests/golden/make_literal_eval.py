"""Freezes what the REFERENCE's own scene-graph model computes in EVAL mode (`get_outputs_for_camera`: `self.training ==
False` under `torch.no_grad()`), the half of `SplatfactoSceneGraphModel.get_outputs` that `make_literal.py` does not run.

Same scene as `make_literal.py` (`test_reference_literal._graph_scene`), the two model files imported unchanged from the
reference checkout through tests/refhost.py, CPU oracle backend.  Two records go to
tests/golden/literal_scene_graph_eval.npz:

* the annotated frame: all eight outputs — rgb, accumulation, depth, sky, object_acc, background_acc, background_rgb,
  object_rgb — with the model's step set to 0, so that a replay which took the SH degree from the step (degree 0) instead
  of the configured one (sgn_splatfacto.py:937-938) cannot reproduce them;
* `empty_*`: a camera time after the last annotated frame, where the object list is empty
  (sgn_splatfacto_scene_graph.py:263-267: one-channel zeros, and `object_depth` appears).

tests/test_literal_eval_golden.py (CPU, oracle ops) and tests/test_gpu_eval_render.py (HIP) compare
`sgn_rast.step.render_scene_graph_eval` against this file without needing the checkout.

Run from the repo root where the reference checkout exists:  python tests/golden/make_literal_eval.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "street-gaussians-ns_amd"), os.path.join(ROOT, "tests")]

import refhost  # noqa: E402
import test_reference_literal as T  # noqa: E402

f = lambda t: t.detach().cpu().numpy()
FRAME = 1
KEYS = ("rgb", "accumulation", "depth", "sky", "object_acc", "background_acc", "background_rgb", "object_rgb")


def _eval_model(ns):
    cam, models, poses = T._graph_scene()
    model, stamps = refhost.build_scene_graph(ns, models, poses)
    model.eval()
    model.step = 0
    for m in model.all_models.values():
        m.eval()
        m.step = 0
    return cam, models, poses, model, stamps


def _outputs(ns, model, cam, time):
    camera = refhost.nerfstudio_camera(ns, cam, time=float(time))
    with refhost.cpu_as_cuda(), torch.no_grad():                       # base_model.get_outputs_for_camera
        return model.get_outputs(camera)


def scene_graph_eval(ns):
    torch.manual_seed(1234)
    cam, models, poses, model, stamps = _eval_model(ns)
    out = _outputs(ns, model, cam, stamps[FRAME])
    assert set(out) == set(KEYS), sorted(out)
    p_t, idft = refhost.scene_graph_tables(ns, models, poses, FRAME)
    rec = {k: f(out[k]) for k in KEYS}
    rec.update(poses=f(p_t), idft=f(idft), frame=np.int64(FRAME))
    # a time after the last annotated frame: `object_annos[time]` is empty
    late = float(stamps[-1]) + 3e5
    out = _outputs(ns, model, cam, late)
    assert set(out) == set(KEYS) | {"object_depth"}, sorted(out)
    for k in sorted(out):
        rec["empty_" + k] = f(out[k])
    return rec


def main():
    ns = refhost.load("oracle")
    rec = scene_graph_eval(ns)
    path = os.path.join(HERE, "literal_scene_graph_eval.npz")
    np.savez_compressed(path, **rec)
    ref = os.path.getsize(os.path.join(HERE, "literal_scene_graph.npz"))
    print(len(rec), "arrays,", os.path.getsize(path) // 1024, "KiB (literal_scene_graph.npz:", ref // 1024, "KiB)")
    assert os.path.getsize(path) <= ref


if __name__ == "__main__":
    main()

"""Evaluation render of the scene graph at the benchmark's scene-graph shape (1 M Gaussians, 8 objects, 1920x1280, sky
on): all eight eval outputs of `SplatfactoSceneGraphModel.get_outputs` per image, four ways on the same inputs:

  a  six passes     step.render_scene_graph_eval(fused=False)                the call-site replay on the drop-in operators
  b  multi-call     step.render_scene_graph_eval(fused=True, layered=False)  what the training-side fused API allows: main
                                                                             pass with groups + depth channel, two id_range
                                                                             colour passes, torch post-processing
  c  layered        step.render_scene_graph_eval(fused=True)                 one layered rasterization + one finishing launch,
                                                                             the objects layer on its own compacted list
  c' layered/shared the same with layers.tail_own_list = False               the objects layer rides the shared list

One process.  Every variant is warmed up, SETTLE untimed images run in front (bench.py --settle: a device that idled
through the set-up runs its first chunk slow), then the variants are timed in alternation — ROUNDS chunks each, device
events around each chunk, a chunk long enough to run for >= 0.3 s — and the median per variant and the spread across the
chunks are printed, with one JSON line at the end.  After the timed part the library's own event spans give the layered
forward's kernel time (raster_fwd slot, one launch per image).  Run it under its own time limit, e.g.
    timeout -k 10 500 python profiles/microbench/eval_render_timing.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "street-gaussians-ns_amd"))
from sgn_rast import _lib as L, layers, ops, scenes, sky as sky_mod, step  # noqa: E402

ROUNDS, WARMUP, SETTLE = 7, 4, 20
ITERS = {"a": 12, "b": 60, "c": 60, "c_shared": 60}

assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
dev = torch.device("cuda", 0)
L.reset_options()
cam, raw = scenes.make_scene("metric")
models, poses, idft = scenes.make_scene_graph(raw["means"].shape[0], cam, n_objects=8, object_frac=0.1)
models = [{k: v.to(dev) for k, v in m.items()} for m in models]
poses, idft = poses.to(dev), idft.to(dev)
cam_d = scenes.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat.to(dev), cam.cam_pos.to(dev))
H, W = cam.height, cam.width
base = torch.rand(6, 64, 64, 3, generator=torch.Generator().manual_seed(1)).to(dev)
sky_img = sky_mod.sky_color(base, H, W, cam.fx, cam.fy, cam.cx, cam.cy, torch.eye(4, device=dev)[:3], None).detach()
bg = torch.zeros(3, device=dev)


def run(name):
    layers.tail_own_list = name != "c_shared"
    try:
        if name == "a":
            return step.render_scene_graph_eval(models, poses, idft, cam_d, bg, sky=sky_img, fused=False)
        return step.render_scene_graph_eval(models, poses, idft, cam_d, bg, sky=sky_img, fused=True,
                                            layered=name != "b")
    finally:
        layers.tail_own_list = True


def chunk_ms(name):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS[name]):
        run(name)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ITERS[name]


VARIANTS = ["a", "b", "c", "c_shared"]
outs = {}
for name in VARIANTS:
    for _ in range(WARMUP):
        outs[name] = run(name)
torch.cuda.synchronize()
# same inputs, same answer, before anything is timed: b, c and c' return the same bits; a differs by the fused front ends
for k in outs["c"]:
    assert torch.equal(outs["c"][k], outs["b"][k]) and torch.equal(outs["c"][k], outs["c_shared"][k]), k
err_a = float((outs["c"]["rgb"] - outs["a"]["rgb"]).abs().mean())
assert err_a < 2e-5, err_a
for _ in range(SETTLE):
    run("c")
times = {name: [] for name in VARIANTS}
for _ in range(ROUNDS):
    for name in VARIANTS:
        times[name].append(chunk_ms(name))

result = {"shape": {"gaussians": sum(m["means"].shape[0] for m in models), "objects": len(models) - 1, "size": [H, W]},
          "rounds": ROUNDS, "images_per_chunk": ITERS, "settle": SETTLE, "rgb_mean_abs_a_vs_c": err_a}
for name in VARIANTS:
    t = times[name]
    med = statistics.median(t)
    result[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_pct": 100.0 * (max(t) - min(t)) / med}
    print(f"{name:9s} {W}x{H}: median {med:.3f} ms/image  (min {min(t):.3f}, max {max(t):.3f}, "
          f"spread {result[name]['spread_pct']:.1f} % over {ROUNDS} chunks of {ITERS[name]})")
for name in ("a", "b", "c_shared"):
    result[f"{name}_over_c"] = result[name]["median_ms"] / result["c"]["median_ms"]

# kernel time of the layered forward from the library's event spans (it is the only raster_fwd launch of variant c)
for name in ("c", "c_shared"):
    L.timing_enable(True)
    for _ in range(20):
        run(name)
    torch.cuda.synchronize()
    rep = L.timing_report()
    L.timing_enable(False)
    n_launch, ms = rep["raster_fwd"]
    result[f"layered_kernel_ms_{name}"] = ms / max(n_launch, 1)
    result[f"layered_kernel_launches_{name}"] = n_launch
    print(f"{name:9s} layered forward kernel: {ms / max(n_launch, 1):.3f} ms per launch ({n_launch} launches)")
print(json.dumps(result))

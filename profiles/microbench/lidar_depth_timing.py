"""LiDAR depth supervision at 1920x1280, three measurements in one process (device events around blocks of calls):

  target   lidar.splat_depth of ONE 180 k-point sweep: begin + splat + finish (radius 2)
  loss     lidar.depth_loss forward + backward against the eager torch chain on the same inputs
           (divide, compare, boolean index — a host sync —, abs, mean), both kinds
  step     step.train_step(fused=True, gt=...) at the benchmark scene ("metric": 1 M Gaussians) with and without
           lidar_depth, in alternation
  fit      (illustration, not a timing) 50 Adam steps with the depth term on the 128x128 test scene: depth_metrics before
           and after

Every variant is warmed up; variants that are compared are timed in alternation over ROUNDS rounds, and the median and
the spread across the rounds (max - min as a percentage of the median) are printed, with one JSON line at the end.  Run
it under its own time limit, e.g.  timeout -k 10 500 python profiles/microbench/lidar_depth_timing.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "street-gaussians-ns_amd"))
from sgn_rast import features, lidar, scenes, seed, step  # noqa: E402

H, W, FOCAL = 1280, 1920, 2000.0
N_POINTS = 180_000
ROUNDS = 7
QUICK = "--quick" in sys.argv                      # a rehearsal at a fraction of the iterations
SCALE = 20 if QUICK else 1

assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(variants, iters, warmup):
    """{name: stats} of variants timed in alternation."""
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            times[name].append(timed(fn, iters))
    out = {}
    for name, _ in variants:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_pct": 100.0 * (max(t) - min(t)) / med}
        print(f"{name:28s} median {med:.4f} ms  (min {min(t):.4f}, max {max(t):.4f}, spread "
              f"{out[name]['spread_pct']:.1f} % over {ROUNDS} rounds of {iters})", flush=True)
    return out


result = {"size": [H, W], "rounds": ROUNDS, "quick": QUICK}

# ---- target: a street-like sweep in the camera's own frame (identity poses): the LiDAR covers the image's lower band
z = 2.0 + 73.0 * torch.rand(N_POINTS, generator=g) ** 2
pts = torch.stack([(torch.rand(N_POINTS, generator=g) * 1.1 - 0.55) * z,
                   (torch.rand(N_POINTS, generator=g) * 0.45 - 0.12) * z, z], dim=1).to(dev)
cam_t = seed.SeedCamera(torch.eye(4), FOCAL, FOCAL, W / 2, H / 2, W, H)
sweep = (pts, torch.eye(4))
target = lidar.splat_depth(sweep, cam_t, min_z=-1e30)
result["target_pixels"] = int((target > 0).sum())
result["target_pixels_unfiltered"] = int((lidar.splat_depth(sweep, cam_t, min_z=-1e30, radius=0) > 0).sum())
print(f"target: {N_POINTS} points -> {result['target_pixels_unfiltered']} pixels with a return, "
      f"{result['target_pixels']} after the occlusion filter", flush=True)
result["target"] = compare([("splat_depth 180k points", lambda: lidar.splat_depth(sweep, cam_t, min_z=-1e30))],
                           2000 // SCALE, 50)

# ---- loss: the rendered pair of a scene whose depth is near the target's where there is one
alpha = (0.05 + 0.95 * torch.rand(H, W, generator=g)).to(dev)
alpha[torch.rand(H, W, generator=g).to(dev) < 0.05] = 0.0                       # sky: nothing rendered
depth = torch.where(target > 0, target, torch.full_like(target, 20.0)) * (1 + 0.1 * torch.randn(H, W, generator=g).to(dev))
dsum0 = (depth.clamp(min=0.5) * alpha).contiguous()
dsum = dsum0.clone().requires_grad_(True)
acc = alpha.clone().requires_grad_(True)


def eager(kind):
    valid = (target > 0) & (acc > 1e-3) & (dsum > 0)
    D, zc = dsum[valid] / acc[valid], target[valid]
    return ((D - zc) if kind == "l1" else (1 / D - 1 / zc)).abs().mean()


def run(fn):
    def once():
        dsum.grad = None
        acc.grad = None
        fn().backward()
    return once


for kind in ("l1", "inverse"):
    run(lambda: eager(kind))()
    ref = (float(eager(kind).detach()), dsum.grad.clone(), acc.grad.clone())
    run(lambda: lidar.depth_loss(dsum, acc, target, kind))()
    got = float(lidar.depth_loss(dsum, acc, target, kind).detach())
    rel = [float((a - b).norm() / b.norm()) for a, b in ((dsum.grad, ref[1]), (acc.grad, ref[2]))]
    assert abs(got - ref[0]) <= 1e-5 * ref[0] and max(rel) < 1e-5, (got, ref[0], rel)     # same inputs, same answer
    result[f"loss_{kind}"] = compare([(f"eager chain {kind}", run(lambda: eager(kind))),
                                      (f"depth_loss {kind}", run(lambda: lidar.depth_loss(dsum, acc, target, kind)))],
                                     1000 // SCALE, 20)
    result[f"loss_{kind}"]["grad_rel_l2_vs_eager"] = rel
result["metrics_example"] = lidar.depth_metrics(dsum, acc, target)

# ---- step: the benchmark scene, fused path, photometric loss, with and without the depth term
cam, raw = scenes.make_scene("metric", seed=0, device=dev, n_override=100_000 if QUICK else 0)
P = step.leaf_params(raw)
w_img, w_a = (t.to(dev) for t in step.loss_weights(cam, seed=7))
gt = torch.rand(cam.height, cam.width, 3, generator=g).to(dev)
sub = torch.randperm(raw["means"].shape[0], generator=g)[:N_POINTS].to(dev)
pos = cam.cam_pos.to(dev)
surf = (pos + 1.05 * (raw["means"][sub] - pos)).contiguous()
cam_s = seed.SeedCamera(cam.viewmat.cpu(), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
target_s = lidar.splat_depth((surf, torch.eye(4)), cam_s, min_z=-1e30)
result["step_target_pixels"] = int((target_s > 0).sum())
result["step"] = compare([("train_step", lambda: step.train_step(P, cam, w_img, w_a, gt=gt, fused=True)),
                          ("train_step + lidar_depth", lambda: step.train_step(P, cam, w_img, w_a, gt=gt, fused=True,
                                                                               lidar_depth=target_s))],
                         40 // min(SCALE, 4), 5)
del P, raw

# ---- fit: the end-to-end test scene, 50 Adam steps with the depth term
cam, raw = scenes.make_scene("c1", seed=2, n_override=500, device=dev)
P = step.leaf_params(raw)
w_img, w_a = (t.to(dev) for t in step.loss_weights(cam, seed=7))
gt = torch.rand(cam.height, cam.width, 3, generator=torch.Generator().manual_seed(4)).to(dev)
pos = cam.cam_pos.to(dev)
surf = (pos + 1.05 * (raw["means"] - pos)).contiguous()
cam_s = seed.SeedCamera(cam.viewmat.cpu(), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
target_s = lidar.splat_depth((surf, torch.eye(4)), cam_s, min_z=-1e30)


def metrics_now():
    with torch.no_grad():
        out = step.render_fused(P, cam)
        pair = features.expected_depth(out.xys, out.depths, out.radii, out.conics, out.num_tiles_hit,
                                       P["opacity_logits"], cam.height, cam.width, 16, opacity_is_logit=True)
        return lidar.depth_metrics(*pair, target_s)


before = metrics_now()
opt = torch.optim.Adam([P["means"]], lr=2e-3)
for _ in range(50):
    step.train_step(P, cam, w_img, w_a, gt=gt, fused=True, lidar_depth=target_s, depth_loss_mult=1.0)
    opt.step()
result["fit"] = {"before": before, "after_50_adam_steps": metrics_now()}
print("fit:", json.dumps(result["fit"]), flush=True)
print(json.dumps(result))

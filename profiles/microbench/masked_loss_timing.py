"""Photometric loss under a pixel mask at 1920x1280x3, forward + backward, three variants on the same inputs:

  torch+fused   photometric_loss(torch.clamp(rgb, max=1) * m, gt * m, 0.2)          what a caller had to write before
  fused masked  photometric_loss(rgb, gt, 0.2, clamp_max=1.0, mask=m)               sgn_l1_ssim_masked_fwd/bwd
  fused no mask photometric_loss(rgb, gt, 0.2, clamp_max=1.0)                       sgn_l1_ssim_fwd/bwd

One process: every variant is warmed up, then the three are timed in alternation (ROUNDS rounds of ITERS steps each,
device events around each block of ITERS steps), and the median per variant and the spread across the rounds
(min .. max, and max - min as a percentage of the median) are printed, with one JSON line at the end.  Run it under
its own time limit, e.g.  timeout -k 10 300 python profiles/microbench/masked_loss_timing.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "street-gaussians-ns_amd"))
from sgn_rast import loss  # noqa: E402

H, W = 1280, 1920
ROUNDS, ITERS, WARMUP = 9, 2500, 50            # 2500 steps of ~0.2 ms or more: each timed block runs >= 0.5 s

assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
gt = torch.rand(H, W, 3, generator=g).to(dev)
pred0 = (gt + 0.15 * torch.randn(H, W, 3, generator=g).to(dev)).clamp(0, 1.2)
mask = torch.ones(H, W, dtype=torch.bool)
mask[H - H // 3:, :] = False                                           # the ego vehicle's hood: the bottom third
mask &= torch.rand(H, W, generator=g) < 0.98                           # plus scattered invalid pixels
mask = mask.to(dev)
mask_f = mask[..., None].float()                                       # what `gt_img *= mask` broadcasts


def composition(p):
    return loss.photometric_loss(torch.clamp(p, max=1.0) * mask_f, gt * mask_f, 0.2)


def fused_masked(p):
    return loss.photometric_loss(p, gt, 0.2, clamp_max=1.0, mask=mask)


def fused_unmasked(p):
    return loss.photometric_loss(p, gt, 0.2, clamp_max=1.0)


VARIANTS = [("torch+fused", composition), ("fused masked", fused_masked), ("fused no mask", fused_unmasked)]
p = pred0.clone().requires_grad_(True)


def steps(fn, n):
    for _ in range(n):
        p.grad = None
        fn(p).backward()


def block_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    steps(fn, ITERS)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ITERS


for _, fn in VARIANTS:
    steps(fn, WARMUP)
torch.cuda.synchronize()
# same inputs, same answer: the composition and the fused masked call agree before either is timed
steps(composition, 1)
g_ref = p.grad.clone()
steps(fused_masked, 1)
rel = float((p.grad - g_ref).norm() / g_ref.norm())
assert rel < 2e-5, rel

times = {name: [] for name, _ in VARIANTS}
for _ in range(ROUNDS):
    for name, fn in VARIANTS:
        times[name].append(block_ms(fn))

result = {"size": [H, W], "rounds": ROUNDS, "iters_per_block": ITERS, "kept_fraction": float(mask.float().mean()),
          "grad_rel_l2_masked_vs_composition": rel}
for name, _ in VARIANTS:
    t = times[name]
    med = statistics.median(t)
    result[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_pct": 100.0 * (max(t) - min(t)) / med}
    print(f"{name:14s} fwd+bwd {W}x{H}x3: median {med:.4f} ms  (min {min(t):.4f}, max {max(t):.4f}, "
          f"spread {result[name]['spread_pct']:.1f} % over {ROUNDS} rounds of {ITERS})")
print(json.dumps(result))

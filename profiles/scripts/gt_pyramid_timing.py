"""What one pyramid level of a batch costs on the device: 1280x1920 uint8 image with a bool mask and a uint8 semantic
map, d = 2, 4, 8, two arms in one process:

  kernel   ``sgn_rast.pyramid.downscale(batch, d)``: one launch of gt_downscale_kernel (csrc/gt_pyramid.hip)
  torch    what a user without it writes on the device: ``image.float() / 255``, a permute, ``F.interpolate`` bilinear
           (``align_corners=False, antialias=False``), back to a contiguous HWC image for the loss, and ``F.interpolate``
           nearest on the mask and on the semantic map (both as uint8: the cheapest form torch has)

Both arms are warmed up, then timed in alternation: ROUNDS rounds of CHUNK calls each between two device events on the
compute stream, so a figure is the time per call as the training loop's stream sees it, the arm's own launch gaps
included.  Per arm and d: the median over the chunks and their spread; the bytes the kernel must touch (per output pixel
twelve tap bytes and two nearest bytes read, twelve float bytes and two map bytes written) over that time; one JSON
line at the end, ``--out FILE`` also writes it there.

``--trace``: no timing; WARMUP + TRACE_CALLS calls of each arm per d, for a separate
``rocprofv3 --kernel-trace --stats -- python profiles/scripts/gt_pyramid_timing.py --trace`` run, whose per-kernel
durations are the kernel times proper.

Run it under its own time limit, e.g.  timeout -k 10 300 python profiles/scripts/gt_pyramid_timing.py
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "street-gaussians-ns_amd"))
from sgn_rast import pyramid  # noqa: E402

H, W, DS = 1280, 1920, (2, 4, 8)
ROUNDS, CHUNK, WARMUP, TRACE_CALLS = 9, 400, 50, 100

ap = argparse.ArgumentParser()
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
image = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
mask = (torch.rand(H, W, generator=g) < 0.7).to(dev)
semantic = torch.randint(0, 20, (H, W), dtype=torch.uint8, generator=g).to(dev)
mask8 = mask.view(torch.uint8)


def arm_kernel(d):
    return pyramid.downscale((image, mask, semantic), d)


def arm_torch(d):
    size = pyramid.level_size(H, W, d)
    x = (image.float() / 255).permute(2, 0, 1)[None]
    img = F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).contiguous()
    m = F.interpolate(mask8[None, None], size=size, mode="nearest")[0, 0].view(torch.bool)
    s = F.interpolate(semantic[None, None], size=size, mode="nearest")[0, 0]
    return pyramid.Level(img, m, s)


ARMS = [("kernel", arm_kernel), ("torch", arm_torch)]

for d in DS:                                     # same level from both arms, before anything is timed
    a, b = arm_kernel(d), arm_torch(d)
    assert a.image.shape == b.image.shape and float((a.image - b.image).abs().max()) <= 1e-5, d
    assert torch.equal(a.mask, b.mask) and torch.equal(a.semantic, b.semantic), d

if args.trace:
    for d in DS:
        for _, fn in ARMS:
            for _ in range(WARMUP + TRACE_CALLS):
                fn(d)
    torch.cuda.synchronize()
    print(f"trace run: {WARMUP + TRACE_CALLS} calls of each arm at d = {DS}")
    sys.exit(0)

for d in DS:
    for _, fn in ARMS:
        for _ in range(WARMUP):
            fn(d)
torch.cuda.synchronize()

result = {"size": [H, W], "rounds": ROUNDS, "calls_per_chunk": CHUNK}
for d in DS:
    oh, ow = pyramid.level_size(H, W, d)
    must_touch = oh * ow * (12 + 2 + 12 + 2)
    times = {name: [] for name, _ in ARMS}
    for _ in range(ROUNDS):
        for name, fn in ARMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(CHUNK):
                fn(d)
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / CHUNK)          # microseconds per call
    row = {"level": [oh, ow], "bytes_must_touch": must_touch}
    for name, _ in ARMS:
        t = times[name]
        med = statistics.median(t)
        row[name] = {"median_us": med, "min_us": min(t), "max_us": max(t), "spread_pct": 100.0 * (max(t) - min(t)) / med,
                     "chunks_us": t}
        print(f"d={d} {name:6s} {H}x{W} -> {oh}x{ow}: median {med:.2f} us/call  (min {min(t):.2f}, max {max(t):.2f}, "
              f"spread {row[name]['spread_pct']:.1f} % over {ROUNDS} chunks of {CHUNK} calls)")
    row["kernel"]["GB_per_s_of_must_touch"] = must_touch / (row["kernel"]["median_us"] * 1e-6) / 1e9
    row["torch_over_kernel"] = row["torch"]["median_us"] / row["kernel"]["median_us"]
    result[f"d{d}"] = row
line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

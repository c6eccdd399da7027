"""What getting the ground truth to the loss costs per training step: 1 M Gaussians at 1920x1280 (the "metric" scene),
``step.train_step(fused=True, gt=...)``, three arms that differ only in where the ground truth comes from, cycling over
N_IMAGES distinct images:

  resident f32   float32 [H,W,3] already on the device                         the benchmark's assumption, the floor
  f32 .to()      a pinned float32 image, ``.to(device)`` on the compute stream   the reference's next_train
                 in front of every step (29.5 MB)                                (data/sgn_datamanager.py:277-293)
  feed u8        ``sgn_rast.ImageFeed``: pinned uint8, prefetched one step        sgn_l1_ssim_gt8_fwd/bwd read the bytes
                 ahead on a side stream (7.4 MB)

One process: every arm is warmed up, then the three are timed in alternation, ROUNDS rounds of CHUNK steps each, a host
clock around each chunk between two device synchronisations (the copies of the second arm block the host, so device
events on one stream would not see them).  Per arm: the median over the chunks and their spread; one JSON line at the
end.  ``--out FILE`` also writes the JSON there.

``--trace``: no timing; WARMUP + TRACE_STEPS steps of the first and the third arm only, for a separate
``rocprofv3 --kernel-trace --stats -- python profiles/scripts/image_feed_timing.py --trace`` run: the loss kernels with
float and with byte ground truth are different instantiations and come out under their own names.

Run it under its own time limit, e.g.  timeout -k 10 300 python profiles/scripts/image_feed_timing.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "street-gaussians-ns_amd"))
from sgn_rast import ImageFeed, scenes, step  # noqa: E402

N_IMAGES, ROUNDS, CHUNK, WARMUP, TRACE_STEPS = 8, 7, 150, 30, 40      # 7 x 150 = 1050 timed steps per arm

ap = argparse.ArgumentParser()
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
dev = torch.device("cuda", 0)
cam, raw = scenes.make_scene("metric", seed=0, device=dev)
H, W = cam.height, cam.width
P = step.leaf_params(raw)
w_img, w_a = (t.to(dev) for t in step.loss_weights(cam, seed=7))

g = torch.Generator().manual_seed(0)
bytes_cpu = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) for _ in range(N_IMAGES)]
float_pinned = [(b.float() / 255.0).pin_memory() for b in bytes_cpu]
float_resident = [f.to(dev) for f in float_pinned]
feed = ImageFeed(bytes_cpu, device=dev, cache="pinned", slots=2)
feed.open()


def run(gt):
    return step.train_step(P, cam, w_img, w_a, fused=True, gt=gt)


def arm_resident(n, s0):
    for s in range(s0, s0 + n):
        run(float_resident[s % N_IMAGES])


def arm_to_device(n, s0):
    for s in range(s0, s0 + n):
        run(float_pinned[s % N_IMAGES].to(dev))


def arm_feed(n, s0):
    feed.prefetch(s0 % N_IMAGES)
    for s in range(s0, s0 + n):
        b = feed.get(s % N_IMAGES)
        feed.prefetch((s + 1) % N_IMAGES)
        run(b.image)


ARMS = [("resident f32", arm_resident), ("f32 .to()", arm_to_device), ("feed u8", arm_feed)]

# same images, same answer, before anything is timed
la = float(run(float_resident[3]).loss)
lb = float(run(float_pinned[3].to(dev)).loss)
lc = float(run(feed.get(3).image).loss)
assert la == lb == lc, (la, lb, lc)

if args.trace:
    for _, fn in (ARMS[0], ARMS[2]):
        fn(WARMUP + TRACE_STEPS, 0)
    torch.cuda.synchronize()
    print(f"trace run: {WARMUP + TRACE_STEPS} steps each of 'resident f32' and 'feed u8'")
    sys.exit(0)

for _, fn in ARMS:
    fn(WARMUP, 0)
torch.cuda.synchronize()

times = {name: [] for name, _ in ARMS}
for r in range(ROUNDS):
    for name, fn in ARMS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(CHUNK, r * CHUNK)
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / CHUNK)

result = {"scene": "metric", "gaussians": int(raw["means"].shape[0]), "size": [H, W], "images": N_IMAGES,
          "rounds": ROUNDS, "steps_per_chunk": CHUNK, "loss_of_image_3": la,
          "bytes_per_step": {"resident f32": 0, "f32 .to()": H * W * 3 * 4, "feed u8": H * W * 3}}
for name, _ in ARMS:
    t = times[name]
    med = statistics.median(t)
    result[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_pct": 100.0 * (max(t) - min(t)) / med,
                    "chunks_ms": t}
    print(f"{name:13s} train_step(fused) {W}x{H}: median {med:.4f} ms/step  (min {min(t):.4f}, max {max(t):.4f}, "
          f"spread {result[name]['spread_pct']:.1f} % over {ROUNDS} chunks of {CHUNK} steps)")
line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

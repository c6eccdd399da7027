"""What getting an eval frame's outputs to a writer costs per frame: the benchmark's scene-graph shape (1 M Gaussians, 8
objects, 1920x1280, sky on), the eight outputs of ``step.render_scene_graph_eval(fused=True)`` rendered fresh every frame
plus a ground-truth panel, three arms that differ only in how the nine panels become ``uint8`` on the host:

  a  reference   per panel the torch colour-map expressions of nerfstudio's apply_colormap / apply_depth_colormap on the
                 device, ``.cpu().numpy()`` as float32 on the compute stream, then the writers' numpy quantiser
                 ``(clip(a, 0, 1) * 255 + 0.5).astype(uint8)``                         (scripts/render.py:159-273)
  b  pack        ``frames.pack`` (one launch) and a synchronous ``.cpu()`` of the canvas
  c  sink        ``frames.FrameSink`` with a no-op ``on_frame``: pack, then the copy to pinned memory on a side stream
                 behind the next frame's render

One process: every arm is warmed up, then the three are timed in alternation, ROUNDS rounds of a chunk each, a host clock
around each chunk between two device synchronisations (arm c's chunk ends with ``drain()``).  Per arm: the median over
the chunks and their spread; the render alone (no panels leave the device) as the floor; bytes across PCIe per frame from
the shapes; one JSON line at the end.  ``--out FILE`` also writes the JSON there.

``--trace``: no timing; WARMUP + TRACE_FRAMES frames of arm c only, for a separate
``rocprofv3 --kernel-trace --stats -- python profiles/scripts/frame_sink_timing.py --trace`` run: the pack kernel comes
out as ``frames_pack_kernel``.

Run it under its own time limit, e.g.  timeout -k 10 400 python profiles/scripts/frame_sink_timing.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "street-gaussians-ns_amd"))
from sgn_rast import _lib as L, frames, scenes, sky as sky_mod, step  # noqa: E402

ROUNDS, WARMUP, TRACE_FRAMES = 5, 3, 40
FRAMES = {"render": 60, "a": 3, "b": 30, "c": 60}        # frames per chunk
NEAR, FAR = 0.5, 60.0                                   # the render script's depth planes for this scene

ap = argparse.ArgumentParser()
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

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
gt_bytes = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
gt_float = gt_bytes.float() / 255.0                      # what the reference's batch holds

try:                                                    # the colour table: turbo where matplotlib is, seeded random otherwise
    import matplotlib
    table_f = torch.tensor(matplotlib.colormaps["turbo"].colors)
except ImportError:
    table_f = torch.rand(256, 3, generator=torch.Generator().manual_seed(5))
table_dev = table_f.to(dev)
lut = frames.byte_lut(table_f).to(dev)

SCALARS = {"depth": (NEAR, FAR), "accumulation": (0.0, 1.0), "object_acc": (0.0, 1.0), "background_acc": (0.0, 1.0)}
ORDER = ["gt", "rgb", "depth", "accumulation", "sky", "object_acc", "background_acc", "background_rgb", "object_rgb"]
PANELS = [frames.Panel(k, *SCALARS[k], lut=lut) if k in SCALARS else frames.Panel(k) for k in ORDER]


def render():
    return step.render_scene_graph_eval(models, poses, idft, cam_d, bg, sky=sky_img, fused=True)


def reference_panel(name, image):
    """render.py's treatment of one output, down to the writer's bytes."""
    if image.shape[-1] != 3:
        if name == "depth":
            image = torch.clip((image - NEAR) / (FAR - NEAR + 1e-10), 0, 1)
        image = torch.clip(image * (1.0 - 0.0) + 0.0, 0, 1)
        image = torch.nan_to_num(image, 0)
        image = table_dev[(image * 255).long()[..., 0]]
    a = image.cpu().numpy()
    return (np.clip(a, 0, 1) * 255 + 0.5).astype(np.uint8)


def arm_render(n):
    for _ in range(n):
        render()


def arm_a(n):
    last = None
    for _ in range(n):
        out = dict(render(), gt=gt_float)
        last = {k: reference_panel(k, out[k]) for k in ORDER}
    return last


def arm_b(n):
    last = None
    for _ in range(n):
        canvas, _views = frames.pack(dict(render(), gt=gt_bytes), PANELS)
        last = canvas.cpu()
    return last


delivered = [0]


def _count(tag, canvas):
    delivered[0] += 1


sink = frames.FrameSink(PANELS, H, W, slots=2, on_frame=_count, device=dev)
sink.open()


def arm_c(n):
    for i in range(n):
        sink.submit(dict(render(), gt=gt_bytes), tag=i)
    sink.drain()


ARMS = [("render", arm_render), ("a", arm_a), ("b", arm_b), ("c", arm_c)]

# same frame, same bytes, before anything is timed.  The depth panel is held to a fraction, not to equality: arm a
# divides by the plane distance in eager torch on the device, which may multiply by a reciprocal where the kernel
# divides (IEEE), so a pixel that sits on an index boundary can take the neighbouring table row.
ref = arm_a(1)
can = arm_b(1).numpy()
depth_differs = 0.0
for i, k in enumerate(ORDER):
    if k == "depth":
        depth_differs = float((can[i * H:(i + 1) * H] != ref[k]).any(axis=-1).mean())
        assert depth_differs < 1e-3, depth_differs
    else:
        assert np.array_equal(can[i * H:(i + 1) * H], ref[k]), k
kept = []
check = frames.FrameSink(PANELS, H, W, slots=2, on_frame=lambda tag, c: kept.append(c.copy()), device=dev)
check.submit(dict(render(), gt=gt_bytes))
check.close()
assert np.array_equal(kept[0], can)
del check, kept, ref, can

if args.trace:
    arm_c(WARMUP + TRACE_FRAMES)
    torch.cuda.synchronize()
    print(f"trace run: {WARMUP + TRACE_FRAMES} frames of arm c")
    sys.exit(0)

for _, fn in ARMS:
    fn(WARMUP)
torch.cuda.synchronize()

times = {name: [] for name, _ in ARMS}
for r in range(ROUNDS):
    for name, fn in ARMS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(FRAMES[name])
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / FRAMES[name])

n_float = len(ORDER) * H * W * 3 * 4                     # arm a moves every panel as float32 [H,W,3]
result = {"shape": {"gaussians": sum(m["means"].shape[0] for m in models), "objects": len(models) - 1, "size": [H, W]},
          "panels": ORDER, "depth_pixels_differing_from_arm_a": depth_differs, "rounds": ROUNDS, "frames_per_chunk": FRAMES, "frames_delivered_by_the_sink": delivered[0],
          "bytes_per_frame": {"render": 0, "a": n_float, "b": len(ORDER) * H * W * 3, "c": len(ORDER) * H * W * 3}}
for name, _ in ARMS:
    t = times[name]
    med = statistics.median(t)
    result[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_pct": 100.0 * (max(t) - min(t)) / med,
                    "chunks_ms": t}
    print(f"{name:7s} {W}x{H}, {len(ORDER)} panels: median {med:.3f} ms/frame  (min {min(t):.3f}, max {max(t):.3f}, "
          f"spread {result[name]['spread_pct']:.1f} % over {ROUNDS} chunks of {FRAMES[name]} frames)")
line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

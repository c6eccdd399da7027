"""Pose-gradient cost on the MI355X (device-event timing, alternating old and new entries after warm-up), at 1 M
Gaussians, 8 objects, 1920x1280 (scenes.make_scene_graph):

- the projection backward alone: sgn_project_bwd_fused against sgn_project_bwd_fused_pose (its POSE kernel plus the
  per-object sum);
- one fused scene-graph train step (render_scene_graph(fused=True), loss, backward) with the pose table from
  poses.ObjectPoses("SO3xR3").table() requiring grad, against the same step with a constant table.

Prints one JSON line.

    python profiles/scripts/pose_grad_timing.py [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "street-gaussians-ns_amd"))

import torch  # noqa: E402

from sgn_rast import _lib as L  # noqa: E402
from sgn_rast import fused, poses, scenes, step  # noqa: E402


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = scenes.make_camera(1920, 1280, 2000.0)
    models, table0, idft = scenes.make_scene_graph(1_000_000, cam, n_objects=8, device=dev)
    cam.viewmat, cam.cam_pos = cam.viewmat.to(dev), cam.cam_pos.to(dev)
    counts = [m["means"].shape[0] for m in models]
    n, m = sum(counts), len(counts)
    ids = fused.object_ids_for(counts, dev)
    cat = lambda k: torch.cat([mm[k] for mm in models]).contiguous()
    means, ls, q = cat("means"), cat("log_scales"), cat("quats")
    vm = cam.viewmat[:3, :].contiguous().reshape(-1)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    cov3d, xys, depths = torch.empty(n, 6, **f32), torch.empty(n, 2, **f32), torch.empty(n, **f32)
    radii, conics, comp, nth = torch.empty(n, **i32), torch.empty(n, 3, **f32), torch.empty(n, **f32), torch.empty(n, **i32)
    lib = L.load()
    P = L.ptr
    L.check(lib.sgn_project_fwd_fused(n, P(means), P(ls), 1.0, P(q), P(ids), P(table0), P(vm), cam.fx, cam.fy, cam.cx,
                                      cam.cy, cam.height, cam.width, 16, 0.01, P(cov3d), P(xys), P(depths), P(radii),
                                      P(conics), P(comp), P(nth), 0, L.stream_ptr()), "fwd")
    g = torch.Generator().manual_seed(0)
    v_xy, v_d, v_c = (torch.randn(n, 2, generator=g).to(dev), torch.randn(n, generator=g).to(dev),
                      torch.randn(n, 3, generator=g).to(dev))
    v_m, v_s, v_q = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32), torch.empty(n, 4, **f32)
    offs = fused.object_offsets(ids, m)
    ws = torch.empty(lib.sgn_project_pose_workspace_bytes(n, m), dtype=torch.uint8, device=dev)
    v_p = torch.empty(m, 16, **f32)
    common = lambda: (n, P(means), P(ls), 1.0, P(q), P(ids), P(table0), P(vm), cam.fx, cam.fy, P(cov3d), P(radii),
                      P(conics), P(comp), P(v_xy), P(v_d), P(v_c), None, P(v_m), P(v_s), P(v_q), 0, cam.height,
                      cam.width)
    old = lambda: lib.sgn_project_bwd_fused(*common(), L.stream_ptr())
    new = lambda: lib.sgn_project_bwd_fused_pose(*common(), m, P(offs), P(v_p), P(ws), ws.numel(), L.stream_ptr())
    for _ in range(5):
        old(); new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(5):
        t_old.append(timed(old, a.reps)); t_new.append(timed(new, a.reps))

    leaves = [{k: v.clone().requires_grad_(True) for k, v in mm.items()} for mm in models]
    op = poses.ObjectPoses(1, m - 1, "SO3xR3", dev)
    rots, centers = table0[1:, :9].reshape(-1, 3, 3).double(), table0[1:, 9:12].double()
    frame, tracks = torch.zeros(m - 1, dtype=torch.long, device=dev), torch.arange(m - 1, device=dev)
    w = torch.rand(cam.height, cam.width, 3, device=dev)

    def train(pose_on):
        table = op.table(frame, tracks, centers, rots) if pose_on else table0
        out = step.render_scene_graph(leaves, table, idft, cam, fused=True)
        loss = (out.rgb * w).mean() + out.alpha.mean() + out.object_acc.mean() + out.background_acc.mean()
        loss.backward()

    for _ in range(3):
        train(False); train(True)
    torch.cuda.synchronize()
    s_off, s_on = [], []
    for _ in range(3):
        s_off.append(timed(lambda: train(False), max(3, a.reps // 4)))
        s_on.append(timed(lambda: train(True), max(3, a.reps // 4)))
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps(dict(n=n, objects=m - 1, bwd_us=med(t_old), bwd_pose_us=med(t_new),
                          bwd_ratio=med(t_new) / med(t_old), step_off_us=med(s_off), step_on_us=med(s_on),
                          step_ratio=med(s_on) / med(s_off), bwd_samples=[t_old, t_new], step_samples=[s_off, s_on])))


if __name__ == "__main__":
    main()

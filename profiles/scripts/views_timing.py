"""Batched views on the MI355X: fwd+bwd time per view of ``views.render_views`` for B cameras against B sequential
``step.render_fused`` calls with backward, 1 M Gaussians at 1920x1280 (scenes.make_gaussians, cameras yawed by 0.05 rad
steps), B in {1, 2, 3, 4, 8}.  Device events around chunks of ``--reps`` iterations, the two forms alternating chunk by
chunk after warm-up, median over ``--chunks``; peak device memory of the batched form at the largest B.  Prints one JSON
line.

    python profiles/scripts/views_timing.py [--reps 5] [--chunks 7] [--bs 1,2,3,4,8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "street-gaussians-ns_amd"))

import torch  # noqa: E402

from sgn_rast import scenes, step, views  # noqa: E402

DEV = torch.device("cuda", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=7)
    ap.add_argument("--bs", default="1,2,3,4,8")
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    base = scenes.make_camera(1920, 1280, 2000.0)
    raw = {k: v.to(DEV) for k, v in scenes.make_gaussians(a.n, base, seed=0).items()}
    P = step.leaf_params(raw)
    bs = [int(x) for x in a.bs.split(",")]
    g = torch.Generator().manual_seed(0)
    w_img = torch.rand(1280, 1920, 3, generator=g).to(DEV)
    res = {"n": a.n, "H": 1280, "W": 1920, "reps": a.reps, "chunks": a.chunks, "per_view_us": {}}

    def batched(cams):
        for p in P.values():
            p.grad = None
        out = views.render_views(P, cams)
        (out.rgb * w_img).sum().backward()

    def sequential(cams):
        for p in P.values():
            p.grad = None
        for c in cams:
            o = step.render_fused(P, c)
            (o.rgb * w_img).sum().backward()

    def chunk(fn, cams):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(a.reps):
            fn(cams)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / a.reps / len(cams)

    for b in bs:
        cams = []
        for v in range(b):
            c = scenes.make_camera(1920, 1280, 2000.0, yaw=0.05 * (v - (b - 1) / 2))
            c.viewmat, c.cam_pos = c.viewmat.to(DEV), c.cam_pos.to(DEV)
            cams.append(c)
        for _ in range(3):                       # warm-up: capacities, caches, allocator
            batched(cams)
            sequential(cams)
        torch.cuda.synchronize()
        tb, ts = [], []
        for _ in range(a.chunks):
            tb.append(chunk(batched, cams))
            ts.append(chunk(sequential, cams))
        mb, ms = statistics.median(tb), statistics.median(ts)
        res["per_view_us"][str(b)] = {"batched": round(mb, 1), "sequential": round(ms, 1),
                                      "speedup": round(ms / mb, 3)}
        if b == max(bs):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            batched(cams)
            torch.cuda.synchronize()
            res["peak_mem_batched_GiB_B%d" % b] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
            torch.cuda.reset_peak_memory_stats()
            sequential(cams)
            torch.cuda.synchronize()
            res["peak_mem_sequential_GiB_B%d" % b] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        print(json.dumps({"B": b, **res["per_view_us"][str(b)]}), flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the absgrad statistic on the MI355X (rasterize_gaussians_fused(absgrad=True), csrc/raster_absgrad.hip): the
fused train step (step.train_step(fused=True), synthetic loss) with the statistic off and on, alternating block by block
(median of 5 blocks of --reps steps after warm-up), on the benchmark scene (1 M Gaussians, 1920x1280, scenes "metric")
and on the street workload (scenes.make_street_gaussians on the same camera).  Per variant:

- the step (device-event time per step);
- the backward's reverse walks and its unpack, from the library's own event spans (slots raster_bwd / unpack_grads): the
  walk span covers whatever launch shape ran — the long-walk and the short-walk kernel together (default), the short-walk
  kernel alone (adapt_bwd = 2^30: no walk counts as long) or the in-kernel adaptive split (tile_order off);
- with the statistic off the node's backward is the one-call entry, with it on the call-by-call path (its launch order
  comes from a separate sgn_tile_order call): the step figure contains that difference, the spans do not.

Prints one JSON line.

    python profiles/scripts/absgrad_timing.py [--reps 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "street-gaussians-ns_amd"))

import torch  # noqa: E402

from sgn_rast import _lib as L  # noqa: E402
from sgn_rast import config, scenes, step  # noqa: E402

SHAPES = {
    "two_kernel": {},                                   # default: long-walk kernel + short-walk kernel
    "short_only": dict(adapt_bwd=1 << 30),              # every walk in the short-walk kernel
    "mode0": dict(tile_order=False),                    # the in-kernel adaptive split
}


def timed_steps(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def spans(fn, reps):
    """us per step inside the raster_bwd and unpack_grads spans over `reps` steps."""
    L.timing_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rep = L.timing_report()
    L.timing_enable(False)
    return {k: rep[k][1] * 1e3 / max(1, reps) for k in ("raster_bwd", "unpack_grads")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam, raw = scenes.make_scene("metric", device=dev)
    res = dict(n=raw["means"].shape[0], image=[cam.width, cam.height], reps=a.reps, blocks=a.blocks)
    w_img, w_a = step.loss_weights(cam, seed=7, device=dev)
    workloads = {"benchmark": raw, "street": scenes.make_street_gaussians(raw["means"].shape[0], cam, seed=0, device=dev)}
    for wname, params in workloads.items():
        P = step.leaf_params(params)
        for sname, kw in SHAPES.items():
            with config.override(**kw):
                fns = {flag: (lambda flag=flag: step.train_step(P, cam, w_img, w_a, fused=True, absgrad=flag))
                       for flag in (False, True)}
                for _ in range(3):
                    for fn in fns.values():
                        fn()
                torch.cuda.synchronize()
                samples = {flag: [] for flag in fns}
                walk = {flag: [] for flag in fns}
                unpack = {flag: [] for flag in fns}
                for _ in range(a.blocks):
                    for flag, fn in fns.items():            # alternating: off, on, off, on, ...
                        samples[flag].append(timed_steps(fn, a.reps))
                        s = spans(fn, max(2, a.reps // 2))
                        walk[flag].append(s["raster_bwd"])
                        unpack[flag].append(s["unpack_grads"])
                med = lambda v: sorted(v)[len(v) // 2]
                for flag in fns:
                    key = f"{wname}.{sname}.{'absgrad' if flag else 'plain'}"
                    res[key] = dict(step_us=med(samples[flag]), walk_us=med(walk[flag]), unpack_us=med(unpack[flag]),
                                    step_samples=samples[flag], walk_samples=walk[flag])
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Cost of the antialiased rasterize mode on the MI355X (device-event timing after warm-up, median of 5 blocks of
--reps calls, the variants of one comparison alternating block by block), 1 M Gaussians at 1920x1280 (scenes "metric"):

- (i)   `sgn_aa_opacity_fwd` / `sgn_aa_opacity_bwd` alone, on the scene's logits and its projection's compensation
        output, on one set of buffers (warm: they stay in the last-level cache, as inside a step) and on 24 sets in
        turn (cold: HBM); next to them a device copy of the same number of bytes as the box's streaming rate;
- (ii)  the fused train step (step.train_step(fused=True), synthetic loss) in classic mode — run this script from a
        checkout of the parent commit with --classic-only for the other side of the comparison;
- (iii) the same step in antialiased mode, with the backward's walked / listed statistic and the mean accumulation of
        both modes: lower opacities lengthen the depth-list walks, so (iii) - (ii) is NOT the cost of the new kernels.

Prints one JSON line.

    python profiles/scripts/antialiased_timing.py [--reps 20] [--classic-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "street-gaussians-ns_amd"))

import torch  # noqa: E402

from sgn_rast import _lib as L  # noqa: E402
from sgn_rast import fused, ops, scenes, step  # noqa: E402


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def alternating(fns, reps, blocks=5, warm=3):
    """name -> (median us per call, the per-block samples): `blocks` rounds, every variant once per round."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            samples[k].append(timed(fn, reps))
    return {k: (sorted(v)[len(v) // 2], v) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--classic-only", action="store_true", help="(ii) alone: runs on a tree without the mode")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam, raw = scenes.make_scene("metric", device=dev)
    n = raw["means"].shape[0]
    w_img, w_a = step.loss_weights(cam, seed=7, device=dev)
    P = step.leaf_params(raw)
    res = dict(n=n, image=[cam.width, cam.height], reps=a.reps)
    walked, acc = {}, {}

    def train(mode):
        kw = {} if mode == "classic" else dict(rasterize_mode=mode)      # (the parent commit has no such argument)
        out = step.train_step(P, cam, w_img, w_a, fused=True, **kw)
        stat = ops._S().walk_stat
        if stat is not None:
            walked[mode] = stat
        acc[mode] = out.alpha.detach()

    modes = ("classic",) if a.classic_only else ("classic", "antialiased")
    t = alternating({m: (lambda m=m: train(m)) for m in modes}, a.reps)
    for m in modes:
        res[f"step_{m}_us"], res[f"step_{m}_samples"] = t[m]
        res[f"walked_permille_{m}"] = int(walked[m]) if m in walked else None
        res[f"mean_accumulation_{m}"] = float(acc[m].mean())
    if not a.classic_only:
        with torch.no_grad():
            comp = fused.project_gaussians_fused(P["means"], P["log_scales"], P["quats"], cam.viewmat[:3, :], cam.fx, cam.fy,
                                                 cam.cx, cam.cy, cam.height, cam.width, 16)[4].contiguous()
        logits = raw["opacity_logits"].reshape(-1).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        o, v_o, v_l, v_c = torch.empty(n, **f32), torch.randn(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32)
        src12, dst12 = torch.empty(6 * n // 4, **f32), torch.empty(6 * n // 4, **f32)        # 6 n bytes read + 6 n written
        src20, dst20 = torch.empty(10 * n // 4, **f32), torch.empty(10 * n // 4, **f32)
        lib, p, s = L.load(), L.ptr, L.stream_ptr()
        # "warm": the same 12 / 20 MB every call — they stay in the 256 MB last-level cache, as they do inside a step,
        # where the projection has just written the factor.  "cold": 24 sets of buffers in turn (480 MB), so every call
        # streams from HBM.
        sets = [tuple(torch.empty_like(t).copy_(t) for t in (logits, comp, v_o)) + (torch.empty(n, **f32),
                torch.empty(n, **f32), torch.empty(10 * n // 4, **f32), torch.empty(10 * n // 4, **f32)) for _ in range(24)]
        turn = [0]

        def cold(kind):
            l_, c_, v_, a_, b_, src, dst = sets[turn[0] % len(sets)]
            turn[0] += 1
            if kind == "fwd":
                lib.sgn_aa_opacity_fwd(n, p(l_), p(c_), p(a_), s)
            elif kind == "bwd":
                lib.sgn_aa_opacity_bwd(n, p(l_), p(c_), p(v_), p(a_), p(b_), s)
            else:
                dst.copy_(src)

        t = alternating({
            "aa_fwd": lambda: lib.sgn_aa_opacity_fwd(n, p(logits), p(comp), p(o), s),
            "aa_bwd": lambda: lib.sgn_aa_opacity_bwd(n, p(logits), p(comp), p(v_o), p(v_l), p(v_c), s),
            "aa_bwd_logits_only": lambda: lib.sgn_aa_opacity_bwd(n, p(logits), p(comp), p(v_o), p(v_l), None, s),
            "copy_12B_per_row": lambda: dst12.copy_(src12),
            "copy_20B_per_row": lambda: dst20.copy_(src20),
            "aa_fwd_cold": lambda: cold("fwd"), "aa_bwd_cold": lambda: cold("bwd"),
            "copy_20B_per_row_cold": lambda: cold("copy")}, 100 * a.reps, warm=30)
        for k, (med, samples) in t.items():
            res[k + "_us"], res[k + "_samples"] = med, samples
        for k, nbytes in (("aa_fwd", 12), ("aa_bwd", 20), ("copy_20B_per_row", 20), ("aa_fwd_cold", 12), ("aa_bwd_cold", 20),
                          ("copy_20B_per_row_cold", 20)):
            res[k + "_GBps"] = nbytes * n / res[k + "_us"] * 1e-3
        res["compensation_on_visible"] = [float(x) for x in torch.quantile(comp[comp > 0], torch.tensor([0.0, 0.5, 1.0],
                                                                                                        device=dev))]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

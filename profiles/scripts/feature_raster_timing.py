"""Forward + backward of `features.rasterize_features` against the multi-pass `ops.rasterize_gaussians(D = K)` on the
benchmark scene (1 M Gaussians, 1920x1280), same process, same tensors, warmed, interleaved (A B A B ...), binning
excluded on both sides (both find the list in the binning cache; asserted).  Device events around each call; the
gradients of one pair of calls are compared first (faster and different is not faster).

    python profiles/scripts/feature_raster_timing.py [--scene metric] [--reps 20] [--ks 1,2,3,4,8,16,20] [--out FILE]

Prints one JSON line per K; profiles/feature_raster.md keeps what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "street-gaussians-ns_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="metric")
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,2,3,4,8,16,20")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from sgn_rast import features as F, ops, scenes
    dev = torch.device("cuda", 0)
    cam, raw = scenes.make_scene(a.scene, n_override=a.n)
    P = {k: v.to(dev) for k, v in raw.items()}
    H, W = cam.height, cam.width
    with torch.no_grad():
        quats = P["quats"] / P["quats"].norm(dim=-1, keepdim=True)
        xys, depths, radii, conics, _c, nth, _cov = ops.project_gaussians(
            P["means"], P["log_scales"].exp(), 1.0, quats, cam.viewmat.to(dev), cam.fx, cam.fy, cam.cx, cam.cy, H, W, 16)
        opac = torch.sigmoid(P["opacity_logits"])
    n = xys.shape[0]
    xys.requires_grad_(True), conics.requires_grad_(True), opac.requires_grad_(True)
    g = torch.Generator().manual_seed(3)
    lines = []
    for K in [int(k) for k in a.ks.split(",")]:
        feats = torch.randn(n, K, generator=g).to(dev).requires_grad_(True)
        bg = (torch.rand(K, generator=g) + 0.1).to(dev)
        v_img, v_alpha = torch.rand(H, W, K, generator=g).to(dev), torch.rand(H, W, generator=g).to(dev)
        leaves = (xys, conics, feats, opac)

        def one_walk():
            return F.rasterize_features(xys, depths, radii, conics, nth, feats, opac, H, W, 16, bg, True)

        def multi_pass():
            return ops.rasterize_gaussians(xys, depths, radii, conics, nth, feats, opac, H, W, 16, bg, True)

        def run(fn, backward=True):
            for t in leaves:
                t.grad = None
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            img, alpha = fn()
            ev[1].record()
            if backward:
                torch.autograd.backward([img, alpha], [v_img, v_alpha])
            ev[2].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]), ev[0].elapsed_time(ev[2])

        # results first: same image bit for bit, gradients within the project's bar
        run(multi_pass)
        ref_img = multi_pass()[0].detach()
        ref = [t.grad.clone() for t in leaves]
        run(one_walk)
        assert torch.equal(one_walk()[0].detach(), ref_img), "forward images differ"
        rel = [float((t.grad.double() - r.double()).norm() / r.double().norm()) for t, r in zip(leaves, ref)]
        assert max(rel) < 1e-4, rel
        for _ in range(a.warmup):
            run(one_walk), run(multi_pass)
        b0 = ops.binning_stats["binnings"]
        t = {"one_walk": [], "multi_pass": []}
        for _ in range(a.reps):                        # interleaved
            t["one_walk"].append(run(one_walk))
            t["multi_pass"].append(run(multi_pass))
        assert ops.binning_stats["binnings"] == b0, "a timed call binned"
        row = {"K": K, "n": n, "image": [W, H], "reps": a.reps, "grad_rel_l2_vs_multi_pass": max(rel)}
        for name, v in t.items():
            fwd, tot = [x[0] for x in v], [x[1] for x in v]
            row[name] = {"fwd_ms": round(statistics.median(fwd), 4), "fwd_bwd_ms": round(statistics.median(tot), 4),
                         "fwd_bwd_min_ms": round(min(tot), 4), "fwd_bwd_max_ms": round(max(tot), 4)}
        row["speedup_fwd_bwd"] = round(row["multi_pass"]["fwd_bwd_ms"] / row["one_walk"]["fwd_bwd_ms"], 3)
        row["speedup_fwd"] = round(row["multi_pass"]["fwd_ms"] / row["one_walk"]["fwd_ms"], 3)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

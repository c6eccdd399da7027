"""Cost of the bilateral-grid colour correction on the MI355X (device-event timing after warm-up, median of 5 blocks of
--reps calls, the variants of one comparison alternating block by block), one 1280x1920 image:

- (i)  `sgn_bilagrid_slice_fwd` / `sgn_bilagrid_slice_bwd` alone for the grids (1,1,1) and (Wg,Hg,L) = (16,16,8), on
       white-noise colours (the tests' input: the luminance level changes from lane to lane) and on a smooth image
       (neighbouring lanes share a level), on one set of buffers (warm: 29.5 MB each, they stay in the last-level cache
       as inside a step) and — the (16,16,8) grid — on 8 sets in turn (cold: HBM); next to them the float32
       `F.grid_sample(align_corners=True, padding_mode="border")` formulation, forward and backward (autograd, graph
       kept), which is what a user would otherwise write, and device copies of 24 and 48 bytes per pixel as the box's
       streaming rate;
- (ii) the fused train step (`step.train_step(fused=True, gt=...)`, 1 M Gaussians, scenes "metric") without and with
       `appearance=(grids, 0)`.

Prints one JSON line.

    python profiles/scripts/bilagrid_timing.py [--reps 20] [--no-step]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "street-gaussians-ns_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sgn_rast import _lib as L  # noqa: E402
from sgn_rast import appearance, scenes, step  # noqa: E402

H, W = 1280, 1920


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


def textbook(grid, rgb):
    """The float32 formulation a user would write: grid [L,Hg,Wg,12] as a [1,12,L,Hg,Wg] volume through grid_sample."""
    x = ((torch.arange(W, device=rgb.device, dtype=torch.float32) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, device=rgb.device, dtype=torch.float32) + 0.5) / H)[:, None].expand(H, W)
    luma = 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]
    coords = torch.stack([x, y, luma], -1) * 2 - 1
    A = F.grid_sample(grid.permute(3, 0, 1, 2)[None], coords[None, None], mode="bilinear", padding_mode="border",
                      align_corners=True)
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] * rgb[..., None, :]).sum(-1) + A[..., 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    f32 = dict(dtype=torch.float32, device=dev)
    noise = (1.2 * torch.rand(H, W, 3, generator=g)).to(dev)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    smooth = torch.stack([0.1 + 0.8 * xx, 0.2 + 0.6 * yy, 0.5 + 0.4 * torch.sin(6 * xx + 3 * yy)], -1).to(dev).contiguous()
    v_out = torch.randn(H, W, 3, generator=g).to(dev)
    out, v_rgb = torch.empty(H, W, 3, **f32), torch.empty(H, W, 3, **f32)
    src24, dst24 = torch.empty(3 * H * W, **f32), torch.empty(3 * H * W, **f32)          # 12 B/px read + 12 written
    src48, dst48 = torch.empty(6 * H * W, **f32), torch.empty(6 * H * W, **f32)
    lib, p, s = L.load(), L.ptr, L.stream_ptr()
    res = dict(image=[W, H], reps=a.reps)
    eye = torch.tensor(appearance._IDENTITY)

    fns = {"copy_24B_per_px": lambda: dst24.copy_(src24), "copy_48B_per_px": lambda: dst48.copy_(src48)}
    keep = []
    for gname, (Lz, Hg, Wg) in (("affine", (1, 1, 1)), ("grid", (8, 16, 16))):
        grid = (eye.expand(Lz, Hg, Wg, 12) + 0.3 * torch.randn(Lz, Hg, Wg, 12, generator=g)).to(dev).contiguous()
        v_grid = torch.zeros_like(grid)
        for cname, rgb in (("noise", noise), ("smooth", smooth)):
            k = f"{gname}_{cname}"
            fns[k + "_fwd"] = lambda grid=grid, rgb=rgb, d=(Lz, Hg, Wg): lib.sgn_bilagrid_slice_fwd(
                *d, p(grid), H, W, H * W, p(rgb), p(out), s)
            fns[k + "_bwd"] = lambda grid=grid, rgb=rgb, d=(Lz, Hg, Wg), v_grid=v_grid: lib.sgn_bilagrid_slice_bwd(
                *d, p(grid), H, W, H * W, p(rgb), p(v_out), p(v_rgb), p(v_grid), s)
            fns[k + "_bwd_grid_only"] = lambda grid=grid, rgb=rgb, d=(Lz, Hg, Wg), v_grid=v_grid: \
                lib.sgn_bilagrid_slice_bwd(*d, p(grid), H, W, H * W, p(rgb), p(v_out), None, p(v_grid), s)
            if cname == "noise":
                gl, pl = grid.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
                o = textbook(gl, pl)
                keep.append((gl, pl, o))
                fns[k + "_torch_fwd"] = lambda grid=grid, rgb=rgb: textbook(grid, rgb)

                def torch_bwd(o=o, gl=gl, pl=pl):
                    gl.grad = pl.grad = None
                    o.backward(v_out, retain_graph=True)

                fns[k + "_torch_bwd"] = torch_bwd
        if gname == "grid":
            sets = [(noise.clone(), v_out.clone(), torch.empty_like(out), torch.empty_like(out)) for _ in range(8)]
            turn = [0]

            def cold(kind, grid=grid, v_grid=v_grid, sets=sets, turn=turn):
                r_, v_, o_, vr_ = sets[turn[0] % len(sets)]
                turn[0] += 1
                if kind == "fwd":
                    lib.sgn_bilagrid_slice_fwd(8, 16, 16, p(grid), H, W, H * W, p(r_), p(o_), s)
                else:
                    lib.sgn_bilagrid_slice_bwd(8, 16, 16, p(grid), H, W, H * W, p(r_), p(v_), p(vr_), p(v_grid), s)

            fns["grid_noise_fwd_cold"] = lambda: cold("fwd")
            fns["grid_noise_bwd_cold"] = lambda: cold("bwd")
    t = alternating(fns, a.reps, warm=5)
    n_pix = H * W
    for k, (med, samples) in t.items():
        res[k + "_us"], res[k + "_samples"] = round(med, 2), [round(x, 2) for x in samples]
        if k.endswith("_fwd") or k.endswith("_fwd_cold") or k.startswith("copy_24"):
            res[k + "_GBps"] = round(24 * n_pix / med * 1e-3, 1)
        elif "torch" not in k and "grid_only" not in k:
            res[k + "_GBps"] = round(48 * n_pix / med * 1e-3, 1)

    if not a.no_step:
        cam, raw = scenes.make_scene("metric", device=dev)
        w_img, w_a = step.loss_weights(cam, seed=7, device=dev)
        P = step.leaf_params(raw)
        gt = torch.rand(cam.height, cam.width, 3, generator=g).to(dev)
        grids = appearance.BilateralGrids(4).to(dev)
        with torch.no_grad():
            grids.grids.add_(0.05 * torch.randn(grids.grids.shape, generator=g).to(dev))
        affine = appearance.BilateralGrids(4, (1, 1, 1)).to(dev)

        def train(app):
            if app is not None:
                app.grids.grad = None
            step.train_step(P, cam, w_img, w_a, fused=True, gt=gt, **({} if app is None else {"appearance": (app, 0)}))

        t = alternating({"step_plain": lambda: train(None), "step_grid": lambda: train(grids),
                         "step_affine": lambda: train(affine)}, a.reps)
        for k, (med, samples) in t.items():
            res[k + "_us"], res[k + "_samples"] = round(med, 1), [round(x, 1) for x in samples]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

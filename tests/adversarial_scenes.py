"""Adversarial splat geometry for the rasterizer's culling shortcuts (plain seeded builders, CPU only).

The shortcuts — exact tile culling (`binning.hip`: cull_threshold / make_ellipse / row_interval), the emission's quadrant
masks (band_extent) and the raster rows' extents (`raster.hip`: build_grec_kernel's ex / ey) — are claimed to change no
image and no gradient.  `scenes.make_gaussians` never stresses them: no needles, no near-threshold opacities, nothing near
the near plane or outside 1.15x the frustum.  Each family here does, and tests/test_adversarial_scenes.py measures with
the C oracle's projection and the kernels' own fp32 validity test that it really does.

Every builder returns a `Scene`: raw parameters in `scenes.make_scene`'s layout, a camera, plus the opacities and colours
the raster tests feed.  `Scene.raster_inputs(CO)` projects with the C oracle (some families then place centres exactly in
pixel space and recompute the tile boxes with the projection's own arithmetic).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import numpy as np
import torch

from sgn_rast import scenes

F32 = np.float32
LOGIT_1_255 = float(np.float32(math.log((1 / 255) / (1 - 1 / 255))))   # the logit whose sigmoid is 1/255


@dataclass
class Scene:
    name: str
    cam: scenes.Camera
    raw: Dict[str, torch.Tensor]        # means, log_scales, quats, opacity_logits, features_dc, features_rest
    opacity: torch.Tensor               # [N,1] what the drop-in surface is given (exact values where it matters)
    colors: torch.Tensor                # [N,3]
    blocks: tuple = (16,)               # tile sizes the raster tests use (16: culling and masks; 8 where useful)
    snap_xy: Optional[torch.Tensor] = None   # [N,2] pixel centres to place the projected rows at exactly (NaN: keep)
    notes: Dict[str, object] = field(default_factory=dict)

    @property
    def n(self) -> int:
        return self.raw["means"].shape[0]

    def scales(self):
        return self.raw["log_scales"].exp()

    def quats(self):
        q = self.raw["quats"]
        return q / q.norm(dim=-1, keepdim=True)

    def project_args(self, block=16):
        c = self.cam
        return (self.raw["means"], self.scales(), 1.0, self.quats(), c.viewmat[:3, :], c.fx, c.fy, c.cx, c.cy,
                c.height, c.width, block)

    def raster_inputs(self, CO, block=16) -> dict:
        """The C oracle's projection (xys, depths, radii, conics, nth) of the scene, with `snap_xy` applied."""
        xys, depths, radii, conics, comp, nth, cov3d = CO.project_fwd(*self.project_args(block))
        if self.snap_xy is not None:
            keep = torch.isnan(self.snap_xy)
            xys = torch.where(keep | (radii[:, None] == 0), xys, self.snap_xy)
            nth = torch.where(radii > 0, tile_count(xys, radii, self.cam.width, self.cam.height, block), nth)
            live = nth > 0
            radii = torch.where(live, radii, torch.zeros_like(radii))
            nth = torch.where(live, nth, torch.zeros_like(nth))
        return dict(xys=xys, depths=depths, radii=radii, conics=conics, nth=nth, opac=self.opacity.clone(),
                    rgb=self.colors.clone(), logits=self.raw["opacity_logits"].clone())


# ---------------------------------------------------------------- the projection's arithmetic, restated in fp32
def _f2i(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, dtype=F32)
    out = np.trunc(np.clip(v, -2147483648.0, 2147483520.0)).astype(np.int64)
    out[v >= F32(2147483648.0)] = 2147483647
    out[np.isnan(v)] = 0
    return out


def tile_boxes(xys, radii, W, H, block):
    """(minx, miny, maxx, maxy) of gsplat's get_tile_bbox — oracle/c/sgn_oracle.c tile_bbox, fp32 step by step."""
    x = xys[:, 0].numpy().astype(F32); y = xys[:, 1].numpy().astype(F32)
    r = radii.numpy().astype(F32)
    b = F32(block)
    tcx, tcy, tr = x / b, y / b, r / b
    tx, ty = (W + block - 1) // block, (H + block - 1) // block
    mnx = np.clip(_f2i(tcx - tr), 0, tx); mxx = np.clip(_f2i((tcx + tr) + F32(1.0)), 0, tx)
    mny = np.clip(_f2i(tcy - tr), 0, ty); mxy = np.clip(_f2i((tcy + tr) + F32(1.0)), 0, ty)
    return [torch.from_numpy(v.astype(np.int64)) for v in (mnx, mny, mxx, mxy)]


def tile_count(xys, radii, W, H, block):
    mnx, mny, mxx, mxy = tile_boxes(xys, radii, W, H, block)
    return ((mxx - mnx).clamp_min(0) * (mxy - mny).clamp_min(0)).to(torch.int32)


# ------------------------------------------------------------------------------------------------- builders
def _quat_z_then_y(theta, phi):
    """Rotation by `theta` about the optical axis after a tilt `phi` about y (the long x axis leans toward the camera)."""
    cz, sz = torch.cos(theta / 2), torch.sin(theta / 2)
    cy, sy = torch.cos(phi / 2), torch.sin(phi / 2)
    # q = qz * qy, (w, x, y, z)
    return torch.stack([cz * cy, -sz * sy, cz * sy, sz * cy], dim=-1)


def _finish(name, cam, means, log_scales, quats, logits, g, opacity=None, blocks=(16,), snap_xy=None, **notes):
    n = means.shape[0]
    logits = logits.reshape(n, 1).float()
    if opacity is None:
        opacity = torch.sigmoid(logits)
    dc = (torch.rand(n, 1, 3, generator=g) - 0.5) / scenes.SH_C0
    rest = torch.randn(n, 15, 3, generator=g) * 0.05
    raw = dict(means=means.float().contiguous(), log_scales=log_scales.float().contiguous(),
               quats=quats.float().contiguous(), opacity_logits=logits.contiguous(), features_dc=dc, features_rest=rest)
    colors = torch.rand(n, 3, generator=g)
    return Scene(name, cam, raw, opacity.reshape(n, 1).float().contiguous(), colors, tuple(blocks), snap_xy, dict(notes))


def _logit(o):
    o = torch.as_tensor(o, dtype=torch.float64)
    return torch.log(o / (1 - o)).float()


def needles(seed=0, n=600, width=1920, height=1280, focal=2000.0) -> Scene:
    """One scale 100-1000x the other two; long axis in the image plane at 0, 0.3, pi/4, 1.0, pi/2 (and random angles),
    or tilted toward the camera.  alpha >= 1/255 lengths 30-1500 px, both tips on screen except for a fifth whose tips
    leave the image.  Opacities from the 255 o ~ 1 edge (the valid region shrinks to a sliver) to the 0.999 clamp."""
    g = torch.Generator().manual_seed(1000 + seed)
    cam = scenes.make_camera(width, height, focal)
    angles = torch.tensor([0.0, 0.3, math.pi / 4, 1.0, math.pi / 2])
    theta = torch.where(torch.rand(n, generator=g) < 0.7, angles[torch.randint(0, 5, (n,), generator=g)],
                        torch.rand(n, generator=g) * math.pi)
    theta = theta * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    phi = torch.where(torch.rand(n, generator=g) < 0.25, torch.rand(n, generator=g) * 1.2, torch.zeros(n))
    u = torch.rand(n, generator=g)
    opac = torch.where(u < 0.3, (1.0 + 0.5 * torch.rand(n, generator=g)) / 255.0,
                       torch.where(u < 0.5, 0.999 + 0.0009 * torch.rand(n, generator=g),
                                   0.05 + 0.9 * torch.rand(n, generator=g)))
    s_thr = torch.log(255.0 * opac).clamp_min(0.02)
    length = torch.exp(torch.rand(n, generator=g) * math.log(1500 / 30)) * 30      # alpha >= 1/255 length, px
    sigma_px = length / 2 / torch.sqrt(2 * s_thr)
    z = 3.0 + 5.0 * torch.rand(n, generator=g)
    L = sigma_px * z / focal
    aniso = torch.exp(torch.rand(n, generator=g) * math.log(10.0)) * 100.0          # 100x - 1000x
    w = L / aniso
    half = length / 2 * torch.cos(phi)
    hx, hy = (half * torch.cos(theta)).abs() + 2, (half * torch.sin(theta)).abs() + 2
    leave = torch.rand(n, generator=g) < 0.2
    rx, ry = torch.rand(n, generator=g), torch.rand(n, generator=g)
    lo_x, hi_x = torch.minimum(hx, torch.tensor(width / 2.0)), torch.maximum(width - hx, torch.tensor(width / 2.0))
    lo_y, hi_y = torch.minimum(hy, torch.tensor(height / 2.0)), torch.maximum(height - hy, torch.tensor(height / 2.0))
    px = torch.where(leave, rx * width, lo_x + rx * (hi_x - lo_x))
    py = torch.where(leave, ry * height, lo_y + ry * (hi_y - lo_y))
    means = torch.stack([(px - cam.cx) / focal * z, (py - cam.cy) / focal * z, z], -1)
    log_scales = torch.stack([L.log(), w.log(), w.log()], -1)
    quats = _quat_z_then_y(theta, phi)
    return _finish("needles", cam, means, log_scales, quats, _logit(opac), g, opacity=opac)


def thresholds(seed=0, n=1200, width=256, height=192, focal=256.0) -> Scene:
    """Opacities at the edges of the alpha test: 255 o in [1, 1.05] (the valid region degenerates toward the centre),
    255 o just below 1 (never visible), o >= 0.999 (the forward clamp); logits +-8, +-20 and logit(1/255) +- 1 ulp for
    the fused sigmoid paths.  Splats 1-25 px, anisotropic up to 50x, rotated."""
    g = torch.Generator().manual_seed(2000 + seed)
    cam = scenes.make_camera(width, height, focal)
    k = torch.arange(n)
    cls = k % 6
    o255 = torch.where(cls == 0, 1.0 + 0.05 * torch.rand(n, generator=g),
                       torch.where(cls == 1, 1.0 - 0.03 * torch.rand(n, generator=g) - 1e-6, torch.zeros(n)))
    opac = torch.where(cls <= 1, (o255.double() / 255.0).float(), 0.999 + 0.001 * torch.rand(n, generator=g))
    opac = torch.where(cls == 2, torch.minimum(opac, torch.tensor(0.99999)), opac)
    logits = _logit(opac.clamp(1e-7, 1 - 1e-7))
    special = torch.tensor([8.0, -8.0, 20.0, -20.0, LOGIT_1_255,
                            float(np.nextafter(F32(LOGIT_1_255), F32(1))), float(np.nextafter(F32(LOGIT_1_255), F32(-1)))])
    pick = special[torch.randint(0, special.numel(), (n,), generator=g)]
    use_logit = cls >= 3
    logits = torch.where(use_logit, torch.where(cls == 3, pick, _logit(torch.rand(n, generator=g) * 0.98 + 0.01)),
                         logits)
    opac = torch.where(use_logit, torch.sigmoid(logits), opac)
    z = 2.0 + 3.0 * torch.rand(n, generator=g)
    px, py = torch.rand(n, generator=g) * (width + 40) - 20, torch.rand(n, generator=g) * (height + 40) - 20
    means = torch.stack([(px - cam.cx) / focal * z, (py - cam.cy) / focal * z, z], -1)
    big = torch.exp(torch.rand(n, generator=g) * math.log(25.0)) * z / focal
    log_scales = torch.stack([big.log(), (big / (1 + 49 * torch.rand(n, generator=g))).log(), (big * 0.5).log()], -1)
    quats = torch.randn(n, 4, generator=g)
    return _finish("thresholds", cam, means, log_scales, quats, logits, g, opacity=opac)


def frustum(seed=0, n=1200, width=256, height=192, focal=200.0) -> Scene:
    """Depths in (0.01, 0.05], exactly 0.01 (culled) and the next float above it (live); centres at 1.3-3x tan_fov whose
    boxes still reach the image (the forward's clamp and the clamped-vjp branches are live); centres behind the camera."""
    g = torch.Generator().manual_seed(3000 + seed)
    cam = scenes.make_camera(width, height, focal)
    tfx, tfy = width / 2 / focal, height / 2 / focal
    k = torch.arange(n)
    cls = k % 4
    z = torch.where(cls == 0, 0.01 + 0.04 * torch.rand(n, generator=g), 1.0 + 4.0 * torch.rand(n, generator=g))
    z = torch.where((cls == 0) & (k % 16 == 0), torch.full((n,), 0.01), z)
    z = torch.where((cls == 0) & (k % 16 == 4), torch.full((n,), float(np.nextafter(F32(0.01), F32(1)))), z)
    z = torch.where(cls == 3, -(0.5 + 3 * torch.rand(n, generator=g)), z)
    u = (torch.rand(n, generator=g) * 2 - 1) * 1.1
    v = (torch.rand(n, generator=g) * 2 - 1) * 1.1
    # clamped rows: 1.3x-3x the half field of view on one axis (sometimes both), radius large enough to reach in
    mult = 1.3 + 1.7 * torch.rand(n, generator=g)
    sgn = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    on_x = torch.rand(n, generator=g) < 0.6
    both = torch.rand(n, generator=g) < 0.2
    u = torch.where((cls == 1) & (on_x | both), sgn * mult, u)
    v = torch.where((cls == 1) & (~on_x | both), -sgn * (1.3 + 1.7 * torch.rand(n, generator=g)), v)
    means = torch.stack([u * tfx * z.abs(), v * tfy * z.abs(), z], -1)
    over = torch.maximum((u.abs() - 1) * width / 2, (v.abs() - 1) * height / 2).clamp_min(0)
    sig_px = torch.where(cls == 1, (over + 10 + 40 * torch.rand(n, generator=g)) / 2.0,
                         2 + 10 * torch.rand(n, generator=g))
    s = sig_px * z.abs() / focal
    log_scales = torch.stack([s.log(), (s * (0.2 + torch.rand(n, generator=g))).log(),
                              (s * (0.2 + torch.rand(n, generator=g))).log()], -1)
    quats = torch.randn(n, 4, generator=g)
    logits = torch.randn(n, generator=g) * 1.5 + 1.0
    return _finish("frustum", cam, means, log_scales, quats, logits, g)


def huge(seed=0, n=160, width=1920, height=1280, focal=2000.0) -> Scene:
    """Radii larger than the image (the emission's whole-image rows), and a few with radii past BINREC_RAD_MAX = 2^30 - 1
    (scale ~2e5 at depth 1: sqrt of the 2D covariance ~4e8 px, still finite and inside int32 once tripled)."""
    g = torch.Generator().manual_seed(4000 + seed)
    cam = scenes.make_camera(width, height, focal)
    k = torch.arange(n)
    z = 1.0 + 9.0 * torch.rand(n, generator=g)
    px, py = torch.rand(n, generator=g) * width * 1.4 - 0.2 * width, torch.rand(n, generator=g) * height * 1.4 - 0.2 * height
    means = torch.stack([(px - cam.cx) / focal * z, (py - cam.cy) / focal * z, z], -1)
    sig_px = torch.exp(math.log(1500.0) + torch.rand(n, generator=g) * math.log(10.0))      # 1500 - 15000 px
    sig_px = torch.where(k % 20 == 0, torch.full((n,), 4.0e8), sig_px)                        # radius > 2^30
    s = sig_px * z / focal
    log_scales = torch.stack([s.log(), (s * (0.3 + 0.7 * torch.rand(n, generator=g))).log(), (s * 0.5).log()], -1)
    quats = torch.randn(n, 4, generator=g)
    quats = torch.where((k % 20 == 0)[:, None], torch.tensor([1.0, 0.0, 0.0, 0.0]), quats)    # keep their conic exact
    # translucent, so the walk reaches the small splats behind them too
    logits = _logit(0.02 + 0.2 * torch.rand(n, generator=g))
    return _finish("huge", cam, means, log_scales, quats, logits, g)


def _grid_targets(n, width, height, g):
    """Pixel-space centres: on 16-px tile borders, 8-px quadrant borders, pixel centres, at negative coordinates and
    beyond W / H."""
    kind = torch.arange(n) % 5
    bx = torch.randint(-1, width // 8 + 2, (n,), generator=g).float() * 8
    by = torch.randint(-1, height // 8 + 2, (n,), generator=g).float() * 8
    x = torch.where(kind == 0, (bx / 16).round() * 16, bx)
    y = torch.where(kind == 0, (by / 16).round() * 16, by)
    x = torch.where(kind == 2, torch.randint(0, width, (n,), generator=g).float() + 0.5, x)
    y = torch.where(kind == 2, torch.randint(0, height, (n,), generator=g).float() + 0.5, y)
    x = torch.where(kind == 3, -(torch.rand(n, generator=g) * 6 + 0.25), x)
    y = torch.where(kind == 3, torch.rand(n, generator=g) * height, y)
    x = torch.where(kind == 4, width + torch.rand(n, generator=g) * 6, x)
    y = torch.where(kind == 4, torch.where(torch.rand(n, generator=g) < 0.5, height + torch.rand(n, generator=g) * 6,
                                           torch.rand(n, generator=g) * height), y)
    # between pixel centres (x.0) for a fifth of the grid ones: sub-pixel splats there touch no pixel at all
    return torch.stack([x, y], -1)


def placement(seed=0, n=900, width=200, height=136, focal=180.0, name="placement") -> Scene:
    """Centres exactly on tile borders, quadrant borders and pixel centres, at negative coordinates and beyond W / H;
    a third are sub-pixel (the projected covariance at the 0.3 floor) and fall between pixel centres."""
    g = torch.Generator().manual_seed(5000 + seed + width)
    cam = scenes.make_camera(width, height, focal)
    xy = _grid_targets(n, width, height, g)
    z = 2.0 + 2.0 * torch.rand(n, generator=g)
    means = torch.stack([(xy[:, 0] - cam.cx) / focal * z, (xy[:, 1] - cam.cy) / focal * z, z], -1)
    tiny = torch.arange(n) % 3 == 0
    sig_px = torch.where(tiny, torch.full((n,), 1e-3), 0.5 + 8 * torch.rand(n, generator=g))
    s = sig_px * z / focal
    log_scales = torch.stack([s.log(), (s * (0.1 + torch.rand(n, generator=g))).log(), s.log()], -1)
    quats = torch.randn(n, 4, generator=g)
    logits = torch.where(tiny, torch.full((n,), 6.0), torch.randn(n, generator=g) * 2.0)
    blocks = (16, 8)
    return _finish(name, cam, means, log_scales, quats, logits, g, blocks=blocks, snap_xy=xy)


def placement_small(seed=0) -> Scene:
    """The placement family on a 45 x 13 image: H < 16 and neither side a multiple of 8 (partial tiles / quadrants)."""
    return placement(seed, n=240, width=45, height=13, focal=40.0, name="placement_small")


def stacks(seed=0, width=96, height=80, focal=100.0) -> Scene:
    """50-300 splats over single tiles, so lists cross the 64-entry LDS batch and the four-wave / long-walk split points
    the GPU tests force: a translucent stack that never saturates (o ~ 0.02, 300 deep), one that saturates inside its
    second batch (o ~ 0.1: T <= 1e-4 after ~90 entries), an opaque one (saturates after a few), and a stack of exact
    depth ties (the stable sort's Gaussian-id order decides)."""
    g = torch.Generator().manual_seed(6000 + seed)
    cam = scenes.make_camera(width, height, focal)
    specs = [((24.0, 24.0), 300, 0.02, False), ((56.0, 24.0), 200, 0.1, False), ((40.0, 56.0), 50, 0.9, False),
             ((72.0, 56.0), 150, 0.3, True)]
    means, ls, qs, ops = [], [], [], []
    for (cx, cy), m, o, ties in specs:
        z = torch.where(torch.full((m,), ties), 3.0 + (torch.arange(m) % 5).float(), 2.0 + 4.0 * torch.rand(m, generator=g))
        jx, jy = cx + torch.randn(m, generator=g) * 2.5, cy + torch.randn(m, generator=g) * 2.5
        means.append(torch.stack([(jx - cam.cx) / focal * z, (jy - cam.cy) / focal * z, z], -1))
        s = (2.0 + 4.0 * torch.rand(m, generator=g)) * z / focal
        ls.append(torch.stack([s.log(), (s * 0.7).log(), s.log()], -1))
        qs.append(torch.randn(m, 4, generator=g))
        ops.append((o * (0.8 + 0.4 * torch.rand(m, generator=g))).clamp(max=0.9995))
    means, ls, qs, opac = torch.cat(means), torch.cat(ls), torch.cat(qs), torch.cat(ops)
    return _finish("stacks", cam, means, ls, qs, _logit(opac), g, opacity=opac, blocks=(16, 8))


FAMILIES: Dict[str, Callable[[], Scene]] = {
    "needles": needles, "thresholds": thresholds, "frustum": frustum, "huge": huge, "placement": placement,
    "placement_small": placement_small, "stacks": stacks,
}


# ------------------------------------------------------------------------------- the kernels' validity test
def _fma_exact(a, b, c):
    """fp32 fma(a, b, c) with one rounding (fp64 product and sum are exact for fp32 inputs up to this range)."""
    return (a.double() * b.double() + c.double()).float()


def sigma_kernel_order(a, b, c, dx, dy):
    """fp32 sigma in the raster kernels' operation order: fma(b dx, dy, fma(hc dy, dy, (ha dx) dx)), ha = a/2, hc = c/2
    (raster.hip entry(); the C oracle's order is the same up to the exact scaling by 1/2).  The two fmas round once
    (fp64 inside), so the result does not depend on whether the device's torch contracts (torch.addcmul on the CPU
    rounds twice).  Shapes broadcast; any device."""
    s = ((0.5 * a) * dx) * dx
    s = _fma_exact((0.5 * c) * dy, dy, s)
    return _fma_exact(b * dx, dy, s)


def valid_pairs(R, W, H, block, rows, sigma_fn=sigma_kernel_order):
    """For the Gaussians `rows` (index tensor): per (Gaussian, tile of its box) the 4-bit mask of 8x8 quadrants (block
    16; block 8: bit 0 = the whole tile) that hold a pixel centre with sigma >= 0 and min(0.999, o exp(-sigma)) >= 1/255
    in fp32, the kernels' order.  Returns (gid, tile, bits) of the box's pairs, in row-major tile order per Gaussian."""
    xys, conics, opac, radii = R["xys"], R["conics"], R["opac"].reshape(-1), R["radii"]
    mnx, mny, mxx, mxy = tile_boxes(xys.cpu(), radii.cpu(), W, H, block)
    tiles_x = (W + block - 1) // block
    out_g, out_t, out_b = [], [], []
    dev = xys.device
    ar = torch.arange(block, dtype=torch.float32, device=dev)
    for gi in rows.tolist():
        if int(radii[gi]) <= 0:
            continue
        ty, tx = torch.meshgrid(torch.arange(int(mny[gi]), int(mxy[gi]), device=dev),
                                torch.arange(int(mnx[gi]), int(mxx[gi]), device=dev), indexing="ij")
        ty, tx = ty.reshape(-1), tx.reshape(-1)
        if ty.numel() == 0:
            continue
        bits = torch.zeros(ty.numel(), dtype=torch.int64, device=dev)
        for c0 in range(0, ty.numel(), 4096):
            cy, cx = ty[c0:c0 + 4096], tx[c0:c0 + 4096]
            px = cx[:, None].float() * block + ar[None, :] + 0.5
            py = cy[:, None].float() * block + ar[None, :] + 0.5
            dx = (xys[gi, 0] - px)[:, None, :]
            dy = (xys[gi, 1] - py)[:, :, None]
            a, b, c = conics[gi, 0], conics[gi, 1], conics[gi, 2]
            sig = sigma_fn(a.expand_as(dx * dy), b, c, dx.expand_as(dx * dy), dy.expand_as(dx * dy))
            alpha = torch.clamp(opac[gi] * torch.exp(-sig), max=0.999)
            inside = (px[:, None, :] < W) & (py[:, :, None] < H)
            ok = (sig >= 0) & (alpha >= 1.0 / 255.0) & inside
            if block == 16:
                q = ok.reshape(-1, 2, 8, 2, 8).any(dim=4).any(dim=2)
                bb = q[:, 0, 0].long() | (q[:, 0, 1].long() << 1) | (q[:, 1, 0].long() << 2) | (q[:, 1, 1].long() << 3)
            else:
                bb = ok.reshape(ok.shape[0], -1).any(dim=1).long()
            bits[c0:c0 + 4096] = bb
        out_g.append(torch.full_like(ty, gi)); out_t.append(ty * tiles_x + tx); out_b.append(bits)
    if not out_g:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return z, z, z
    return torch.cat(out_g), torch.cat(out_t), torch.cat(out_b)


def anisotropy(conics):
    """Ratio of the projected covariance's eigenvalues (= the conic's), per row."""
    a, b, c = conics[:, 0].double(), conics[:, 1].double(), conics[:, 2].double()
    mid, d = 0.5 * (a + c), torch.sqrt((0.5 * (a - c)) ** 2 + b * b)
    return (mid + d) / (mid - d).clamp_min(1e-300)

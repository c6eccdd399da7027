"""The rolling-shutter pass (include/sgn_rast.h "ROLLING SHUTTER", csrc/rolling_shutter.hip) restated in plain torch:
generic in dtype (the expressions in the contract's order, so the float32 run forms the kernel's numbers), differentiable
by autograd — and the time-sliced truth the model is measured against: per line of the shutter axis, render through
ordinary ops at the exact pose of that line's time and keep that line.  Test infrastructure only."""
import math
from types import SimpleNamespace

import torch

from sgn_rast import scenes, shutter

SH_C0 = 0.28209479177387814
BLOCK = 16

# (camera twist in world axes = camera axes for the identity camera, readout T, axis): the four motions of the profile note
MOTIONS = {
    "forward+yaw": ((0.3, 0.0, 6.0), (0.0, 0.6, 0.0), 0.03, "rows"),
    "sideways+roll": ((8.0, 1.0, 0.0), (0.1, 0.0, 0.3), 0.03, "rows"),
    "cols-reversed": ((0.3, 0.0, 6.0), (0.0, 0.6, 0.1), -0.03, "cols"),
    "fast": ((4.0, 0.0, 15.0), (0.0, 1.2, 0.0), 0.04, "rows"),
}


def _trunc(v):
    """C float -> int cast (toward zero), saturating, NaN -> 0."""
    return torch.clamp(torch.trunc(torch.nan_to_num(v.detach(), nan=0.0)), -2147483648.0, 2147483647.0).to(torch.int64)


def shear(xys, depths, radii, conics, cam, lin, ang, duration, axis, block=BLOCK, margin=0, clip_thresh=0.01,
          object_ids=None):
    """The contract, row-parallel.  ``lin`` [3] (or [M,3] with ``object_ids``) and ``ang`` [3] are CAMERA-frame
    velocities; everything is evaluated in ``xys.dtype``.  -> (xys', depths', radii', conics', num_tiles_hit', aux);
    ``aux.pre_int``: every value that goes under a ceil or a trunc, [N,5] (for the callers that must know how close to
    an integer the float64 run came), ``aux.alive``: the rows that are not culled."""
    dt = xys.dtype
    c = lambda v: torch.tensor(float(v), dtype=dt)
    fx, fy, cx, cy, T, m = c(cam.fx), c(cam.fy), c(cam.cx), c(cam.cy), c(duration), c(margin)
    rows = axis == "rows"
    assert rows or axis == "cols"
    E = c(cam.height if rows else cam.width)
    lin, ang = lin.to(dt), ang.to(dt)
    l = lin[object_ids.long()] if object_ids is not None else lin[None, :].expand(xys.shape[0], 3)
    valid = radii > 0
    one = torch.ones((), dtype=dt)
    z = torch.where(valid, depths, one)                       # keep the rows the projection culled finite
    ux, uy = xys[:, 0] - m, xys[:, 1] - m
    zz = z + c(1e-6)
    x = (ux - cx) * zz / fx
    y = (uy - cy) * zz / fy
    wx, wy, wz = ang[0], ang[1], ang[2]
    pdx = -l[:, 0] - (wy * z - wz * y)
    pdy = -l[:, 1] - (wz * x - wx * z)
    pdz = -l[:, 2] - (wx * y - wy * x)
    ax = fx * (pdx - (x / z) * pdz) / z
    ay = fy * (pdy - (y / z) * pdz) / z
    gx, gy = ax * T / E, ay * T / E
    gs, go = (gy, gx) if rows else (gx, gy)
    a_s, a_o = (ay, ax) if rows else (ax, ay)
    us, uo = (uy, ux) if rows else (ux, uy)
    k = 1.0 - gs
    b = -go
    slow = ~(k < 0.5)
    ks = torch.where(slow, k, one)                            # a row that k culls divides by 1 instead
    us1 = (us - c(0.5) * T * a_s) / ks
    tau1 = T * (us1 / E - c(0.5))
    uo1 = uo + a_o * tau1
    d1 = z + pdz * tau1
    q0, q1, q2 = conics[:, 0], conics[:, 1], conics[:, 2]
    qoo, qss = (q0, q2) if rows else (q2, q0)
    qos1 = qoo * b + q1 * k
    qss1 = b * qos1 + k * (q1 * b + qss * k)
    cc, d = go / ks, 1.0 + gs / ks
    t = 1.0 + cc * cc + d * d
    sigma = torch.sqrt(c(0.5) * (t + torch.sqrt(torch.clamp(t * t - c(4.0) * (d * d), min=0.0))))
    r_pre = radii.to(dt) * sigma.detach()
    radius = torch.ceil(r_pre)
    x1, y1 = (uo1, us1) if rows else (us1, uo1)
    tiles_x, tiles_y = (cam.width + block - 1) // block, (cam.height + block - 1) // block
    fb = c(block)
    tcx, tcy, tr = x1.detach() / fb, y1.detach() / fb, radius / fb
    pre = [tcx - tr, tcx + tr + 1.0, tcy - tr, tcy + tr + 1.0]
    mnx, mxx = _trunc(pre[0]).clamp(0, tiles_x), _trunc(pre[1]).clamp(0, tiles_x)
    mny, mxy = _trunc(pre[2]).clamp(0, tiles_y), _trunc(pre[3]).clamp(0, tiles_y)
    area = (mxx - mnx) * (mxy - mny)
    alive = valid & slow & (d1.detach() > clip_thresh) & (area > 0)
    zero = torch.zeros((), dtype=dt)
    izero = torch.zeros((), dtype=torch.int32)
    xys1 = torch.where(alive[:, None], torch.stack([x1, y1], dim=-1), zero)
    depths1 = torch.where(alive, d1, zero)
    sheared = torch.stack([qoo if rows else qss1, qos1, qss1 if rows else qoo], dim=-1)
    # a culled row's conic is written but carries no gradient; a row the projection culled keeps its own
    conics1 = torch.where(alive[:, None], sheared, torch.where(valid[:, None], sheared.detach(), conics.detach()))
    radii1 = torch.where(alive, _trunc(radius).to(torch.int32), izero)
    nth1 = torch.where(alive, area.to(torch.int32), izero)
    aux = SimpleNamespace(pre_int=torch.stack([r_pre] + pre, dim=-1).detach(), alive=alive, valid=valid, k=k.detach(),
                          shift=torch.where(alive[:, None], xys1.detach() - torch.stack([ux, uy], -1).detach(), zero))
    return xys1, depths1, radii1, conics1, nth1, aux


def camera_velocities(cam, rs, dtype=torch.float32):
    """(lin, ang) of the camera in its own frame as the host hands them to the kernel: float64, rounded once to float32."""
    l, w = shutter.camera_twist(cam, rs)
    return l.to(torch.float32).to(dtype), w.to(torch.float32).to(dtype)


def apply(xys, depths, radii, conics, cam, rs, block=BLOCK, object_ids=None, lin_table=None, dtype=None):
    """:func:`sgn_rast.shutter.apply` on the oracle: the five outputs (+ aux) for a ``RollingShutter``."""
    dt = dtype or xys.dtype
    lin, ang = camera_velocities(cam, rs, dt)
    if lin_table is not None:
        lin = lin_table.to(dt)
    return shear(xys.to(dt), depths.to(dt), radii, conics.to(dt), cam, lin, ang, rs.duration, rs.axis, block,
                 margin=rs.margin, object_ids=object_ids)


# ------------------------------------------------------------------------------------------------------ scenes

def _flat_colours(raw, rgb):
    """View-independent colours in the layout every entry takes (degree-0 coefficient, the higher bands zero): the
    renders below evaluate SH degree 0."""
    raw["features_dc"] = ((rgb - 0.5) / SH_C0)[:, None, :]
    raw["features_rest"] = torch.zeros_like(raw["features_rest"])
    return raw


def scene(n=400, seed=3):
    """The 64x48 scene of the profile note: 400 Gaussians, seeded uniform colours (SH degree 0), block 16."""
    cam = scenes.make_camera(64, 48, 60.0)
    raw = scenes.make_gaussians(n, cam, seed=seed, z_range=(2, 12), scale_range=(0.03, 0.25))
    rgb = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed + 100))
    return cam, _flat_colours(raw, rgb)


def edge_scene(n=120, seed=5):
    """The margin scene: small Gaussians whose centres project 0..7 px above the top edge of the 64x48 image."""
    cam = scenes.make_camera(64, 48, 60.0)
    g = torch.Generator().manual_seed(seed)
    raw = scenes.make_gaussians(n, cam, seed=seed, z_range=(2, 12), scale_range=(0.02, 0.06))
    z = raw["means"][:, 2]
    px = torch.rand(n, generator=g) * 60 + 2
    py = -torch.rand(n, generator=g) * 7
    raw["means"] = torch.stack([(px - cam.cx) * z / cam.fx, (py - cam.cy) * z / cam.fy, z], dim=-1)
    raw["opacity_logits"] = raw["opacity_logits"].clamp(min=0.5)
    rgb = torch.rand(n, 3, generator=g) * 0.7 + 0.3
    return cam, _flat_colours(raw, rgb)


EDGE_MOTION = ((0.0, 0.0, 0.0), (-3.0, 0.0, 0.0), 0.03, "rows")


def colours(raw):
    """SH degree 0 + 0.5, clamped: what every render below composites."""
    return torch.clamp(raw["features_dc"][:, 0, :] * SH_C0 + 0.5, min=0.0)


def _activated(raw):
    q = raw["quats"] / raw["quats"].norm(dim=-1, keepdim=True)
    return raw["means"], torch.exp(raw["log_scales"]), q, torch.sigmoid(raw["opacity_logits"])


def _render(ops, raw, cam, viewmat, project_frame=None, shear_with=None, **raster_kw):
    means, scales, quats, opac = _activated(raw)
    pcx, pcy, pH, pW = project_frame or (cam.cx, cam.cy, cam.height, cam.width)
    xys, depths, radii, conics, _comp, nth, _ = ops.project_gaussians(
        means, scales, 1, quats, viewmat[:3, :], cam.fx, cam.fy, pcx, pcy, pH, pW, BLOCK)
    if shear_with is not None:
        xys, depths, radii, conics, nth = shear_with(xys, depths, radii, conics)
    bg = torch.zeros(3, device=means.device)
    if not bool((nth > 0).any()):
        return bg.repeat(cam.height, cam.width, 1)
    return ops.rasterize_gaussians(xys, depths, radii, conics, nth, colours(raw), opac, cam.height, cam.width, BLOCK,
                                   background=bg, **raster_kw)


def plain_image(ops, raw, cam):
    """The global-shutter render at the mid-exposure pose (what the model produces without the pass)."""
    return _render(ops, raw, cam, cam.viewmat)


def compensated_image(ops, raw, cam, rs):
    """Projection on the margin-padded frame, the ORACLE's shear, the ordinary rasterizer."""
    def sh(xys, depths, radii, conics):
        dev = xys.device
        out = apply(xys.cpu(), depths.cpu(), radii.cpu(), conics.cpu(), cam_cpu(cam), rs)
        return tuple(t.to(dev) for t in out[:5])
    return _render(ops, raw, cam, cam.viewmat, project_frame=shutter.projection_frame(cam, rs), shear_with=sh)


def cam_cpu(cam):
    return scenes.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat.cpu(), cam.cam_pos.cpu())


def truth_image(ops, raw, cam, rs, band_kw=False):
    """The time-sliced truth: line c of the shutter axis comes from a global-shutter render at
    ``shutter.viewmat_at(cam, rs, T * ((c + 0.5) / E - 0.5))`` (pixel centres at c + 0.5).  ``band_kw``: the ops'
    rasterizer takes ``tile_rows=`` (the torch oracle's: only the tile row that holds the line is composited)."""
    rows = rs.axis == "rows"
    E = cam.height if rows else cam.width
    out = torch.zeros(cam.height, cam.width, 3, device=raw["means"].device)
    for c in range(E):
        t = rs.duration * ((c + 0.5) / E - 0.5)
        kw = dict(tile_rows=(c // BLOCK, c // BLOCK + 1)) if (band_kw and rows) else {}
        img = _render(ops, raw, cam, shutter.viewmat_at(cam, rs, t), **kw)
        if rows:
            out[c] = img[c]
        else:
            out[:, c] = img[:, c]
    return out


def psnr(a, b) -> float:
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10.0 * math.log10(1.0 / max(mse, 1e-30))

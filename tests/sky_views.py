"""Seeded camera views for the sky cube-map kernels' texture gradient (plain builders, CPU only).

`csrc/cubemap.hip` scatters the texture gradient per 16x16 pixel tile through `TileAcc`: an LDS window of 24x24 texels
anchored on the first texel of the tile's corner pixel, a segmented scan over each 16-lane pixel row that sums runs of
equal texel keys, a face and window check that routes each tap to LDS or to a global atomic, a bypass for C > 4 and a
flush of the non-zero cells.  Random directions reach almost none of that.  Each family here is built to put one of
those paths under load; tests/test_sky_views.py measures with the C oracle's taps (`c_oracle.cube_taps`) and a numpy
model of the routing that each one does, and tests/test_gpu_sky_per_texel.py compares the kernels texel by texel.

A `View` is a pinhole camera (h, w, fx, fy, cx, cy, c2w, jitter), a cube map (R, C), the entry points it is run through
(`texture`, `sky` = sky_color, `blend` = sky_blend) and, for the `texture` entry, optional directions that replace the
camera's (`dirs`, [..., 3] in the grid shape that entry point is given).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

TILE = 16
SKY_TW = 24            # csrc/cubemap.hip: SKY_TW = SKY_TH = 24, SKY_CMAX = 4
SKY_CMAX = 4


@dataclass
class View:
    name: str
    h: int
    w: int
    fx: float
    fy: float
    cx: float
    cy: float
    c2w_full: torch.Tensor              # the tensor the camera matrix is a view of
    R: int
    C: int
    entries: Tuple[str, ...]
    c2w_cols: int = 4                   # c2w = c2w_full[:3, :c2w_cols] (row stride = c2w_full's)
    jitter: Optional[torch.Tensor] = None   # [2,h,w] in [0,1) or None (pixel centres)
    dirs: Optional[torch.Tensor] = None     # override for the `texture` entry, [..., 3]
    batch: int = 1                      # `texture` entry: B independent maps / direction sets through sky.texture

    def c2w(self, device="cpu") -> torch.Tensor:
        return self.c2w_full.to(device)[:3, :self.c2w_cols]

    def texture_dirs(self, CO) -> torch.Tensor:
        """The `texture` entry's input [B, ..., 3]: the override, or the fused kernels' own directions (bit for bit)."""
        if self.dirs is not None:
            return self.dirs
        d = CO.sky_dirs(self.h, self.w, self.fx, self.fy, self.cx, self.cy, self.c2w(), self.jitter)
        return d.reshape(1, self.h, self.w, 3).expand(self.batch, -1, -1, -1).contiguous()

    def grid(self) -> Tuple[int, int]:
        """(h, w) of the pixel grid the backward tiles 16 x 16 (sky._CubeTexture's choice for the `texture` entry)."""
        if self.dirs is None:
            return self.h, self.w
        d = self.dirs[0]
        return (d.shape[-3], d.shape[-2]) if d.dim() >= 3 else (1, d.reshape(-1, 3).shape[0])


# ---------------------------------------------------------------- cameras
def rot(yaw: float, pitch: float, roll: float = 0.0) -> torch.Tensor:
    cy, sy, cp, sp, cr, sr = (math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll),
                              math.sin(roll))
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Rx = torch.tensor([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], dtype=torch.float64)
    Rz = torch.tensor([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]], dtype=torch.float64)
    return Ry @ Rx @ Rz


def look_along_gl(l, roll: float = 0.0) -> torch.Tensor:
    """A camera rotation whose optical axis looks along the GL-space direction `l` (the lookup's axes: (x, z, -y))."""
    lx, ly, lz = l
    f = torch.tensor([lx, -lz, ly], dtype=torch.float64)
    f = f / f.norm()
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    x = torch.linalg.cross(up, f)
    x = x / x.norm()
    y = torch.linalg.cross(f, x)
    R = torch.stack([x, y, f], 1)
    return R @ rot(0.0, 0.0, roll)


def c2w34(Rm: torch.Tensor, t=(1.0, 2.0, 3.0)) -> torch.Tensor:
    m = torch.zeros(3, 4, dtype=torch.float64)
    m[:, :3] = Rm
    m[:, 3] = torch.tensor(t, dtype=torch.float64)
    return m.float()


def jitter(h, w, seed) -> torch.Tensor:
    return torch.rand(2, h, w, generator=torch.Generator().manual_seed(seed))


# the benchmark's camera (bench.py / sgn_rast.scenes "metric": 1920 x 1280, fx = fy = 2000) and the reference's map size
PH, PW, PF = 1280, 1920, 2000.0
PROD_POSES = {"horizon": (0.0, 0.0), "yaw-pitch": (0.8, 0.3), "down": (2.4, -0.35)}


def _prod(name, pose, R, C, entries, jit_seed=None):
    yaw, pitch = PROD_POSES[pose]
    return View(name, PH, PW, PF, PF, PW / 2, PH / 2, c2w34(rot(yaw, pitch)), R, C, entries,
                jitter=None if jit_seed is None else jitter(PH, PW, jit_seed))


def production() -> List[View]:
    """1920x1280 at fx = 2000 on the 1024^2 map: ~3 pixels per texel, nearly every tap lands in its tile's window."""
    return [_prod("production/horizon/eval", "horizon", 1024, 3, ("sky", "blend")),
            _prod("production/horizon/jitter", "horizon", 1024, 3, ("sky", "texture"), jit_seed=1),
            _prod("production/yaw-pitch/eval", "yaw-pitch", 1024, 3, ("sky",)),
            _prod("production/yaw-pitch/jitter", "yaw-pitch", 1024, 3, ("sky", "blend"), jit_seed=2),
            _prod("production/down/jitter", "down", 1024, 3, ("sky",), jit_seed=3)]


def magnified() -> List[View]:
    """The same camera on 1-, 2- and 8-texel faces: whole tiles on 1-4 texels, runs of all 16 lanes of a pixel row; at
    R = 1 every lookup has two edge taps and a dropped corner tap."""
    return [_prod("magnified/R1/jitter", "yaw-pitch", 1, 3, ("sky", "texture"), jit_seed=4),
            _prod("magnified/R2/eval", "yaw-pitch", 2, 3, ("sky", "blend")),
            _prod("magnified/R8/jitter", "down", 8, 3, ("sky", "blend"), jit_seed=5)]


def minified() -> List[View]:
    """Small ragged images with a very wide field of view on the 1024^2 map: neighbouring pixels are tens of texels
    apart, so most taps miss the window and take the global path."""
    out = []
    for (h, w, f, pose, seed) in ((13, 45, 20.0, "yaw-pitch", 6), (120, 200, 22.0, "down", 7)):
        yaw, pitch = PROD_POSES[pose]
        out.append(View(f"minified/{w}x{h}", h, w, f, f * 1.1, w / 2 - 0.3, h / 2 + 0.2, c2w34(rot(yaw, pitch)), 1024,
                        3, ("sky", "texture", "blend"), jitter=jitter(h, w, seed)))
    return out


def _seam(name, l, R, C, entries, h=192, w=256, f=70.0, seed=8, roll=0.2):
    # (the optical axis off the tile grid's corners by half a tile: the corner or edge crosses tiles, not their borders)
    return View(name, h, w, f, f, w / 2 + 8.25, h / 2 - 7.75, c2w34(look_along_gl(l, roll)), R, C, entries,
                jitter=jitter(h, w, seed))


def seams() -> List[View]:
    """A wide field of view aimed at a cube corner (1,1,1) and along a cube edge (1,1,0): tiles that span two and three
    faces, edge taps re-projected onto the neighbouring face, corner taps dropped and the rest renormalised."""
    return [_seam("seams/corner/R6", (1, 1, 1), 6, 3, ("sky", "texture", "blend")),
            _seam("seams/corner/R96", (-1, 1, -1), 96, 3, ("sky", "blend"), seed=9, roll=-0.3),
            _seam("seams/edge/R64", (1, 1, 0), 64, 3, ("sky", "texture"), seed=10, roll=0.0)]


def invalid() -> List[View]:
    """NaN and zero directions for the `texture` entry: on the corner pixels of some tiles (the window's anchor is then
    invalid, hdr[0] = -1, and the whole tile goes to global memory) and scattered elsewhere."""
    out = []
    for (h, w, R, pose, seed) in ((96, 160, 64, "yaw-pitch", 11), (61, 77, 1024, "horizon", 12)):
        yaw, pitch = PROD_POSES[pose]
        v = View(f"invalid/{w}x{h}/R{R}", h, w, 0.9 * w, 0.9 * w, w / 2, h / 2, c2w34(rot(yaw, pitch)), R, 3,
                 ("texture",), jitter=jitter(h, w, seed))
        from oracle import c_oracle as CO
        d = CO.sky_dirs(h, w, v.fx, v.fy, v.cx, v.cy, v.c2w(), v.jitter).reshape(h, w, 3).clone()
        g = torch.Generator().manual_seed(seed)
        tiles = [(ty, tx) for ty in range(0, h, TILE) for tx in range(0, w, TILE)]
        pick = torch.randperm(len(tiles), generator=g)[: max(2, len(tiles) // 3)].tolist()
        bad = [torch.tensor([float("nan"), 0.3, 0.2]), torch.zeros(3), torch.tensor([0.1, float("nan"), 0.0])]
        for j, t in enumerate(pick):
            d[tiles[t][0], tiles[t][1]] = bad[j % len(bad)]
        scatter = torch.randperm(h * w, generator=g)[: h * w // 50]
        flat = d.reshape(-1, 3)
        flat[scatter[::2]] = torch.tensor([float("nan")] * 3)
        flat[scatter[1::2]] = torch.zeros(3)
        v.dirs = d[None]
        out.append(v)
    return out


def channels() -> List[View]:
    """C in {1, 2, 4, 5, 8} on the production geometry (reduced to 480x320 with the same pixels per texel) and on the
    seam geometry: the window for C <= 4 (exactly full at C = 4), the bypass to global atomics above."""
    out = []
    for C in (1, 2, 4, 5, 8):
        yaw, pitch = PROD_POSES["yaw-pitch"]
        out.append(View(f"channels/production/C{C}", 320, 480, PF / 4, PF / 4, 240.0, 160.0, c2w34(rot(yaw, pitch)),
                        256, C, ("sky", "texture"), jitter=jitter(320, 480, 20 + C)))
        out.append(_seam(f"channels/corner/C{C}", (1, 1, 1), 24, C, ("sky",), h=96, w=128, f=35.0, seed=30 + C))
    return out


def layouts() -> List[View]:
    """The flat grid (sky._CubeTexture's (1, n) fallback for [B, n, 3] directions), a batch of two maps through
    sky.texture, and c2w row strides other than 4: a [3,3] view of a [4,4] matrix, a [3,3] matrix, a [3,4] view of
    [3,8]."""
    from oracle import c_oracle as CO
    out = []
    yaw, pitch = PROD_POSES["yaw-pitch"]
    v = View("layouts/flat", 40, 130, 120.0, 120.0, 65.0, 20.0, c2w34(rot(yaw, pitch)), 32, 3, ("texture",),
             jitter=jitter(40, 130, 40))
    v.dirs = CO.sky_dirs(v.h, v.w, v.fx, v.fy, v.cx, v.cy, v.c2w(), v.jitter).reshape(1, -1, 3)
    out.append(v)
    v = View("layouts/batch2", 72, 100, 90.0, 90.0, 50.0, 36.0, c2w34(rot(2.0, 0.5)), 48, 3, ("texture",),
             jitter=jitter(72, 100, 41), batch=2)
    d0 = CO.sky_dirs(v.h, v.w, v.fx, v.fy, v.cx, v.cy, v.c2w(), v.jitter).reshape(v.h, v.w, 3)
    d1 = CO.sky_dirs(v.h, v.w, v.fx, v.fy, v.cx, v.cy, c2w34(rot(-1.0, -0.4)), None).reshape(v.h, v.w, 3)
    v.dirs = torch.stack([d0, d1], 0)
    out.append(v)
    m44 = torch.eye(4)
    m44[:3, :4] = c2w34(rot(0.5, 0.7))
    out.append(View("layouts/c2w-3x3-of-4x4", 80, 112, 95.0, 95.0, 56.0, 40.0, m44, 40, 3, ("sky", "blend"),
                    c2w_cols=3, jitter=jitter(80, 112, 42)))
    out.append(View("layouts/c2w-3x3", 80, 112, 95.0, 95.0, 56.0, 40.0, c2w34(rot(1.5, -0.2))[:, :3].contiguous(), 40,
                    3, ("sky",), c2w_cols=3))
    m38 = torch.full((3, 8), float("nan"))
    m38[:, :4] = c2w34(rot(-2.2, 0.1))
    out.append(View("layouts/c2w-3x4-of-3x8", 80, 112, 95.0, 95.0, 56.0, 40.0, m38, 40, 3, ("sky", "blend"),
                    jitter=jitter(80, 112, 43)))
    return out


FAMILIES = {"production": production, "magnified": magnified, "minified": minified, "seams": seams,
            "invalid": invalid, "channels": channels, "layouts": layouts}


def all_views() -> Dict[str, View]:
    return {v.name: v for fn in FAMILIES.values() for v in fn()}


# ---------------------------------------------------------------- the kernels' routing, modelled in numpy
def face_of(dirs: np.ndarray) -> np.ndarray:
    """The lookup's own face (cube_face_uv: z wins ties over y over x), -1 for a non-finite direction."""
    d = dirs.reshape(-1, 3).astype(np.float32)
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    zf = az > np.fmax(ax, ay)
    yf = ~zf & (ay > ax)
    idx = np.where(zf, 4, np.where(yf, 2, 0))
    c = np.where(zf, d[:, 2], np.where(yf, d[:, 1], d[:, 0]))
    idx = idx + (c < 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.isfinite(d).all(1) & (np.abs(c) > 0)
    return np.where(ok, idx, -1)


def routing(off: np.ndarray, h: int, w: int, R: int, C: int) -> dict:
    """Where TileAcc sends each tap of an h x w grid (off [h*w, 4] from cube_taps, -1 = dropped).

    The window is anchored on the tile's corner pixel (tile-local (0,0)): its first non-dropped tap gives the face and
    the origin (ix - 12, iy - 12); a tap goes to LDS when C <= 4, it is on that face and within the 24 x 24 window,
    else to a global atomic.  Returns per-tap `lds` / `glob` masks [h*w, 4], the per-tile anchor face, and the tile of
    every pixel."""
    off = off.reshape(h * w, 4).astype(np.int64)
    RR = R * R
    face, rem = off // RR, off % RR
    iy, ix = rem // R, rem % R
    py, px = np.divmod(np.arange(h * w), w)
    tx_n = (w + TILE - 1) // TILE
    tile = (py // TILE) * tx_n + px // TILE
    ty_all, tx_all = np.divmod(np.arange(((h + TILE - 1) // TILE) * tx_n), tx_n)
    corner = ty_all * TILE * w + tx_all * TILE
    co = off[corner]
    first = np.argmax(co >= 0, axis=1)
    anc = co[np.arange(len(corner)), first]
    has = (co >= 0).any(1)
    a_face = np.where(has, anc // RR, -1)
    a_x = (anc % RR) % R - SKY_TW // 2
    a_y = (anc % RR) // R - SKY_TW // 2
    valid = off >= 0
    t = tile[:, None]
    lds = valid & (C <= SKY_CMAX) & (face == a_face[t]) & (ix - a_x[t] >= 0) & (ix - a_x[t] < SKY_TW) & \
        (iy - a_y[t] >= 0) & (iy - a_y[t] < SKY_TW)
    return dict(lds=lds, glob=valid & ~lds, anchor_face=a_face, tile=tile, face=np.where(valid, face, -1))


def row_runs(off: np.ndarray, h: int, w: int) -> np.ndarray:
    """Length of the run of equal keys that ends at each tap, within the 16-lane pixel rows of the tiles, for the taps
    that end a run (the lanes that emit in add_seg); 0 elsewhere.  [h*w, 4]."""
    off = off.reshape(h * w, 4)
    Wp = (w + TILE - 1) // TILE * TILE
    grid = np.full((h, Wp, 4), -2, dtype=np.int64)
    grid[:, :w] = off.reshape(h, w, 4)
    rows = grid.reshape(h, Wp // TILE, TILE, 4)
    run = np.zeros_like(rows)
    run[:, :, 0] = 1
    for j in range(1, TILE):
        run[:, :, j] = np.where(rows[:, :, j] == rows[:, :, j - 1], run[:, :, j - 1] + 1, 1)
    last = np.ones_like(rows, dtype=bool)
    last[:, :, :-1] = rows[:, :, 1:] != rows[:, :, :-1]
    out = np.where(last & (rows >= 0), run, 0).reshape(h, Wp, 4)[:, :w]
    return out.reshape(h * w, 4)

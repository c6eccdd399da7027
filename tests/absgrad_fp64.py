"""float64 numpy restatement of the 3-channel compositing and its per-pixel reverse walk, written from the contract in
`csrc/raster.hip` / `csrc/raster_common.h` (not from the kernels' code), for the absgrad statistic (AbsGS): per Gaussian
the SIGNED sum of the per-pixel screen-space gradients — what `v_xy` is — and the sum of their ABSOLUTE values — what
`sgn_raster_bwd_abs` writes to `v_xy_abs`.

Contract, per tile of `block` x `block` pixels and per entry of its depth list (Gaussians whose tile bounding box —
`trunc((c -+ r) / block)` in float32, as the binning forms it — holds the tile, by float32 depth, ties by id), with
d = centre - pixel centre, (A, B, C) the conic and o the opacity:
    sigma = (A dx^2 + C dy^2) / 2 + B dx dy;   av = o exp(-sigma);   alpha = min(0.999, av)
    forward:  skipped if sigma < 0 or alpha < 1/255;  nT = T (1 - alpha);  the pixel STOPS (entry not composited) if
              nT <= 1e-4;  else C += colour alpha T,  T = nT,  last = position
    image = C + T_final background,  alpha image = 1 - T_final
    reverse walk (positions <= last, T starts at T_final; pixels nothing was composited onto take no part):
              alpha_b = min(alpha_clamp_bwd, av);  skipped if sigma < 0 or alpha_b < 1/255
              ra = 1 / (1 - alpha_b);  T_before = T ra;  v_alpha = ra (T dotc + c0 - bv)  with  dotc = colour . v_img,
              c0 = T_final (v_alpha_img - background . v_img),  bv = sum over the entries behind of alpha_b T_before dotc
              v_sigma = -av v_alpha   (gsplat 0.1.x: NOT zeroed where the clamp is active; `clamp_zeroes_grad` gives
                                       autograd's version, -alpha v_alpha and 0 where av > clamp, for the torch oracle)
              per-pixel gradient  g = v_sigma (A dx + B dy,  B dx + C dy)
    signed[g] = sum_pixels g,   absolute[g] = sum_pixels |g|   (componentwise)

"Threshold-adjacent" Gaussians — where float32 and float64 may legitimately take different sides of a test, so that a
comparison must leave them out — have some pair whose alpha is within 1e-5 of 1/255 or whose av is within 1e-5 of a
clamp (0.999, `alpha_clamp_bwd`), or a valid pair at a pixel where some nT is within 1e-5 (relative) of 1e-4.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

ADJ = 1e-5
H, W = 40, 56                      # 3 x 4 tiles of 16 with ragged right and bottom edges; 5 x 7 tiles of 8
# The seed of the scenes the GPU tests use (tests/test_gpu_absgrad.py), chosen so that at most 2 % of the visible
# Gaussians are threshold-adjacent at both tile sizes — tests/test_absgrad_fp64.py asserts it.
SEED = 21


def tile_bbox(xys, radii, tiles_x, tiles_y, block):
    """Inclusive-min / exclusive-max tile range of every Gaussian, float32 like the binning."""
    fb = np.float32(block)
    tcx, tcy, tr = xys[:, 0] / fb, xys[:, 1] / fb, radii.astype(np.float32) / fb
    one = np.float32(1.0)
    mnx = np.clip(np.trunc(tcx - tr).astype(np.int64), 0, tiles_x)
    mxx = np.clip(np.trunc(tcx + tr + one).astype(np.int64), 0, tiles_x)
    mny = np.clip(np.trunc(tcy - tr).astype(np.int64), 0, tiles_y)
    mxy = np.clip(np.trunc(tcy + tr + one).astype(np.int64), 0, tiles_y)
    return mnx, mny, mxx, mxy


def make_scene(seed, n_small=230, n_large=10, n_cluster=60, block=16, single=False):
    """A 40 x 56 scene in screen space (float32 arrays, what the projection would hand the rasterizer): ~300 Gaussians —
    `n_large` that cover several tiles, a cluster of `n_cluster` opaque ones over the single tile (1, 1), small ones
    everywhere, a few with an opacity above the backward's clamp.  `single`: ONE isotropic Gaussian centred on a pixel
    centre well inside tile (1, 1) — the cancellation case."""
    rng = np.random.default_rng(seed)
    if single:
        n = 1
        xy = np.array([[24.5, 23.5]])
        s = np.array([[1.75, 1.75]]); th = np.zeros(1); opac = np.array([0.6])
    else:
        n = n_small + n_large + n_cluster
        xy = np.concatenate([rng.uniform([-2, -2], [W + 2, H + 2], (n_small, 2)),
                             rng.uniform([4, 4], [W - 4, H - 4], (n_large, 2)),
                             rng.uniform([17, 17], [31, 31], (n_cluster, 2))])
        s = np.concatenate([rng.uniform(0.35, 0.8, (n_small, 2)), rng.uniform(3.0, 4.0, (n_large, 2)),
                            rng.uniform(0.7, 1.2, (n_cluster, 2))])
        th = rng.uniform(0, np.pi, n)
        opac = np.concatenate([rng.uniform(0.05, 0.95, n_small), rng.uniform(0.3, 0.9, n_large),
                               rng.uniform(0.7, 0.95, n_cluster)])
        opac[:6] = rng.uniform(0.992, 0.9995, 6)             # above the backward's clamp (0.99)
    c, sn = np.cos(th), np.sin(th)
    sxx = c * c * s[:, 0] ** 2 + sn * sn * s[:, 1] ** 2
    syy = sn * sn * s[:, 0] ** 2 + c * c * s[:, 1] ** 2
    sxy = c * sn * (s[:, 0] ** 2 - s[:, 1] ** 2)
    det = sxx * syy - sxy * sxy
    conics = np.stack([syy / det, -sxy / det, sxx / det], 1).astype(np.float32)
    lam = 0.5 * (sxx + syy) + np.sqrt(np.maximum(0.25 * (sxx - syy) ** 2 + sxy ** 2, 0))
    radii = np.ceil(3.0 * np.sqrt(lam)).astype(np.int32)
    xys = xy.astype(np.float32)
    depths = rng.permutation(n).astype(np.float32) * np.float32(0.03) + np.float32(1.0)    # distinct
    tiles_x, tiles_y = (W + block - 1) // block, (H + block - 1) // block
    mnx, mny, mxx, mxy = tile_bbox(xys, radii, tiles_x, tiles_y, block)
    nth = ((mxx - mnx) * (mxy - mny)).astype(np.int32)
    radii = np.where(nth > 0, radii, 0).astype(np.int32)     # off-screen: culled, as the projection reports it
    colors = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    return SimpleNamespace(n=n, H=H, W=W, block=block, xys=xys, depths=depths, radii=radii, conics=conics,
                           num_tiles_hit=nth, colors=colors, opacities=opac.astype(np.float32),
                           background=np.array([0.2, 0.5, 0.3], np.float32),
                           w_img=rng.uniform(-1, 1, (H, W, 3)).astype(np.float32),
                           w_alpha=rng.uniform(-1, 1, (H, W)).astype(np.float32))


def reverse_walk(sc, v_img, v_alpha_img, alpha_clamp_bwd=0.99, clamp_zeroes_grad=False):
    """-> SimpleNamespace(signed [N,2], absolute [N,2], adjacent [N] bool, visible [N] bool, img [H,W,3],
    alpha [H,W], n_stopped) in float64; `v_img` [H,W,3] / `v_alpha_img` [H,W]: the loss's gradients w.r.t. the two
    images."""
    f8 = np.float64
    n, B = sc.n, sc.block
    xys, conics, colors, opac, bg = (np.asarray(a, f8) for a in (sc.xys, sc.conics, sc.colors, sc.opacities,
                                                                 sc.background))
    v_img, v_alpha_img = np.asarray(v_img, f8), np.asarray(v_alpha_img, f8)
    tiles_x, tiles_y = (sc.W + B - 1) // B, (sc.H + B - 1) // B
    mnx, mny, mxx, mxy = tile_bbox(sc.xys, sc.radii, tiles_x, tiles_y, B)
    by_depth = np.lexsort((np.arange(n), sc.depths))         # float32 depth, ties by id
    signed, absolute = np.zeros((n, 2)), np.zeros((n, 2))
    adjacent, visible = np.zeros(n, bool), np.zeros(n, bool)
    n_stopped = 0                                            # pixels whose walk ended at the 1e-4 test
    img, alpha_img = np.empty((sc.H, sc.W, 3)), np.empty((sc.H, sc.W))
    third = 1.0 / 255.0
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            y0, y1, x0, x1 = ty * B, min((ty + 1) * B, sc.H), tx * B, min((tx + 1) * B, sc.W)
            py, px = (a.reshape(-1) for a in np.meshgrid(np.arange(y0, y1) + 0.5, np.arange(x0, x1) + 0.5,
                                                         indexing="ij"))
            lst = [g for g in by_depth if sc.radii[g] > 0 and mnx[g] <= tx < mxx[g] and mny[g] <= ty < mxy[g]]
            P = px.size
            T, C, last = np.ones(P), np.zeros((P, 3)), np.full(P, -1)
            live, near_stop = np.ones(P, bool), np.zeros(P, bool)
            pairs = []                                                      # per entry: dx, dy, sigma, av
            for k, g in enumerate(lst):
                dx, dy = xys[g, 0] - px, xys[g, 1] - py
                A, Bc, Cc = conics[g]
                sigma = 0.5 * (A * dx * dx + Cc * dy * dy) + Bc * dx * dy
                av = opac[g] * np.exp(-sigma)
                alpha = np.minimum(0.999, av)
                pairs.append((dx, dy, sigma, av))
                # a pair float32 may put on the other side of the 1/255 test or of a clamp (pixels still compositing)
                if (live & (sigma >= 0) & ((np.abs(alpha - third) <= ADJ) | (np.abs(av - 0.999) <= ADJ) |
                                           (np.abs(av - alpha_clamp_bwd) <= ADJ))).any():
                    adjacent[g] = True
                valid = live & (sigma >= 0) & (alpha >= third)
                nT = T * (1.0 - alpha)
                near_stop |= valid & (np.abs(nT - 1e-4) <= ADJ * 1e-4)
                stop = valid & (nT <= 1e-4)
                acc = valid & ~stop
                C += np.where(acc, alpha * T, 0.0)[:, None] * colors[g][None, :]
                T = np.where(acc, nT, T)
                last = np.where(acc, k, last)
                live &= ~stop
            n_stopped += int((~live).sum())
            img[y0:y1, x0:x1] = (C + T[:, None] * bg[None, :]).reshape(y1 - y0, x1 - x0, 3)
            alpha_img[y0:y1, x0:x1] = (1.0 - T).reshape(y1 - y0, x1 - x0)
            # ---- the reverse walk
            vo = v_img[y0:y1, x0:x1].reshape(P, 3)
            voa = v_alpha_img[y0:y1, x0:x1].reshape(P)
            part = last >= 0                                   # pixels something was composited onto
            Tf = T.copy()
            c0 = Tf * (voa - vo @ bg)
            bv = np.zeros(P)
            for k in range(len(lst) - 1, -1, -1):
                g = lst[k]
                dx, dy, sigma, av = pairs[k]
                alpha_b = np.minimum(alpha_clamp_bwd, av)
                valid = part & (k <= last) & (sigma >= 0) & (alpha_b >= third)
                if not valid.any():
                    continue
                visible[g] = True
                if (valid & near_stop).any():
                    adjacent[g] = True
                ra = 1.0 / (1.0 - alpha_b)
                Tb = T * ra
                dotc = vo @ colors[g]
                v_a = ra * (T * dotc + c0 - bv)
                v_a = np.where(valid, v_a, 0.0)
                bv = bv + np.where(valid, alpha_b * Tb * dotc, 0.0)
                T = np.where(valid, Tb, T)
                if clamp_zeroes_grad:
                    v_sigma = np.where(av < alpha_clamp_bwd, -alpha_b * v_a, 0.0)
                else:
                    v_sigma = -av * v_a
                A, Bc, Cc = conics[g]
                gx, gy = v_sigma * (A * dx + Bc * dy), v_sigma * (Bc * dx + Cc * dy)
                signed[g] += (gx.sum(), gy.sum())
                absolute[g] += (np.abs(gx).sum(), np.abs(gy).sum())
    return SimpleNamespace(signed=signed, absolute=absolute, adjacent=adjacent, visible=visible, img=img,
                           alpha=alpha_img, n_stopped=n_stopped)


@lru_cache(maxsize=None)
def reference(seed, block=16, single=False, alpha_clamp_bwd=0.99, clamp_zeroes_grad=False, rgb_sum_loss=False):
    """(scene, reverse_walk result) for the loss sum(img * w_img) + sum(alpha * w_alpha) of the scene's own weights
    (`rgb_sum_loss`: img.sum()), computed once per argument tuple and shared; callers leave both unchanged."""
    sc = make_scene(seed, block=block, single=single)
    if rgb_sum_loss:
        v_img, v_a = np.ones((sc.H, sc.W, 3)), np.zeros((sc.H, sc.W))
    else:
        v_img, v_a = sc.w_img, sc.w_alpha
    return sc, reverse_walk(sc, v_img, v_a, alpha_clamp_bwd, clamp_zeroes_grad)



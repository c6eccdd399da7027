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


def walk(sc, v_img, v_alpha_img, alpha_clamp_bwd=0.99, clamp_zeroes_grad=False, *, on_pair, on_tile=None, id_range=None,
         dtype=np.float64, exp=np.exp, opacities=None, sigma_adjacent=False):
    """The contract above, tile by tile: the forward compositing, then the reverse walk.  What is summed from it is the
    caller's business — `reverse_walk` below sums the screen-space gradient, `tests/raster_fp64.py` every output:
        on_tile(t)  once per tile after its forward: t.y0, t.y1, t.x0, t.x1, t.lst (the depth list), t.C [P,3], t.T [P]
                    (T_final), t.weights (per entry alpha T where it was composited, else 0), t.last [P]
        on_pair(p)  once per entry of the reverse walk some pixel evaluates, back to front: p.tile (the on_tile record),
                    p.g, p.k, p.valid [P], p.dx, p.dy, p.e (= exp(-sigma)), p.av, p.alpha_b, p.T_before, p.v_alpha,
                    p.v_sigma (the last two are 0 on pixels that are not valid WHERE av is finite), p.vo [P,3]
    `dtype`: every array and constant, hence every operation, in that type (float32: an emulation of a float32
    implementation).  `exp`: the exponential (called on -sigma).  `id_range=(lo, hi)`: the sub-list of those ids, same
    relative order.  `opacities`: instead of the scene's.  `sigma_adjacent`: a pair with |sigma| <= 1e-5 (the sigma < 0
    test) is threshold-adjacent too.
    -> SimpleNamespace(adjacent [N], visible [N], adjacent_px [H,W], n_stopped, list_len [tiles], walk_len [tiles])."""
    dt = np.dtype(dtype).type
    n, B = sc.n, sc.block
    xys, conics, colors, bg = (np.asarray(a, dt) for a in (sc.xys, sc.conics, sc.colors, sc.background))
    opac = np.asarray(sc.opacities if opacities is None else opacities, dt)
    v_img, v_alpha_img = np.asarray(v_img, dt), np.asarray(v_alpha_img, dt)
    tiles_x, tiles_y = (sc.W + B - 1) // B, (sc.H + B - 1) // B
    mnx, mny, mxx, mxy = tile_bbox(sc.xys, sc.radii, tiles_x, tiles_y, B)
    by_depth = np.lexsort((np.arange(n), sc.depths))         # float32 depth, ties by id
    lo, hi = (0, n) if id_range is None else id_range
    adjacent, visible = np.zeros(n, bool), np.zeros(n, bool)
    adjacent_px = np.zeros((sc.H, sc.W), bool)
    n_stopped = 0                                            # pixels whose walk ended at the 1e-4 test
    list_len, walk_len = [], []
    half, one, zero, a_max, a_bwd, t_min = dt(0.5), dt(1.0), dt(0.0), dt(0.999), dt(alpha_clamp_bwd), dt(1e-4)
    third = one / dt(255.0)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            y0, y1, x0, x1 = ty * B, min((ty + 1) * B, sc.H), tx * B, min((tx + 1) * B, sc.W)
            py, px = (a.reshape(-1).astype(dt) for a in np.meshgrid(np.arange(y0, y1) + 0.5, np.arange(x0, x1) + 0.5,
                                                                    indexing="ij"))
            lst = [g for g in by_depth if lo <= g < hi and sc.radii[g] > 0 and mnx[g] <= tx < mxx[g]
                   and mny[g] <= ty < mxy[g]]
            P = px.size
            T, C, last = np.ones(P, dt), np.zeros((P, 3), dt), np.full(P, -1)
            live, near_stop, near_px = np.ones(P, bool), np.zeros(P, bool), np.zeros(P, bool)
            pairs, weights = [], []                                         # per entry: dx, dy, sigma, e, av
            for k, g in enumerate(lst):
                dx, dy = xys[g, 0] - px, xys[g, 1] - py
                A, Bc, Cc = conics[g]
                sigma = half * (A * dx * dx + Cc * dy * dy) + Bc * dx * dy
                e = exp(-sigma)
                av = opac[g] * e
                alpha = np.minimum(a_max, av)
                pairs.append((dx, dy, sigma, e, av))
                # a pair float32 may put on the other side of the 1/255 test or of a clamp (pixels still compositing)
                near = live & (sigma >= 0) & ((np.abs(alpha - third) <= ADJ) | (np.abs(av - a_max) <= ADJ) |
                                              (np.abs(av - a_bwd) <= ADJ))
                if sigma_adjacent:
                    near |= live & (np.abs(sigma) <= ADJ)
                if near.any():
                    adjacent[g] = True
                    near_px |= near
                valid = live & (sigma >= 0) & (alpha >= third)
                nT = T * (one - alpha)
                near_stop |= valid & (np.abs(nT - t_min) <= ADJ * 1e-4)
                stop = valid & (nT <= t_min)
                acc = valid & ~stop
                w = np.where(acc, alpha * T, zero)
                weights.append(w)
                C += w[:, None] * colors[g][None, :]
                T = np.where(acc, nT, T)
                last = np.where(acc, k, last)
                live &= ~stop
            n_stopped += int((~live).sum())
            list_len.append(len(lst))
            walk_len.append(int(last.max()) + 1)
            adjacent_px[y0:y1, x0:x1] = (near_px | near_stop).reshape(y1 - y0, x1 - x0)
            tile = SimpleNamespace(y0=y0, y1=y1, x0=x0, x1=x1, lst=lst, C=C, T=T, weights=weights, last=last)
            if on_tile is not None:
                on_tile(tile)
            # ---- the reverse walk
            vo = v_img[y0:y1, x0:x1].reshape(P, 3)
            voa = v_alpha_img[y0:y1, x0:x1].reshape(P)
            part = last >= 0                                   # pixels something was composited onto
            Tf = T.copy()
            c0 = Tf * (voa - vo @ bg)
            bv = np.zeros(P, dt)
            for k in range(len(lst) - 1, -1, -1):
                g = lst[k]
                dx, dy, sigma, e, av = pairs[k]
                alpha_b = np.minimum(a_bwd, av)
                valid = part & (k <= last) & (sigma >= 0) & (alpha_b >= third)
                if not valid.any():
                    continue
                visible[g] = True
                if (valid & near_stop).any():
                    adjacent[g] = True
                ra = one / (one - alpha_b)
                Tb = T * ra
                dotc = vo @ colors[g]
                v_a = ra * (T * dotc + c0 - bv)
                v_a = np.where(valid, v_a, zero)
                bv = bv + np.where(valid, alpha_b * Tb * dotc, zero)
                T = np.where(valid, Tb, T)
                if clamp_zeroes_grad:
                    v_sigma = np.where(av < a_bwd, -alpha_b * v_a, zero)
                else:
                    v_sigma = -av * v_a
                on_pair(SimpleNamespace(tile=tile, g=g, k=k, valid=valid, dx=dx, dy=dy, e=e, av=av, alpha_b=alpha_b,
                                        T_before=Tb, v_alpha=v_a, v_sigma=v_sigma, vo=vo))
    return SimpleNamespace(adjacent=adjacent, visible=visible, adjacent_px=adjacent_px, n_stopped=n_stopped,
                           list_len=np.array(list_len), walk_len=np.array(walk_len))


def reverse_walk(sc, v_img, v_alpha_img, alpha_clamp_bwd=0.99, clamp_zeroes_grad=False):
    """-> SimpleNamespace(signed [N,2], absolute [N,2], adjacent [N] bool, visible [N] bool, img [H,W,3],
    alpha [H,W], n_stopped) in float64; `v_img` [H,W,3] / `v_alpha_img` [H,W]: the loss's gradients w.r.t. the two
    images."""
    conics, bg = np.asarray(sc.conics, np.float64), np.asarray(sc.background, np.float64)
    signed, absolute = np.zeros((sc.n, 2)), np.zeros((sc.n, 2))
    img, alpha_img = np.empty((sc.H, sc.W, 3)), np.empty((sc.H, sc.W))

    def on_tile(t):
        img[t.y0:t.y1, t.x0:t.x1] = (t.C + t.T[:, None] * bg[None, :]).reshape(t.y1 - t.y0, t.x1 - t.x0, 3)
        alpha_img[t.y0:t.y1, t.x0:t.x1] = (1.0 - t.T).reshape(t.y1 - t.y0, t.x1 - t.x0)

    def on_pair(p):
        A, Bc, Cc = conics[p.g]
        gx, gy = p.v_sigma * (A * p.dx + Bc * p.dy), p.v_sigma * (Bc * p.dx + Cc * p.dy)
        signed[p.g] += (gx.sum(), gy.sum())
        absolute[p.g] += (np.abs(gx).sum(), np.abs(gy).sum())

    w = walk(sc, v_img, v_alpha_img, alpha_clamp_bwd, clamp_zeroes_grad, on_pair=on_pair, on_tile=on_tile)
    return SimpleNamespace(signed=signed, absolute=absolute, adjacent=w.adjacent, visible=w.visible, img=img,
                           alpha=alpha_img, n_stopped=w.n_stopped)


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



"""float64 numpy definition of EVERY output of the 3-channel rasterizer — per pixel the image, alpha = 1 - T_final and the
depth channel, per Gaussian the nine sums of the backward and the four gradients made from them — each with the sum of
the ABSOLUTE values of its terms, the scale of an implementation's float32 rounding error.  Written from the contract in
the docstring of `tests/absgrad_fp64.py` (whose tile walk it shares: `absgrad_fp64.walk`), DESIGN.md section 4 and the
row layout comment of `csrc/raster_common.h`, not from the kernels' code.

Per evaluated (pixel, entry) pair of the reverse walk, with d = centre - pixel centre and the walk's v_sigma, v_alpha,
alpha_b, T_before:
    raw moments   m_x = sum v_sigma dx,  m_y = sum v_sigma dy,  s_xx = sum v_sigma dx^2,  s_xy = sum v_sigma dx dy,
                  s_yy = sum v_sigma dy^2
    v_xy      = (A m_x + B m_y,  B m_x + C m_y)            scale (|A| sum|v_sigma dx| + |B| sum|v_sigma dy|, ...): the
                                                           implementations sum the moments FIRST and apply the conic
                                                           afterwards, that is where their rounding error lives
    v_conic   = (s_xx / 2,  s_xy,  s_yy / 2)
    v_colors  = sum alpha_b T_before v_img                 (`colors_pre >= 0` masks it where the colour was a clamp)
    v_opacity = sum exp(-sigma) v_alpha                    (gsplat 0.1.x: NOT zeroed where the clamp is active;
                                                           `clamp_zeroes_grad`: autograd's version, 0 where av >= clamp)
    v_logit   = v_opacity s (1 - s)                        scale sum|.| s (1 + s): float32 implementations (and torch's
                                                           sigmoid backward) form 1 - s by SUBTRACTION, whose absolute
                                                           error is that of s — for s -> 1 the factor keeps only a few
                                                           digits, and the scale says so
Per pixel: img = C + T_final bg (scale sum|colour alpha T| + T_final |bg|), alpha = 1 - T_final (scale 1 + T_final),
depth = sum depth_g alpha T (scale sum|depth_g| alpha T).

The bound of the tests, per row or pixel and per component:  |got - exp| <= K 2^-24 scale,  exactly 0 where scale == 0.

`emulate` evaluates the same definition with every operation rounded to float32 (the walk in float32, the T ra
recurrence kept), sums the per-pixel terms of every Gaussian in seeded random orders and in 64-lane-tree order, and, for
the hardware-exp mode, multiplies exp(-sigma) by (1 + d), |d| = (1 + sigma log2 e) 2^-23 with a seeded random sign.  K is
4 x the worst ratio it and the C oracle reach, rounded up to a power of two (tests/test_raster_fp64.py measures and
asserts; profiles/raster_fp64.md records)."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import absgrad_fp64 as A

SEED, SEED_VIEW2 = A.SEED, 4
H, W = A.H, A.W
EPS = 2.0 ** -24
N_EDGE = 30
# both cut through the cluster (ids 240..299): most of the scene (walked over the shared list: row0, the id tests) and
# less than half of it (walked over a compacted list window)
ID_RANGE, ID_WINDOW = (30, 270), (260, 330)

# ---- the bounds.  K = 4 x (worst ratio |err| / (2^-24 scale) over the float32 emulation — blocks 16 / 8 / 5, 8 random
# orders + the 64-lane tree — and the C oracle), rounded up to a power of two; the 4 is for FMA contraction differences
# and v_rcp_f32's 1 ulp, neither of which the emulation has.  K_HW: the same with the emulation's perturbed exp.
# Measured ratios: profiles/raster_fp64.md; tests/test_raster_fp64.py asserts 4 x worst <= K on every run.
K = dict(img=256, alpha=64, depth=256, v_xy=64, v_conic=128, v_colors=128, v_opacity=128, v_logit=32)
K_HW = dict(img=256, alpha=64, depth=256, v_xy=128, v_conic=128, v_colors=512, v_opacity=512, v_logit=64)
PIXEL_OUTPUTS, ROW_OUTPUTS = ("img", "alpha", "depth"), ("v_xy", "v_conic", "v_colors", "v_opacity", "v_logit")


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _edge_rows():
    """~30 rows appended to `absgrad_fp64.make_scene`'s (whose rows and random stream do not move): the edges where a
    kernel goes wrong.  -> xy [E,2], conic [E,3], radius [E], opacity (probability) [E], colour before the clamp [E,3]."""
    iso = lambda a: (a, 0.0, a)
    L = lambda logit: float(_sigmoid(logit))
    rows = [
        # centres outside the image whose footprint reaches in
        (-3.2, 10.3, iso(0.25), 6, 0.6), (58.6, 20.2, iso(0.25), 6, 0.6), (30.1, -2.7, iso(0.25), 6, 0.6),
        (20.7, 42.9, iso(0.25), 6, 0.6),
        # opacity below 1/255: never visible, exact zeros
        (8.3, 30.7, iso(0.5), 5, 0.0035), (44.2, 6.6, iso(0.5), 5, 0.002), (50.1, 33.3, iso(0.5), 5, 0.0005),
        # opacity 0.9999, both over pixel (12.5, 8.5): its walk stops at the second one in every view
        (12.45, 8.55, iso(0.8), 4, 0.9999), (12.55, 8.45, iso(0.8), 4, 0.9999),
        # logits +12, -12 (never visible) and -5 (visible on a few pixels around the centre): s (1 - s) towards 0
        (36.3, 12.6, iso(1.0), 3, L(12.0)), (6.7, 20.1, iso(1.0), 3, L(12.0)),
        (47.7, 22.4, iso(1.0), 3, L(-12.0)), (14.2, 35.5, iso(1.0), 3, L(-12.0)),
        (33.4, 33.6, iso(0.3), 6, L(-5.0)), (22.2, 5.4, iso(0.3), 6, L(-5.0)),
        # non-PSD conics (B^2 > A C): sigma < 0 on part of the footprint
        (27.7, 9.2, (0.2, 0.27, 0.2), 6, 0.5), (10.2, 26.1, (0.2, -0.23, 0.2), 6, 0.5),
        (45.3, 28.7, (0.15, 0.3, 0.3), 6, 0.5),
        # the only pixel where alpha >= 1/255 is the image's last one (55.5, 39.5)
        (56.3, 40.2, iso(5.0), 2, 0.5),
        # two of exactly equal depth over the cluster's tile (ties go by id)
        (24.3, 24.6, iso(0.6), 4, 0.7), (25.1, 23.9, iso(0.6), 4, 0.6),
        # colours whose value before the clamp is negative
        (18.6, 12.4, iso(0.4), 5, 0.5), (38.3, 20.8, iso(0.4), 5, 0.5), (4.4, 36.2, iso(0.4), 5, 0.5),
        (52.3, 14.8, iso(0.4), 5, 0.5),
        # a needle across several tiles, one over nine of the twelve 16-tiles (the last tile's walk stays below 16
        # entries: the short-walk kernel's), three centred on tile corners
        (28.3, 30.4, (0.05, 0.0, 4.0), 14, 0.8), (20.2, 14.3, iso(0.02), 22, 0.3),
        (32.0, 16.0, iso(1.0), 3, 0.9), (48.0, 32.0, iso(1.0), 3, 0.9),
        (16.0, 32.0, iso(1.0), 3, 0.9),
    ]
    assert len(rows) == N_EDGE
    pre = np.full((N_EDGE, 3), np.nan)
    pre[21:25] = [(-0.3, 0.5, 0.2), (0.4, -0.1, -0.2), (-0.5, -0.5, -0.5), (0.0, -1e-3, 0.7)]
    rng = np.random.default_rng(7)                           # (a stream of its own)
    pre = np.where(np.isnan(pre), rng.uniform(0, 1, (N_EDGE, 3)), pre)
    return (np.array([r[:2] for r in rows]), np.array([r[2] for r in rows]), np.array([r[3] for r in rows]),
            np.array([r[4] for r in rows]), pre)


@lru_cache(maxsize=None)
def make_scene(seed=SEED, block=16, shared_logits_of=None):
    """`absgrad_fp64.make_scene(seed)` (rows 0..299, unchanged) + the edge rows; float32 arrays.  Adds `logits` (float32;
    `opacities` is float32(sigmoid(logits)): both routes see the same scene up to that rounding), `colors_pre` (`colors`
    is its clamp at 0).  `shared_logits_of=seed0`: the opacities of THAT scene (a second view of the same Gaussians)."""
    b = A.make_scene(seed, block=block)
    xy, conic, radius, opac, pre = _edge_rows()
    n0, n = b.n, b.n + N_EDGE
    f4 = np.float32
    xys = np.concatenate([b.xys, xy.astype(f4)])
    conics = np.concatenate([b.conics, conic.astype(f4)])
    j = np.arange(N_EDGE)
    j[20] = 19                                               # rows n0+19, n0+20: exactly equal depths
    depths = np.concatenate([b.depths, (1.015 + 0.3 * j).astype(f4)])
    assert np.unique(depths).size == n - 1
    tiles_x, tiles_y = (W + block - 1) // block, (H + block - 1) // block
    radii = np.concatenate([b.radii, radius.astype(np.int32)])
    mnx, mny, mxx, mxy = A.tile_bbox(xys, radii, tiles_x, tiles_y, block)
    nth = np.where(radii > 0, (mxx - mnx) * (mxy - mny), 0).astype(np.int32)
    radii = np.where(nth > 0, radii, 0).astype(np.int32)
    p = np.concatenate([b.opacities.astype(np.float64), opac])
    logits = np.log(p / (1.0 - p)).astype(f4)
    if shared_logits_of is not None:
        logits = make_scene(shared_logits_of, block).logits
    colors_pre = np.concatenate([b.colors, pre.astype(f4)])
    return SimpleNamespace(n=n, n_base=n0, H=H, W=W, block=block, xys=xys, depths=depths, radii=radii, conics=conics,
                           num_tiles_hit=nth, colors=np.maximum(colors_pre, 0).astype(f4), colors_pre=colors_pre,
                           logits=logits, opacities=_sigmoid(logits.astype(np.float64)).astype(f4),
                           background=b.background, w_img=b.w_img, w_alpha=b.w_alpha)


def hardware_exp(seed):
    """exp with `v_exp_f32`'s error model: 1 ulp of the result + the rounding of the argument's scaling by log2 e —
    exp(x) (1 + d), |d| = (1 + |x| log2 e) 2^-23, seeded random sign."""
    rng = np.random.default_rng(seed)

    def f(x):
        d = (1.0 + np.abs(x.astype(np.float64)) * np.log2(np.e)) * 2.0 ** -23 * rng.choice([-1.0, 1.0], x.shape)
        return (np.exp(x.astype(np.float64)) * (1.0 + d)).astype(x.dtype)
    return f


def rounded_exp(x):
    """exp evaluated in float64 and rounded to x's type: the same on every machine (numpy's float32 exp is not)."""
    return np.exp(x.astype(np.float64)).astype(x.dtype)


def _tree_sum(chunks):
    """[9] float32: every chunk [9, P] (one tile's pixels for one entry) reduced in 64-lane waves by a butterfly, the
    wave sums added one after the other — the order a wave reduction + atomics per wave would give."""
    total = np.zeros(chunks[0].shape[0], chunks[0].dtype)
    for c in chunks:
        pad = (-c.shape[1]) % 64
        x = np.pad(c, ((0, 0), (0, pad))).reshape(c.shape[0], -1, 64)
        while x.shape[2] > 1:
            x = x[:, :, :x.shape[2] // 2] + x[:, :, x.shape[2] // 2:]
        for wv in range(x.shape[1]):
            total = total + x[:, wv, 0]
    return total


def _finish(sc, raw, raw_abs, opac_p, dt):
    """The outputs from the nine sums [N,9] and their absolute sums, in `dt`: -> (values, scales) dicts."""
    conics = np.asarray(sc.conics, dt)
    Ac, Bc, Cc = conics[:, 0], conics[:, 1], conics[:, 2]
    half = dt(0.5)
    val, scl = {}, {}
    val["moments"], scl["moments"] = raw[:, :5], raw_abs[:, :5]
    mx, my, ax, ay = raw[:, 0], raw[:, 1], raw_abs[:, 0], raw_abs[:, 1]
    val["v_xy"] = np.stack([Ac * mx + Bc * my, Bc * mx + Cc * my], 1)
    scl["v_xy"] = np.stack([np.abs(Ac) * ax + np.abs(Bc) * ay, np.abs(Bc) * ax + np.abs(Cc) * ay], 1)
    val["v_conic"] = np.stack([half * raw[:, 2], raw[:, 3], half * raw[:, 4]], 1)
    scl["v_conic"] = np.stack([half * raw_abs[:, 2], raw_abs[:, 3], half * raw_abs[:, 4]], 1)
    val["v_colors"], scl["v_colors"] = raw[:, 5:8], raw_abs[:, 5:8]
    mask = (np.asarray(sc.colors_pre) >= 0) if hasattr(sc, "colors_pre") else np.ones((sc.n, 3), bool)
    val["v_colors_pre"], scl["v_colors_pre"] = np.where(mask, raw[:, 5:8], dt(0)), np.where(mask, raw_abs[:, 5:8], dt(0))
    val["v_opacity"], scl["v_opacity"] = raw[:, 8], raw_abs[:, 8]
    s = np.asarray(opac_p, dt)
    val["v_logit"] = raw[:, 8] * s * (dt(1) - s)
    scl["v_logit"] = raw_abs[:, 8] * s * (dt(1) + s)
    return val, scl


def definition(sc, v_img, v_alpha_img, alpha_clamp_bwd=0.99, clamp_zeroes_grad=False, id_range=None, logit=False,
               dtype=np.float64, exp=np.exp, orders=None):
    """Every output of the rasterizer for the loss gradients `v_img` [H,W,3], `v_alpha_img` [H,W].
    `logit`: the opacities are sigmoid(sc.logits) evaluated in `dtype` (what an entry given logits sees), else the scene's
    float32 probabilities.  `orders` (float32 emulation): a list of "tree" / int seeds — the per-pixel terms of every
    Gaussian are summed in each of these orders and `runs` holds one `val` dict per order; default: one exact `np.sum`.
    -> SimpleNamespace(val, scale: dicts over img [H,W,3], alpha, depth [H,W], moments [N,5], v_xy [N,2], v_conic [N,3],
    v_colors, v_colors_pre [N,3], v_opacity, v_logit [N];  runs;  adjacent [N], adjacent_px [H,W], visible [N],
    n_stopped, list_len, walk_len [tiles], depth_max)."""
    dt = np.dtype(dtype).type
    n = sc.n
    opac_p = (dt(1) / (dt(1) + rounded_exp(-sc.logits.astype(dt)))) if logit else np.asarray(sc.opacities, dt)
    bg, depths = np.asarray(sc.background, dt), np.asarray(sc.depths, dt)
    colors = np.asarray(sc.colors, dt)
    img, img_s = np.empty((sc.H, sc.W, 3), dt), np.empty((sc.H, sc.W, 3), dt)
    alpha, alpha_s = np.empty((sc.H, sc.W), dt), np.empty((sc.H, sc.W), dt)
    depth, depth_s = np.empty((sc.H, sc.W), dt), np.empty((sc.H, sc.W), dt)
    raw, raw_abs = np.zeros((n, 9), dt), np.zeros((n, 9), dt)
    chunks = [[] for _ in range(n)] if orders is not None else None

    def on_tile(t):
        shp = (t.y1 - t.y0, t.x1 - t.x0)
        P = t.T.size
        Cs, D, Ds = np.zeros((P, 3), dt), np.zeros(P, dt), np.zeros(P, dt)
        for g, w in zip(t.lst, t.weights):
            Cs += w[:, None] * np.abs(colors[g])[None, :]
            D += depths[g] * w
            Ds += np.abs(depths[g]) * w
        img[t.y0:t.y1, t.x0:t.x1] = (t.C + t.T[:, None] * bg[None, :]).reshape(*shp, 3)
        img_s[t.y0:t.y1, t.x0:t.x1] = (Cs + t.T[:, None] * np.abs(bg)[None, :]).reshape(*shp, 3)
        alpha[t.y0:t.y1, t.x0:t.x1] = (dt(1) - t.T).reshape(shp)
        alpha_s[t.y0:t.y1, t.x0:t.x1] = (dt(1) + t.T).reshape(shp)
        depth[t.y0:t.y1, t.x0:t.x1], depth_s[t.y0:t.y1, t.x0:t.x1] = D.reshape(shp), Ds.reshape(shp)

    def on_pair(p):
        z = dt(0)
        vs = np.where(p.valid, p.v_sigma, z)                 # (exp(-sigma) may overflow where sigma < 0)
        wb = np.where(p.valid, p.alpha_b * p.T_before, z)
        vop = np.where(p.valid, p.e, z) * p.v_alpha
        if clamp_zeroes_grad:
            vop = np.where(p.av < dt(alpha_clamp_bwd), vop, z)
        vx, vy = vs * p.dx, vs * p.dy
        terms = np.stack([vx, vy, vx * p.dx, vx * p.dy, vy * p.dy, wb * p.vo[:, 0], wb * p.vo[:, 1], wb * p.vo[:, 2],
                          vop])
        if chunks is None:
            raw[p.g] += terms.sum(1)
        else:
            chunks[p.g].append(terms)
        raw_abs[p.g] += np.abs(terms).sum(1)

    w = A.walk(sc, v_img, v_alpha_img, alpha_clamp_bwd, clamp_zeroes_grad, on_pair=on_pair, on_tile=on_tile,
               id_range=id_range, dtype=dtype, exp=exp, opacities=opac_p, sigma_adjacent=True)
    pix = dict(img=img, alpha=alpha, depth=depth)
    pix_s = dict(img=img_s, alpha=alpha_s, depth=depth_s)
    runs = []
    for order in orders or ():
        r = np.zeros((n, 9), dt)
        for g in range(n):
            if not chunks[g]:
                continue
            if order == "tree":
                r[g] = _tree_sum(chunks[g])
            else:
                x = np.concatenate(chunks[g], 1)
                x = x[:, np.random.default_rng([order, g]).permutation(x.shape[1])]
                r[g] = np.cumsum(x, 1, dtype=dt)[:, -1]       # one after the other, each addition rounded to `dt`
        runs.append({**pix, **_finish(sc, r, raw_abs, opac_p, dt)[0]})
    val, scale = _finish(sc, raw, raw_abs, opac_p, dt)
    if runs:
        val = runs[0]                                        # (`val` of an emulation is its first order)
    return SimpleNamespace(val={**pix, **val}, scale={**pix_s, **scale}, runs=runs, adjacent=w.adjacent,
                           adjacent_px=w.adjacent_px, visible=w.visible, n_stopped=w.n_stopped, list_len=w.list_len,
                           walk_len=w.walk_len, depth_max=float(np.abs(depths).max()))


@lru_cache(maxsize=None)
def reference(block=16, alpha_clamp_bwd=0.99, id_range=None, logit=False, clamp_zeroes_grad=False, seed=SEED,
              shared_logits_of=None):
    """(scene, float64 definition) for the loss sum(img w_img) + sum(alpha w_alpha) of the scene's own weights; computed
    once per argument tuple and shared: callers leave both unchanged."""
    sc = make_scene(seed, block, shared_logits_of)
    return sc, definition(sc, sc.w_img, sc.w_alpha, alpha_clamp_bwd, clamp_zeroes_grad, id_range, logit)


@lru_cache(maxsize=None)
def views_reference(block=16, alpha_clamp_bwd=0.99):
    """The batched-views contract: B = 2 scenes sharing the opacity logits; per view its own definition (logit route),
    `v_logit` / its scale summed over the views.  -> ([(scene, definition)] per view, v_logit [N], scale [N])."""
    views = [reference(block, alpha_clamp_bwd, None, True), reference(block, alpha_clamp_bwd, None, True, False,
                                                                      SEED_VIEW2, SEED)]
    return (views, sum(r.val["v_logit"] for _s, r in views), sum(r.scale["v_logit"] for _s, r in views))


def emulate(block=16, alpha_clamp_bwd=0.99, hw_exp=False, logit=False, n_random=8):
    """The float32 emulation of `reference(block, alpha_clamp_bwd, logit=logit)`: one `val` dict per summation order."""
    sc = make_scene(SEED, block)
    return definition(sc, sc.w_img, sc.w_alpha, alpha_clamp_bwd, False, None, logit, np.float32,
                      hardware_exp(1000 + block) if hw_exp else rounded_exp, ["tree"] + list(range(n_random))).runs


def compare(got, ref, name, keep=None, scale=None, exp=None):
    """One output against the definition, per element: -> (worst ratio |got - exp| / (2^-24 scale) over the kept
    elements with a scale > 0, number of kept elements with scale == 0 whose value is not exactly 0.0).
    `keep`: bool over rows / pixels (broadcast over components)."""
    got = np.asarray(got, np.float64)
    exp = ref.val[name] if exp is None else exp
    scale = ref.scale[name] if scale is None else scale
    got = got.reshape(exp.shape)
    keep = np.ones(exp.shape[:1] if exp.ndim <= 2 and name not in PIXEL_OUTPUTS else exp.shape[:2], bool) \
        if keep is None else keep
    keep = np.broadcast_to(keep.reshape(keep.shape + (1,) * (exp.ndim - keep.ndim)), exp.shape)
    pos = keep & (scale > 0)
    ratio = float((np.abs(got - exp)[pos] / (EPS * scale[pos])).max()) if pos.any() else 0.0
    return ratio, int((keep & (scale == 0) & (got != 0)).sum())

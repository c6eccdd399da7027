"""numpy restatement of the LiDAR depth contract (include/sgn_rast.h "LiDAR DEPTH", csrc/lidar_depth.hip) and the inputs
the LiDAR depth tests share.

* `splat` / `filter_returns`: the target in float32 with the contract's operation order — the bit-exact reference of the
  HIP kernels.  The projection is `seed_oracle.classify` (the seeding contract), the rest a per-pixel minimum.
* `loss64`: loss, count, per-pixel gradients and the metrics in float64 from the float32 inputs; `loss32` restates the
  forward value with the kernels' float32 per-pixel terms (summed in float64, as the kernels sum them).
* `splat_scene`, `loss_inputs`: the generated inputs of tests/test_gpu_lidar_depth.py; tests/test_lidar_depth_oracle.py
  holds them to the conditions the GPU tolerances rest on.
"""
import functools

import numpy as np

import seed_oracle as SO

F32 = np.float32
ALPHA_MIN = F32(1e-3)
KINDS = {"l1": 0, "inverse": 1}
SPLAT_SIZES = (1, 257, 5000)
MAX_DEPTH = 30.0


# ---------------------------------------------------------------- target

def counted_points(sc, max_depth=np.inf):
    """(counted [n] bool, u, v, z = pc.z float32) of one sweep against the scene's camera."""
    c = SO.classify(sc["points"], sc["l2w"], np.zeros((0, 15), F32), sc["w2c"], sc["fx"], sc["fy"], sc["cx"], sc["cy"],
                    sc["width"], sc["height"], min_z=sc["min_z"], dtype=F32)
    with np.errstate(invalid="ignore"):
        counted = c["ok"] & (c["pcz"] <= F32(max_depth))
    return counted, c["u"], c["v"], c["pcz"].astype(F32), c


def begin(height, width):
    return np.full((height, width), np.inf, dtype=F32)


def splat(sc, depth, max_depth=np.inf):
    """One sweep into `depth` (in place): the nearest counted return per pixel."""
    counted, u, v, z, _ = counted_points(sc, max_depth)
    np.minimum.at(depth, (v[counted], u[counted]), z[counted])
    return depth


def filter_returns(depth, radius, rel_tol):
    """out [H,W] float32: 0 without a return; a return z is kept iff z * (1 - rel_tol) <= the minimum return over the
    (2 radius + 1)^2 window clipped to the image; the product is one float32 multiply by the float32 constant."""
    H, W = depth.shape
    keep = F32(1.0) - F32(rel_tol)
    pad = np.full((H + 2 * radius, W + 2 * radius), np.inf, dtype=F32)
    pad[radius:radius + H, radius:radius + W] = depth
    m = np.full((H, W), np.inf, dtype=F32)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            m = np.minimum(m, pad[dy:dy + H, dx:dx + W])
    with np.errstate(invalid="ignore"):
        kept = np.isfinite(depth) & ((depth * keep).astype(F32) <= m)
    return np.where(kept, depth, F32(0)).astype(F32)


def splat_depth(scenes, radius=2, rel_tol=0.05, max_depth=np.inf):
    d = begin(scenes[0]["height"], scenes[0]["width"])
    for sc in scenes:
        splat(sc, d, max_depth)
    return filter_returns(d, radius, rel_tol)


def _to_lidar(sc, pc):
    """Camera-frame points (float64 [k,3]) -> LiDAR-frame float32 rows, through the scene's float32 matrices."""
    V, Lm = sc["w2c"].astype(np.float64), sc["l2w"].astype(np.float64)
    pw = (pc - V[:, 3]) @ np.linalg.inv(V[:, :3]).T
    return ((pw - Lm[:, 3]) @ np.linalg.inv(Lm[:, :3]).T).astype(F32)


@functools.lru_cache(maxsize=None)
def splat_scene(n, seed=31):
    """The seed oracle's street-like sweep (treat as read-only) with its NaN rows, points behind the camera, rows with
    z <= min_z and returns past MAX_DEPTH — and, from n = 257 on, planted rows: two returns in column 0 through
    fu in (-1, 0), and one row twice (two points with equal z on one pixel).  Returns (scene, planted) with `planted` the
    row indices {"fu_neg": [..], "twin": [a, b]}."""
    sc = dict(SO.scene(n, 0, seed))
    pts = sc["points"].copy()
    planted = {}
    if n == 1:
        pts[0] = (10.0, 0.5, 0.25)                  # one live, visible point
    else:
        ray = lambda u, v, z: [(u - sc["cx"]) / sc["fx"] * z, (v - sc["cy"]) / sc["fy"] * z, z]
        pts[0:2] = _to_lidar(sc, np.array([ray(-0.5, 20.5, 8.0), ray(-0.25, 60.5, 12.0)]))
        pts[2] = _to_lidar(sc, np.array([ray(40.5, 30.5, 9.0)]))[0]
        pts[3] = pts[2]
        planted = {"fu_neg": [0, 1], "twin": [2, 3]}
    sc["points"] = pts
    return sc, planted


# ---------------------------------------------------------------- loss

def counted_pixels(dsum, alpha, target, mask=None):
    """The contract's rule on the float32 inputs (the comparisons are exact in any precision)."""
    with np.errstate(invalid="ignore"):
        c = (target > 0) & (alpha > ALPHA_MIN) & (dsum > 0)
    if mask is not None:
        c = c & (np.asarray(mask).reshape(c.shape) != 0)
    return c


def loss64(dsum, alpha, target, mask=None, kind="l1", v_loss=1.0):
    """Everything in float64 from the float32 inputs: loss, count, v_dsum / v_alpha per pixel, D, the metrics."""
    s, a, z = (np.asarray(t, dtype=F32).astype(np.float64) for t in (dsum, alpha, target))
    c = counted_pixels(np.asarray(dsum, F32), np.asarray(alpha, F32), np.asarray(target, F32), mask)
    n = int(c.sum())
    with np.errstate(all="ignore"):
        D = np.where(c, s / np.where(c, a, 1.0), 1.0)
        zz = np.where(c, z, 1.0)
        res = (D - zz) if kind == "l1" else (1.0 / D - 1.0 / zz)
        res = np.where(c, res, 0.0)
        g = float(v_loss) / max(n, 1)
        sg = np.sign(res)
        v_dsum = g * sg / np.where(c, a, 1.0) if kind == "l1" else -g * sg / (D * D) / np.where(c, a, 1.0)
        v_dsum = np.where(c, v_dsum, 0.0)
        v_alpha = np.where(c, -v_dsum * D, 0.0)
        e = np.where(c, np.abs(D - zz), 0.0)
        ratio = np.maximum(D / zz, zz / D)
    m = max(n, 1)
    metrics = {"abs_rel": float((e / zz).sum() / m), "rmse": float(np.sqrt((e * e).sum() / m)), "mae": float(e.sum() / m),
               "delta1": float((c & (ratio < 1.25)).sum() / m), "count": n}
    return dict(loss=float(np.abs(res).sum() / m), count=n, v_dsum=v_dsum, v_alpha=v_alpha, counted=c,
                D=np.where(c, D, 0.0), residual=res, metrics=metrics)


def loss32(dsum, alpha, target, mask=None, kind="l1"):
    """The forward value as the kernels form it: float32 per-pixel terms, a float64 sum, one rounding of the mean."""
    s, a, z = (np.asarray(t, dtype=F32) for t in (dsum, alpha, target))
    c = counted_pixels(s, a, z, mask)
    one = F32(1)
    with np.errstate(all="ignore"):
        D = (s / a).astype(F32)
        res = (D - z) if kind == "l1" else ((one / D).astype(F32) - (one / z).astype(F32))
        l = np.where(c, np.abs(res.astype(F32)), F32(0))
    n = int(c.sum())
    return F32(l.astype(np.float64).sum() / max(n, 1)), n


def sign_ambiguous(o64, target):
    """Counted pixels whose residual's sign float32 may decide differently: D is off z, but by no more than 2^-22 z.
    (D == z exactly is not ambiguous: the correctly rounded float32 quotient of an exactly representable result is that
    result, so both precisions see a zero residual.)"""
    z = np.asarray(target, F32).astype(np.float64)
    d = np.abs(o64["D"] - z)
    return o64["counted"] & (d > 0) & (d <= 2.0 ** -22 * z)


LOSS_SHAPES = ((37, 53), (1, 1))


@functools.lru_cache(maxsize=None)
def loss_inputs(h, w, seed=5):
    """dict(dsum, alpha, target, mask, equal) of float32 / uint8 / bool arrays (treat as read-only).

    alpha in [0.05, 1] plus a band at or below 1e-3; z in [1, 80] with a third of the pixels 0; D = z (1 + r) with
    1e-3 <= |r| <= 0.15, or 0.3 <= |r| <= 0.4 for a tenth of them (so that delta1 < 1), well clear of the delta1
    thresholds r = 0.25 and r = -0.2; a few pixels with dsum <= 0; `equal` marks the exact-equality pixels: alpha in
    {0.5, 0.25} and dsum = z alpha (a power-of-two scaling, exact), so that dsum / alpha == z exactly in float32."""
    rng = np.random.default_rng(seed)
    shape = (h, w)
    alpha = rng.uniform(0.05, 1.0, shape).astype(F32)
    z = rng.uniform(1.0, 80.0, shape).astype(F32)
    mag = np.where(rng.random(shape) < 0.1, rng.uniform(0.3, 0.4, shape), rng.uniform(1e-3, 0.15, shape))
    r = np.where(rng.random(shape) < 0.5, mag, -mag)
    dsum = (z.astype(np.float64) * (1.0 + r) * alpha.astype(np.float64)).astype(F32)
    pick = rng.random(shape)
    if h * w > 1:
        band = pick < 0.06                              # alpha at or below the validity threshold
        alpha[band] = rng.choice(np.array([1e-3, 5e-4, 0.0], F32), int(band.sum()))
        bad = (pick >= 0.06) & (pick < 0.08)            # dsum <= 0
        dsum[bad] = rng.choice(np.array([0.0, -1.5], F32), int(bad.sum()))
        equal = (pick >= 0.08) & (pick < 0.12)
        alpha[equal] = rng.choice(np.array([0.5, 0.25], F32), int(equal.sum()))
        dsum[equal] = z[equal] * alpha[equal]
        z[(pick >= 0.12) & (pick < 0.12 + 0.88 / 3)] = 0    # a third: no return
    else:
        equal = np.zeros(shape, bool)
    mask = rng.choice(np.array([0, 1, 255], np.uint8), shape, p=[0.3, 0.4, 0.3])
    if h * w == 1:
        mask[:] = 1
    return dict(dsum=dsum, alpha=alpha, target=z, mask=mask, equal=equal)


def uncounted_inputs(h=9, w=7, seed=6):
    """An image without a single counted pixel: every pixel fails one of the three rules."""
    d = {k: v.copy() for k, v in loss_inputs(37, 53, seed).items()}
    d = {k: v[:h, :w].copy() for k, v in d.items()}
    which = np.arange(h * w).reshape(h, w) % 3
    d["target"][which == 0] = 0
    d["alpha"][which == 1] = ALPHA_MIN
    d["dsum"][which == 2] = 0
    return d

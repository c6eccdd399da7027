"""numpy restatement of the LiDAR seeding contract (include/sgn_rast.h "LiDAR SEEDING", csrc/seed.hip) and the scenes the
seeding tests share.

`classify` runs the contract's arithmetic in the dtype it is given: float32 with exactly the contract's operation order
(every product and sum is a separate float32 numpy operation, so nothing is contracted or reassociated) — the bit-exact
reference of the HIP kernels — or float64 on the same float32 inputs, which is what the reference's scripts compute in.
`partition` turns the per-point verdicts into the stable output segments.  `adjacent` marks the points whose verdict may
legitimately differ between the two precisions.
"""
import functools

import numpy as np

# (n points, n boxes, seed): the generated scenes of tests/test_gpu_seed.py; tests/test_seed_oracle.py holds each of them
# to the "at most 1 % threshold-adjacent live points" condition
SCENES = [(1, 1, 11), (63, 0, 12), (65, 7, 13), (4099, 7, 14), (20000, 64, 15)]
ACC_SCENES = [(3000, 5, 100 + i) for i in range(6)]      # 3 sweeps x 2 cameras of the accumulator test

WIDTH, HEIGHT = 160, 96


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_boxes(centers, rots, extents, scale=1.1):
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(rots, dtype=np.float64).reshape(-1, 9)
    e = np.asarray(extents, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([c, r, e * (scale * 0.5)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(n, n_boxes, seed, width=WIDTH, height=HEIGHT, focal=120.0, cx=79.3, cy=47.6):
    """A street-like sweep: dict of float32 inputs (treat as read-only: the result is cached and shared)."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-5.0, 45.0, n), rng.uniform(-15.0, 15.0, n), rng.uniform(-2.6, 4.0, n)], axis=1)
    # LiDAR -> world: a fixed axis permutation (x <-> y, z negated) and a small rotation
    perm = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    R_l2w = _rot([0.3, -0.5, 0.8], 0.04) @ perm
    t_l2w = np.array([12.5, -7.25, 3.0])
    # camera 1.5 m up, looking along LiDAR +x (camera x = -y_lidar, y = -z_lidar, z = x_lidar), tilted a little
    R_c2l = _rot([0.2, 1.0, 0.1], 0.02) @ np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    t_c2l = np.array([0.0, 0.0, 1.5])
    R_c2w, t_c2w = R_l2w @ R_c2l, R_l2w @ t_c2l + t_l2w
    w2c = np.concatenate([R_c2w.T, (-R_c2w.T @ t_c2w)[:, None]], axis=1)
    centers_l, yaws, extents = [], [], []
    for b in range(n_boxes):
        x = rng.uniform(6.0, 40.0)
        c = np.array([x, rng.uniform(-0.5, 0.5) * x, rng.uniform(0.2, 1.2)])
        if b == 1:                                  # boxes 0 and 1 overlap
            c = centers_l[0] + np.array([0.8, 0.5, 0.1])
        centers_l.append(c)
        yaws.append(rng.uniform(-np.pi, np.pi))
        extents.append([rng.uniform(3.6, 5.6), rng.uniform(1.4, 2.2), rng.uniform(1.6, 2.4)])
    centers_l = np.array(centers_l).reshape(-1, 3)
    extents = np.array(extents).reshape(-1, 3)
    rots_l = [_rot([0, 0, 1], y) for y in yaws]
    plant = min(200, n // (2 * n_boxes)) if n_boxes else 0
    if plant:
        rows = rng.choice(n, plant * n_boxes, replace=False)
        for b in range(n_boxes):
            loc = rng.uniform(-1.2, 1.2, (plant, 3)) * (extents[b] * 0.55)
            pts[rows[b * plant:(b + 1) * plant]] = centers_l[b] + loc @ rots_l[b].T
    pts = pts.astype(np.float32)
    nan_rows = np.nonzero(rng.random(n) < 0.02)[0]
    pts[nan_rows, rng.integers(0, 3, nan_rows.size)] = np.nan
    boxes = make_boxes(centers_l @ R_l2w.T + t_l2w, [R_l2w @ r for r in rots_l], extents) if n_boxes \
        else np.zeros((0, 15), np.float32)
    return dict(points=pts, l2w=np.concatenate([R_l2w, t_l2w[:, None]], axis=1).astype(np.float32), boxes=boxes,
                w2c=w2c.astype(np.float32), fx=focal, fy=focal, cx=cx, cy=cy, width=width, height=height,
                min_z=-2.0, centers_lidar=centers_l.astype(np.float32))


@functools.lru_cache(maxsize=None)
def image(seed, height=HEIGHT, width=WIDTH):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def _affine(M, x, y, z):
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]


def classify(points, l2w, boxes, w2c, fx, fy, cx, cy, width, height, min_z=-2.0, dtype=np.float32, **_):
    """The per-point verdicts of the contract, computed in `dtype` from the float32 inputs."""
    T = dtype
    P = np.asarray(points, dtype=np.float32).astype(T)
    L, V, B = np.asarray(l2w, np.float32).astype(T), np.asarray(w2c, np.float32).astype(T), np.asarray(boxes, np.float32).astype(T)
    fx, fy, cx, cy = (T(np.float32(v)) for v in (fx, fy, cx, cy))
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        live = ~np.isnan(P).any(axis=1) & (z > T(np.float32(min_z)))
        pw = _affine(L, x, y, z)
        live &= ~(np.abs(pw[0]) > T(1e5))
        pc = _affine(V, pw[0], pw[1], pw[2])
        fu = (fx * pc[0] + cx * pc[2]) / pc[2]
        fv = (fy * pc[1] + cy * pc[2]) / pc[2]
        tu, tv = np.trunc(fu), np.trunc(fv)
        visible = (pc[2] > 0) & np.isfinite(fu) & np.isfinite(fv) & (tu >= 0) & (tu < width) & (tv >= 0) & (tv < height)
        ok = live & visible
        u = np.where(ok, tu, 0).astype(np.int64)
        v = np.where(ok, tv, 0).astype(np.int64)
        inside = np.zeros((P.shape[0], B.shape[0]), dtype=bool)
        loc = np.zeros((P.shape[0], B.shape[0], 3), dtype=T)
        for b in range(B.shape[0]):
            c, R, h = B[b, 0:3], B[b, 3:12].reshape(3, 3), B[b, 12:15]
            d = [pw[k] - c[k] for k in range(3)]
            for k in range(3):
                loc[:, b, k] = (R[0, k] * d[0] + R[1, k] * d[1]) + R[2, k] * d[2]
            inside[:, b] = (np.abs(loc[:, b, 0]) <= h[0]) & (np.abs(loc[:, b, 1]) <= h[1]) & (np.abs(loc[:, b, 2]) <= h[2])
    return dict(live=live, ok=ok, u=u, v=v, inside=inside, member=inside & ok[:, None], loc=loc,
                pw=np.stack(pw, axis=1), pcz=pc[2], fu=fu, fv=fv, half=B[:, 12:15])


def partition(cls, img):
    """The stable output segments: object rows box after box, background rows, totals (box counts, background, live)."""
    n, nb = cls["member"].shape
    idx = np.arange(n)
    rgb = img[cls["v"], cls["u"]]
    local, o_rgb, o_src, offsets = [], [], [], [0]
    for b in range(nb):
        rows = idx[cls["member"][:, b]]
        local.append(cls["loc"][rows, b]); o_rgb.append(rgb[rows]); o_src.append(rows)
        offsets.append(offsets[-1] + rows.size)
    bg = idx[cls["ok"] & ~cls["inside"].any(axis=1)]
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
    T = cls["loc"].dtype
    return dict(local=cat(local, (0, 3), T), obj_rgb=cat(o_rgb, (0, 3), np.uint8), obj_src=cat(o_src, (0,), np.int64),
                offsets=offsets, world=cls["pw"][bg], bg_rgb=rgb[bg], bg_src=bg,
                totals=[offsets[b + 1] - offsets[b] for b in range(nb)] + [int(bg.size), int(cls["live"].sum())])


def seed_sweep(sc, img, dtype=np.float32):
    return partition(classify(dtype=dtype, **sc), img)


def adjacent(c64):
    """Threshold-adjacent points, from the float64 verdicts: within 5e-5 of a box face or of the camera plane, or a
    pixel coordinate within 5e-4 of an integer.  Only these may be classified differently in float32."""
    with np.errstate(all="ignore"):
        face = (np.abs(np.abs(c64["loc"]) - c64["half"][None]) < 5e-5).any(axis=(1, 2))
        plane = np.abs(c64["pcz"]) < 5e-5
        edge = (np.abs(c64["fu"] - np.rint(c64["fu"])) < 5e-4) | (np.abs(c64["fv"] - np.rint(c64["fv"])) < 5e-4)
    return face | plane | edge


def differs(c32, c64):
    """Points whose verdict (live, visible, pixel, membership) is not the same in the two precisions."""
    px = c32["ok"] & c64["ok"] & ((c32["u"] != c64["u"]) | (c32["v"] != c64["v"]))
    return (c32["live"] != c64["live"]) | (c32["ok"] != c64["ok"]) | px | (c32["member"] != c64["member"]).any(axis=1)

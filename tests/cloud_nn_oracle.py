"""fp64 brute-force nearest neighbour ACROSS two clouds (test infrastructure): for every row of `query` the smallest
|q - t_j| over all rows j of `target` and that j, chunked over query rows like knn_oracle.knn_brute; the chamfer pair of
the reference (geometric_metric.py:59-69: two means over CD_UNIT); numpy restatements of the two LiDAR row filters
(:36-48) and of the world -> scene arithmetic (:86-92); and the seeded cloud pairs the two-cloud tests run on."""
from __future__ import annotations

import numpy as np

import knn_oracle as KO

CD_UNIT = 1e-4


def nearest_brute(query, target, chunk: int = 512):
    """(dist [Nq] float64, idx [Nq] int64): direct differences in float64, the first of equal distances."""
    q = np.asarray(query, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    assert q.ndim == 2 and t.ndim == 2 and q.shape[1] == 3 and t.shape[1] == 3 and t.shape[0] >= 1
    out_d = np.empty(q.shape[0])
    out_i = np.empty(q.shape[0], dtype=np.int64)
    for s in range(0, q.shape[0], chunk):
        c = q[s:s + chunk]
        d2 = np.zeros((c.shape[0], t.shape[0]))
        for a in range(3):                                     # direct differences, no |a|^2 + |b|^2 - 2ab
            diff = c[:, a, None] - t[None, :, a]
            diff *= diff
            d2 += diff
        j = np.argmin(d2, axis=1)
        out_i[s:s + j.size] = j
        out_d[s:s + j.size] = np.sqrt(d2[np.arange(j.size), j])
    return out_d, out_i


def chamfer(pred, gt):
    """(d1, d2): mean nearest distance pred -> gt and gt -> pred, each over CD_UNIT."""
    return nearest_brute(pred, gt)[0].mean() / CD_UNIT, nearest_brute(gt, pred)[0].mean() / CD_UNIT


def filter_lidar(points, ignore_nan=True, filter_ego=True):
    """Rows with a NaN dropped; then rows strictly inside the ego box -1 < x < 3, |y| < 1, -1 < z < 2 dropped."""
    p = np.asarray(points)
    if ignore_nan:
        p = p[~np.isnan(p).any(axis=1)]
    if filter_ego:
        inside = (p[:, 0] > -1) & (p[:, 0] < 3) & (np.abs(p[:, 1]) < 1) & (p[:, 2] > -1) & (p[:, 2] < 2)
        p = p[~inside]
    return p


def lidar_to_scene(points, translation, transform, scale):
    """float64: (p + (ty, tx, -tz)) R^T + T, times scale, with [R | T] the first three rows of `transform`."""
    p = np.asarray(points, dtype=np.float64)
    tx, ty, tz = np.asarray(translation, dtype=np.float64)
    m = np.asarray(transform, dtype=np.float64)
    return ((p + np.array([ty, tx, -tz])) @ m[:3, :3].T + m[:3, 3]) * float(scale)


def evaluate_lidar_geometric(means, lidar_points, translation, transform, scale):
    lidar = lidar_to_scene(filter_lidar(np.asarray(lidar_points, dtype=np.float64)), translation, transform, scale)
    d1, d2 = chamfer(means, lidar)
    return {"lidar_chamfer_distance_1": d1, "lidar_chamfer_distance_2": d2, "lidar_chamfer_distance_avg": (d1 + d2) / 2}


def lattice_pair():
    """A 10^3 integer lattice and the same lattice shifted by (0.5, 0, 0): every nearest distance is 0.5 both ways."""
    a = np.arange(10)
    t = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return t + np.array([0.5, 0, 0], dtype=np.float32), t


def asymmetric_pair():
    """pred = {(0,0,0), (4,0,0)}, gt = {(0,0,0), (0,3,0), (1,0,0), (0,0,12)}.
    pred -> gt: 0 and 3 (to (1,0,0)), mean 1.5;  gt -> pred: 0, 3, 1, 12, mean 4."""
    pred = np.array([[0, 0, 0], [4, 0, 0]], dtype=np.float32)
    gt = np.array([[0, 0, 0], [0, 3, 0], [1, 0, 0], [0, 0, 12]], dtype=np.float32)
    return pred, gt, 1.5 / CD_UNIT, 4.0 / CD_UNIT


def cloud(name: str) -> np.ndarray:
    """float32 [N,3]: the clouds of knn_oracle plus a few of this module's own (seeded)."""
    g = np.random.default_rng(20_240)
    if name == "uniform_10k":
        x = g.random((10_037, 3)) * 10                       # N not a multiple of 64
    elif name == "uniform_20k":
        x = np.random.default_rng(20_241).random((20_000, 3)) * 10
    elif name == "coplanar_lattice":                         # a plane through lattice cells: mass ties against "lattice"
        uv = g.random((5_000, 2)) * 26
        x = np.stack([uv[:, 0], uv[:, 1], np.full(5_000, 12.5)], 1)
    elif name == "collinear_5k":
        x = KO.cloud("collinear")[:5_000]
    elif name == "far":                                      # 1e4 away from everything in [0, 10]^3
        x = g.random((3_000, 3)) * 10 + 1e4
    elif name.startswith("uniform_n"):                       # uniform_n<N>: N points in [0, 10]^3
        x = np.random.default_rng(int(name[9:])).random((int(name[9:]), 3)) * 10
    elif name == "street_jitter":                            # the Gaussians-vs-LiDAR shape: street_1m, every point moved
        x = KO.cloud("street_1m") + np.random.default_rng(20_242).normal(0, 0.05, (1_000_000, 3))
    else:
        return KO.cloud(name)
    return np.ascontiguousarray(x, dtype=np.float32)


def lidar_scene(seed: int = 5):
    """A raw LiDAR cloud with NaN rows, ego-box rows and rows exactly on the ego box's faces, a set of Gaussian
    centres near its transformed image, and a non-trivial translation / rotation / scale."""
    g = np.random.default_rng(seed)
    world = g.uniform(-40, 40, (6_000, 3)) * np.array([1, 1, 0.1])
    world[::97, g.integers(0, 3)] = np.nan
    world[5::53] = g.uniform([-1, -1, -1], [3, 1, 2], (len(world[5::53]), 3))      # inside the ego box
    world[:6] = [[3, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 2], [0, 0, -1]]   # on its faces: kept
    translation = np.array([12.5, -7.25, 3.0])
    ax = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    th = 0.7
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    rot = np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)
    transform = np.concatenate([rot, np.array([[1.5], [-2.0], [0.25]])], 1)
    scale = 0.0375
    scene = lidar_to_scene(filter_lidar(world), translation, transform, scale)
    means = (scene[::2] + g.normal(0, 0.01, scene[::2].shape)).astype(np.float32)
    return means, world, translation, transform, scale

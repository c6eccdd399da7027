"""fp64 brute-force k-nearest neighbours (test infrastructure): for every row i the k smallest |x_i - x_j| over
j != i, ascending, and those j.  Chunked over query rows so that N = 20 000 runs in seconds.  Also the clouds the
k-NN tests run on (deterministic, seeded)."""
from __future__ import annotations

import numpy as np


def knn_brute(x, k: int, chunk: int = 1024, rows=None):
    """(dist [R,k] float64 ascending, idx [R,k] int64) for query rows `rows` (default: all) of x [N,3]."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    assert n > k
    out_d = np.empty((rows.size, k))
    out_i = np.empty((rows.size, k), dtype=np.int64)
    for s in range(0, rows.size, chunk):
        r = rows[s:s + chunk]
        diff = x[r, None, :] - x[None, :, :]               # direct differences, no |a|^2 + |b|^2 - 2ab
        d2 = np.einsum("ijk,ijk->ij", diff, diff)
        d2[np.arange(r.size), r] = np.inf                  # j != i
        part = np.argpartition(d2, k - 1, axis=1)[:, :k]
        pd = np.take_along_axis(d2, part, 1)
        order = np.argsort(pd, axis=1, kind="stable")
        out_i[s:s + r.size] = np.take_along_axis(part, order, 1)
        out_d[s:s + r.size] = np.sqrt(np.take_along_axis(pd, order, 1))
    return out_d, out_i


def cloud(name: str, seed: int = 0) -> np.ndarray:
    """float32 [N,3] point clouds: typical and adversarial shapes for the search."""
    g = np.random.default_rng(seed)
    if name == "uniform":
        x = g.random((100_000, 3))
    elif name.startswith("street"):
        n = 1_000_000 if name == "street_1m" else 200_000
        x = street(n, g)
    elif name == "identical":
        x = np.tile(np.array([[1.5, -2.25, 3.0]]), (50_000, 1))
    elif name == "repeat5":
        x = np.repeat(g.random((4_000, 3)) * 10, 5, axis=0)
        x = x[g.permutation(x.shape[0])]
    elif name == "collinear":
        t = g.random(20_000)
        x = np.stack([t, 2 * t, -t], 1) * 50
    elif name == "coplanar":
        uv = g.random((20_000, 2)) * 10
        x = np.stack([uv[:, 0], uv[:, 1], np.full(20_000, 0.75)], 1)
    elif name == "lattice":
        a = np.arange(27)
        x = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)   # 19 683 points, mass ties
    elif name == "two_clusters":
        x = g.normal(size=(20_000, 3))
        x[10_000:] += 1e4
    elif name == "ragged":
        x = g.random((10_000 + 37, 3))          # N not a multiple of 64
    elif name.startswith("tiny"):                # tiny<k>: N = k + 1
        x = g.random((int(name[4:]) + 1, 3))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, dtype=np.float32)


def street(n: int, g) -> np.ndarray:
    """Street-like: a ground plane with density ~ 1/r^2 around the road, thin clutter above it, 5 % far outliers
    (1e3 x further out)."""
    n_out = n // 20
    m = n - n_out
    r = np.exp(g.uniform(np.log(1.0), np.log(80.0), m))           # 1/r^2 areal density
    th = g.uniform(0, 2 * np.pi, m)
    z = np.where(g.random(m) < 0.7, g.normal(0, 0.02, m), g.uniform(0, 4, m))
    core = np.stack([r * np.cos(th), r * np.sin(th), z], 1)
    d = g.normal(size=(n_out, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = d * g.uniform(1e4, 8e4, (n_out, 1))
    return np.concatenate([core, far])[g.permutation(n)]

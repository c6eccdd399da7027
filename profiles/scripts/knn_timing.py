"""k-nearest-neighbour timing (csrc/knn.hip via sgn_rast.knn.k_nearest) on the MI355X: device-event time after warm-up
for 1 M and 4 M uniform and street-like points at k = 3, visited / N (candidate distances per query) there and on the
adversarial clouds of tests/knn_oracle.py at k = 1, 3, 8, 16, and sklearn's time (NearestNeighbors(k + 1), as the
reference calls it) on the same host for the 1 M clouds when sklearn is importable.  Prints one JSON line.

    python profiles/scripts/knn_timing.py [--reps 10] [--no-sklearn] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "street-gaussians-ns_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import knn_oracle as KO  # noqa: E402
from sgn_rast import knn  # noqa: E402


def make(name, n, seed=0):
    g = np.random.default_rng(seed)
    x = g.random((n, 3)) * 100 if name == "uniform" else KO.street(n, g)
    return np.ascontiguousarray(x, dtype=np.float32)


def gpu_time(xd, k, reps):
    for _ in range(3):
        knn.k_nearest(xd, k)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    ms = []
    for r in range(reps):
        ev[2 * r].record()
        knn.k_nearest(xd, k)
        ev[2 * r + 1].record()
    torch.cuda.synchronize()
    ms = [ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(reps)]
    return float(np.median(ms)), float(np.min(ms))


def visited_per_point(xd, k):
    v = torch.zeros(1, dtype=torch.int64, device=xd.device)
    knn.k_nearest(xd, k, visited=v)
    return round(int(v.item()) / xd.shape[0], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "knn_timing needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "k": 3, "timing": {}, "visited_adversarial": {}}
    for name in ("uniform", "street"):
        for n in (1 << 20, 1 << 22):
            x = make(name, n)
            xd = torch.from_numpy(x).cuda()
            med, mn = gpu_time(xd, 3, a.reps)
            row = {"n": n, "gpu_ms_median": round(med, 3), "gpu_ms_min": round(mn, 3),
                   "visited_per_point": visited_per_point(xd, 3)}
            if n == 1 << 20 and not a.no_sklearn:
                try:
                    from sklearn.neighbors import NearestNeighbors
                    t0 = time.perf_counter()
                    NearestNeighbors(n_neighbors=4, algorithm="auto", metric="euclidean").fit(x).kneighbors(x)
                    row["sklearn_s"] = round(time.perf_counter() - t0, 3)
                    row["speedup"] = round(row["sklearn_s"] * 1e3 / med, 1)
                except ImportError:
                    row["sklearn_s"] = None
            res["timing"][f"{name}_{n}"] = row
            del xd
    for name in ("identical", "repeat5", "collinear", "coplanar", "lattice", "two_clusters", "ragged", "uniform",
                 "street", "street_1m"):
        xd = torch.from_numpy(KO.cloud(name)).cuda()
        res["visited_adversarial"][name] = {k: visited_per_point(xd, k) for k in (1, 3, 8, 16)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Two-cloud nearest-neighbour timing (csrc/cloud_nn.hip via sgn_rast.geometry.nearest) on the MI355X: device-event time
after warm-up, median of --reps, for 1 M street-like points against a jittered copy of themselves (the
Gaussians-vs-LiDAR shape) and for 1 M against 4 M street-like points, each in both directions (a chamfer distance needs
both), with visited / n_query there, sgn_knn's time (k = 3 and k = 1) on the same targets beside them, and
visited / n_query on every pair of tests/test_gpu_cloud_nn.py.  Prints one JSON line.

    python profiles/scripts/cloud_nn_timing.py [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "street-gaussians-ns_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cloud_nn_oracle as CO  # noqa: E402
import knn_oracle as KO  # noqa: E402
from sgn_rast import geometry, knn  # noqa: E402


def gpu_time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for r in range(reps):
        ev[2 * r].record()
        fn()
        ev[2 * r + 1].record()
    torch.cuda.synchronize()
    ms = [ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(reps)]
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)


def visited_per_query(qd, td):
    v = torch.zeros(1, dtype=torch.int64, device=qd.device)
    geometry.nearest(qd, td, visited=v)
    return round(int(v.item()) / qd.shape[0], 2)


def knn_visited_per_point(xd, k):
    v = torch.zeros(1, dtype=torch.int64, device=xd.device)
    knn.k_nearest(xd, k, visited=v)
    return round(int(v.item()) / xd.shape[0], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cloud_nn_timing needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "timing": {}, "knn": {}, "visited_test_pairs": {}}

    street_1m = torch.from_numpy(CO.cloud("street_1m")).cuda()
    jitter_1m = torch.from_numpy(CO.cloud("street_jitter")).cuda()
    street_4m = torch.from_numpy(np.ascontiguousarray(KO.street(1 << 22, np.random.default_rng(1)),
                                                      dtype=np.float32)).cuda()
    pairs = {"street_1m->jitter_1m": (street_1m, jitter_1m), "jitter_1m->street_1m": (jitter_1m, street_1m),
             "street_1m->street_4m": (street_1m, street_4m), "street_4m->street_1m": (street_4m, street_1m)}
    for name, (qd, td) in pairs.items():
        med, mn = gpu_time(lambda: geometry.nearest(qd, td), a.reps)
        res["timing"][name] = {"n_query": qd.shape[0], "n_target": td.shape[0], "gpu_ms_median": med, "gpu_ms_min": mn,
                               "visited_per_query": visited_per_query(qd, td)}
    for name, xd in (("jitter_1m", jitter_1m), ("street_1m", street_1m), ("street_4m", street_4m)):
        row = {"n": xd.shape[0]}
        for k in (1, 3):
            med, mn = gpu_time(lambda: knn.k_nearest(xd, k), a.reps)
            row[f"k{k}"] = {"gpu_ms_median": med, "gpu_ms_min": mn, "visited_per_point": knn_visited_per_point(xd, k)}
        res["knn"][name] = row
    del street_4m, pairs

    import test_gpu_cloud_nn as T
    for qn, tn in T._both(T.SMALL_PAIRS) + T.LARGE_PAIRS:
        qd, td = torch.from_numpy(CO.cloud(qn)).cuda(), torch.from_numpy(CO.cloud(tn)).cuda()
        res["visited_test_pairs"][f"{qn}->{tn}"] = visited_per_query(qd, td)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

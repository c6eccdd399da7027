"""The visibility-gated Adam step against the dense one, at the headline's parameter set: 1 M Gaussians, SH degree 3
(means, scales, quats, opacity, features_dc [N,1,3], features_rest [N,15,3]: 59 floats per Gaussian, 944 MB of
parameter + gradient + moments, well past the 256 MiB Infinity Cache).

Both C entries are called directly (ctypes, arrays built once), so the host costs ~10 us per call and the device events
time the kernels.  One sample = CALLS back-to-back calls between two device events; after a warm-up of every variant
the variants are sampled round-robin, REPEATS times (alternating repeats: drift and neighbours hit all variants alike).
Reported: the median per call and the min..max of the samples.

Visibility: int32 radii, visible rows placed at random or in contiguous runs of 4096 rows, at fractions 1.0 / 0.5 / 0.25
/ 0.1 (exact counts).  Run from the repository root:  python profiles/scripts/selective_adam_timing.py [--json FILE]
"""
import argparse
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, "street-gaussians-ns_amd")
from sgn_rast import _lib as L  # noqa: E402

DEV, N, RUN = "cuda", 1_000_000, 4096
CALLS, REPEATS = 20, 9
FRACTIONS = (1.0, 0.5, 0.25, 0.1)
SHAPES = {"means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacity": (N, 1), "features_dc": (N, 1, 3),
          "features_rest": (N, 15, 3)}
LRS = {"means": 1.6e-4, "scales": 0.005, "quats": 0.001, "opacity": 0.05, "features_dc": 0.0025, "features_rest": 0.0025 / 20}


def radii(fraction, placement, gen):
    """int32 [N]: round(fraction x N) rows (random) or round(fraction x runs) runs of 4096 rows (runs) hold a radius > 0."""
    vis = torch.zeros(N, dtype=torch.bool)
    if placement == "random":
        vis[torch.randperm(N, generator=gen)[: round(fraction * N)]] = True
    else:
        runs = (N + RUN - 1) // RUN
        on = torch.zeros(runs, dtype=torch.bool)
        on[torch.randperm(runs, generator=gen)[: round(fraction * runs)]] = True
        vis = on.repeat_interleave(RUN)[:N]
    r = torch.where(vis, torch.randint(1, 50, (N,), generator=gen, dtype=torch.int32), torch.zeros((), dtype=torch.int32))
    return r.to(DEV), float(vis.float().mean())


def make_call(lib, names, T, vis):
    """A closure that steps the tensors ``names`` once: dense (vis None) or gated by the radii ``vis``."""
    n = len(names)
    ptrs = lambda k: (C.c_void_p * n)(*[T[name][k].data_ptr() for name in names])
    dbl = lambda v: (C.c_double * n)(*v)
    head = (n, ptrs(0), ptrs(1), ptrs(2), ptrs(3), (C.c_int64 * n)(*[T[name][0].numel() for name in names]),
            dbl([LRS[name] for name in names]), dbl([0.9] * n), dbl([0.999] * n), dbl([1e-15] * n), (C.c_int64 * n)(*[100] * n))
    stream = L.stream_ptr()
    if vis is None:
        return lambda: L.check(lib.sgn_adam_step(*head, stream), "sgn_adam_step")
    tail = ((C.c_int64 * n)(*[N] * n), (C.c_void_p * n)(*[vis.data_ptr()] * n), (C.c_int32 * n)(*[2] * n))
    return lambda: L.check(lib.sgn_adam_step_visible(*head, *tail, stream), "sgn_adam_step_visible")


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS              # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = L.load()
    gen = torch.Generator().manual_seed(0)
    dgen = torch.Generator(DEV).manual_seed(0)
    rnd = lambda s, scale: scale * torch.randn(*s, device=DEV, generator=dgen)
    # param, grad, exp_avg, exp_avg_sq
    T = {k: (rnd(s, 1.0), rnd(s, 1e-3), rnd(s, 1e-3), rnd(s, 1e-3) ** 2) for k, s in SHAPES.items()}
    masks = {(f, pl): radii(f, pl, gen) for f in FRACTIONS for pl in ("random", "runs")}
    groups = {"all six": list(SHAPES)}
    groups.update({k: [k] for k in SHAPES})
    variants = {}
    for gname, names in groups.items():
        variants[(gname, "dense", None)] = make_call(lib, names, T, None)
        for (f, pl), (r, _actual) in masks.items():
            variants[(gname, pl, f)] = make_call(lib, names, T, r)
    for fn in variants.values():                           # warm-up: every variant, code objects and caches
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, fn in variants.items():
            samples[k].append(sample(fn))
    med = {k: statistics.median(v) for k, v in samples.items()}
    floats = {g: sum(T[k][0].numel() for k in names) for g, names in groups.items()}

    print(f"{N} Gaussians, {CALLS} calls per sample, {REPEATS} alternating samples; us per call, median (min..max)")
    cell = lambda k: f"{med[k]:7.1f} ({min(samples[k]):.1f}..{max(samples[k]):.1f})"
    for gname in groups:
        d = med[(gname, "dense", None)]
        print(f"\n## {gname}: {floats[gname] / 1e6:.0f} M floats, dense sgn_adam_step {cell((gname, 'dense', None))} us"
              f" = {floats[gname] * 28 / d / 1e6:.2f} TB/s of the 28 B/element stream")
        print("| visible fraction | random: us | vs dense | runs of 4096: us | vs dense |")
        print("|---|---|---|---|---|")
        for f in FRACTIONS:
            a, b = (gname, "random", f), (gname, "runs", f)
            print(f"| {f:g} (actual {masks[(f, 'random')][1]:.3f} / {masks[(f, 'runs')][1]:.3f}) | {cell(a)} | {med[a] / d:.3f} |"
                  f" {cell(b)} | {med[b] / d:.3f} |")
        # break-even under random placement: where the line between two measured fractions crosses the dense time
        pts = sorted((f, med[(gname, "random", f)]) for f in FRACTIONS)
        even = None
        for (f0, t0), (f1, t1) in zip(pts, pts[1:]):
            if (t0 - d) * (t1 - d) <= 0 and t0 != t1:
                even = f0 + (d - t0) * (f1 - f0) / (t1 - t0)
        where = (f"{even:.2f} (linear between the measured fractions)" if even is not None else
                 ("below 0.1: no measured fraction is faster than dense" if pts[0][1] > d else "above 1.0: every measured fraction is faster"))
        print(f"break-even fraction, random placement: {where}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"n": N, "calls": CALLS, "repeats": REPEATS,
                       "samples_us": {"|".join(str(x) for x in k): v for k, v in samples.items()}}, fh, indent=1)


if __name__ == "__main__":
    main()

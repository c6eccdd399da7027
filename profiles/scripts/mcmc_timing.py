"""The MCMC refinement's two costs at the headline's parameter set (1 M Gaussians, SH degree 3), profiles/mcmc.md:

1. ``sgn_mcmc_noise``, the per-step pass, called directly (ctypes) beside the dense six-tensor ``sgn_adam_step`` of
   profiles/selective_adam.md, re-measured here: one sample = CALLS back-to-back calls between two device events,
   the two sampled round-robin REPEATS times after a warm-up; median and min..max per call, and the noise's implied
   GB/s against its 56 B per row (44 read, 12 written).
2. One relocate + grow (5 % dead rows, growth 1.05) through ``MCMCDensifier._phase``: the HIP engine against the torch
   engine on the same device, each on a fresh copy of the same world, a host clock around the call ending in a device
   synchronise (the phases read their totals back, so the host is part of the cost); median of REPEATS after a warm-up.

Run from the repository root:  python profiles/scripts/mcmc_timing.py [--json FILE]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, "street-gaussians-ns_amd")
from sgn_rast import _lib as L, mcmc  # noqa: E402
from sgn_rast.optim import FusedAdam  # noqa: E402

DEV, N = "cuda", 1_000_000
CALLS, REPEATS = 20, 9
SHAPES = {"means": (N, 3), "log_scales": (N, 3), "quats": (N, 4), "opacity_logits": (N, 1), "features_dc": (N, 1, 3),
          "features_rest": (N, 15, 3)}
LRS = {"means": 1.6e-4, "log_scales": 0.005, "quats": 0.001, "opacity_logits": 0.05, "features_dc": 0.0025,
       "features_rest": 0.0025 / 20}


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS              # us per call


def world(gen):
    P = {k: torch.randn(*s, device=DEV, generator=gen) for k, s in SHAPES.items()}
    P["log_scales"] = -4.0 + 0.5 * P["log_scales"]
    logits = 2.0 * P["opacity_logits"]
    dead = torch.rand(N, 1, device=DEV, generator=gen) < 0.05
    P["opacity_logits"] = torch.where(dead, torch.full_like(logits, -6.0), logits.clamp(min=-4.0))
    return P


def refine_once(P0, engine):
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    opt = {k: FusedAdam([P[k]], lr=LRS[k], eps=1e-15) for k in P}
    for k in P:
        opt[k].state[P[k]] = dict(step=torch.tensor(1.0), exp_avg=torch.zeros_like(P[k]) + 1e-3,
                                  exp_avg_sq=torch.zeros_like(P[k]) + 1e-6)
    D = mcmc.MCMCDensifier(P, opt, mcmc.MCMCConfig(cap_max=2 * N), seed=1, engine=engine)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        relocated = D._phase(600, mcmc.RELOCATE)
        added = D._phase(600, mcmc.GROW)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, relocated, added          # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = L.load()
    gen = torch.Generator(DEV).manual_seed(0)
    P0 = world(gen)

    # 1. the per-step noise beside the dense Adam step
    T = {k: (P0[k].clone(), 1e-3 * torch.randn_like(P0[k]), 1e-3 * torch.randn_like(P0[k]),
             (1e-3 * torch.randn_like(P0[k])) ** 2) for k in SHAPES}
    names, n = list(SHAPES), len(SHAPES)
    ptrs = lambda k: (C.c_void_p * n)(*[T[name][k].data_ptr() for name in names])
    dbl = lambda v: (C.c_double * n)(*v)
    head = (n, ptrs(0), ptrs(1), ptrs(2), ptrs(3), (C.c_int64 * n)(*[T[name][0].numel() for name in names]),
            dbl([LRS[name] for name in names]), dbl([0.9] * n), dbl([0.999] * n), dbl([1e-15] * n), (C.c_int64 * n)(*[100] * n))
    stream = L.stream_ptr()
    key = mcmc.phase_key(1, 600, mcmc.NOISE)
    noise_args = (N, key, 1.6e-4 * 5e5, T["means"][0].data_ptr(), T["log_scales"][0].data_ptr(),
                  T["quats"][0].data_ptr(), T["opacity_logits"][0].data_ptr(), None, stream)
    variants = {"sgn_adam_step (dense, six tensors)": lambda: L.check(lib.sgn_adam_step(*head, stream), "sgn_adam_step"),
                "sgn_mcmc_noise": lambda: L.check(lib.sgn_mcmc_noise(*noise_args), "sgn_mcmc_noise")}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, fn in variants.items():
            samples[k].append(sample(fn))
    print(f"{N} Gaussians, {CALLS} calls per sample, {REPEATS} alternating samples; us per call, median (min..max)")
    for k, v in samples.items():
        print(f"{k}: {statistics.median(v):.1f} ({min(v):.1f}..{max(v):.1f}) us")
    t_noise = statistics.median(samples["sgn_mcmc_noise"])
    print(f"sgn_mcmc_noise: {N * 56 / t_noise / 1e3:.0f} GB/s of its 56 B per row")

    # 2. one relocate + grow, HIP engine against the torch engine on the device
    refine = {}
    for engine in ("hip", "torch"):
        refine_once(P0, engine)                                          # warm-up
    for _ in range(REPEATS):
        for engine in ("hip", "torch"):
            refine.setdefault(engine, []).append(refine_once(P0, engine))
    for engine, v in refine.items():
        ms = [x[0] for x in v]
        print(f"relocate + grow, engine={engine}: {statistics.median(ms):.2f} ({min(ms):.2f}..{max(ms):.2f}) ms; "
              f"{v[0][1]} relocated, {v[0][2]} added")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"n": N, "calls": CALLS, "repeats": REPEATS, "kernel_us": samples,
                       "refine_ms": {k: [x[0] for x in v] for k, v in refine.items()}}, fh, indent=1)


if __name__ == "__main__":
    main()

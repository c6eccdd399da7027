"""Time one densifying refinement (step 45 of tests/golden/make_densify_reference.py's configuration: split + duplicate
+ every cull) per engine of sgn_rast.densify on street-scale inputs at SH degree 3 with Adam state present: device events
around `refinement_after` after a warm-up call, every call on a fresh copy of the inputs, the arms alternating; the number
of implicit host synchronisations (torch's sync debug mode) and, with --profile, of kernel launches and copies
(torch.profiler).  --parts 9 splits the Gaussians over nine sub-models of one SceneGraphDensifier.  --parent PATH adds
the torch engine of another densify.py (the commit before the HIP engine) as the baseline arm.

    python profiles/scripts/densify_refine_timing.py --n 1000000 --parts 1 --out profiles/densify_refine_timing.jsonl"""
import argparse
import importlib.util
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "street-gaussians-ns_amd"), os.path.join(ROOT, "tests", "golden")]
import make_densify_reference as M  # noqa: E402
from sgn_rast import densify, scenes  # noqa: E402



def load_parent(path):
    spec = importlib.util.spec_from_file_location("sgn_rast._parent_densify", path)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    return parent


DEV = torch.device("cuda", 0)


def world(n, seed):
    raw = scenes.make_gaussians(n, scenes.make_camera(96, 64, 80.0), seed=seed, z_range=(1.0, 5.0), sh_degree=3)
    g = torch.Generator().manual_seed(seed + 5)
    stats = (torch.rand(n, generator=g) * 0.0004, torch.randint(1, 6, (n,), generator=g).float(),
             torch.rand(n, generator=g) * 0.12)
    raw = {k: v.to(DEV) for k, v in raw.items()}
    state = {k: (torch.randn_like(v) * 1e-3, torch.rand_like(v) * 1e-6) for k, v in raw.items()}
    return raw, state, tuple(t.to(DEV) for t in stats)


def make(mod, worlds, engine):
    kw = {} if engine is None else {"engine": engine}
    models = [{k: torch.nn.Parameter(v.clone()) for k, v in raw.items()} for raw, _, _ in worlds]
    opts = {k: torch.optim.Adam([m[k] for m in models], lr=1e-3, eps=1e-15) for k in densify.PARAM_NAMES}
    for m, (_, state, _) in zip(models, worlds):
        for k in m:
            opts[k].state[m[k]] = {"step": torch.tensor(7.0), "exp_avg": state[k][0].clone(), "exp_avg_sq": state[k][1].clone()}
    cfg = mod.DensifyConfig(num_train_data=M.NUM_TRAIN, **M.CFG)
    G = mod.SceneGraphDensifier(models, opts, cfg, seed=M.SEED, **kw)
    for part, (_, _, stats) in zip(G.parts, worlds):
        part.last_size = (64, 96)
        part.stats.xys_grad_norm, part.stats.vis_counts, part.stats.max_2Dsize = (t.clone() for t in stats)
    return G


def one(mod, worlds, engine, step=45):
    G = make(mod, worlds, engine)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    G.refinement_after(step)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, sum(m["means"].shape[0] for m in G.models)


def syncs(mod, worlds, engine):
    G = make(mod, worlds, engine)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        G.refinement_after(45)
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(x.message).lower() for x in w)


def launches(mod, worlds, engine):
    from torch.profiler import ProfilerActivity, profile
    G = make(mod, worlds, engine)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        G.refinement_after(45)
        torch.cuda.synchronize()
    kernels = memcpy = 0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                memcpy += 1
            else:
                kernels += 1
    return kernels, memcpy


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--parts", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default="profiles/densify_refine_timing.jsonl")
    a = ap.parse_args()
    sizes = [a.n // a.parts + (1 if i < a.n % a.parts else 0) for i in range(a.parts)]
    worlds = [world(n, 20 + i) for i, n in enumerate(sizes)]
    arms = (("torch", densify, "torch"), ("hip", densify, "hip"))
    if a.parent:
        arms = (("parent_torch", load_parent(a.parent), None),) + arms
    res = {"n": a.n, "parts": a.parts, "device": torch.cuda.get_device_name(0)}
    if a.profile:
        for name, mod, eng in arms:
            one(mod, worlds, eng)
            res[name] = dict(zip(("kernel_launches", "memcpy_memset"), launches(mod, worlds, eng)))
    else:
        for name, mod, eng in arms:
            one(mod, worlds, eng)                                   # warm-up
        times = {name: [] for name, _, _ in arms}
        for _ in range(a.reps):                                     # alternate the arms
            for name, mod, eng in arms:
                ev, wall, n_out = one(mod, worlds, eng)
                times[name].append((ev, wall))
                res.setdefault("n_out", {})[name] = n_out
        for name, mod, eng in arms:
            res[name] = {"event_ms": [round(t[0], 3) for t in times[name]], "wall_ms": [round(t[1], 3) for t in times[name]],
                         "implicit_host_syncs": syncs(mod, worlds, eng)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")

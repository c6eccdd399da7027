"""Freezes what the REFERENCE's own densification computes (`refinement_after` / `split_gaussians` / `dup_gaussians` /
`cull_gaussians` / `dup_in_optim` / `remove_from_optim`, sgn_splatfacto.py:459-720), executed literally from the
reference checkout through tests/refhost.py (nothing is copied), on the inputs of tests/test_densify_reference.py: the
point count and every new parameter and Adam moment, for every step the test takes, in
tests/golden/densify_reference.npz.  Most output rows are bit-exact copies of input rows (kept or duplicated
Gaussians), so each array is stored as `src` — per output row, the input row it copies, or -1 — and `new`, the values of
the other rows (split samples, reset opacities and moments); `load()` rebuilds the arrays from `world()`'s inputs.  The
test compares `sgn_rast.densify.Densifier` against this file on any machine, and where the checkout exists also against
the reference run again, bit for bit.

Run from the repo root where the reference checkout exists:  python tests/golden/make_densify_reference.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "street-gaussians-ns_amd"), os.path.join(ROOT, "tests")]

OUT = os.path.join(HERE, "densify_reference.npz")
STEPS = (15, 45, 40, 100)
REF2OURS = dict(means="means", scales="log_scales", quats="quats", features_dc="features_dc",
                features_rest="features_rest", opacities="opacity_logits")
CFG = dict(warmup_length=0, refine_every=10, reset_alpha_every=3, cull_alpha_thresh=0.08, densify_grad_thresh=0.004,
           densify_size_thresh=0.04, cull_scale_thresh=0.09, stop_split_at=1000, stop_screen_size_at=400)
SEED, NUM_TRAIN = 11, 2


def world(n=1500, seed=0):
    """Parameters, Adam moments (exp_avg, exp_avg_sq) and per-Gaussian statistics both sides start from."""
    from sgn_rast import scenes
    cam = scenes.make_camera(96, 64, 80.0)
    raw = scenes.make_gaussians(n, cam, seed=seed, z_range=(1.0, 5.0))
    g = torch.Generator().manual_seed(seed + 5)
    state = {k: (torch.randn(v.shape, generator=g) * 1e-3, torch.rand(v.shape, generator=g) * 1e-6)
             for k, v in raw.items()}
    stats = (torch.rand(n, generator=g) * 0.0004, torch.randint(1, 6, (n,), generator=g).float(),
             torch.rand(n, generator=g) * 0.12)
    return raw, state, stats


def reference_outcome(step):
    """The reference's `refinement_after(opt, step)`, literally: {"num_points", "<ours>/param|exp_avg|exp_avg_sq"}."""
    import refhost
    ns = refhost.load("oracle")
    raw, state, stats = world()
    model = refhost.build_single(ns, raw, sky_res=0, step=step, **CFG)
    model.num_train_data = NUM_TRAIN
    model._model_idx_in_scene_graph = 0
    groups = model.get_param_groups()
    opt = ns.Optimizers({k: {"optimizer": ns.AdamOptimizerConfig(lr=1e-3, eps=1e-15)} for k in groups}, groups)
    for ref_name, ours in REF2OURS.items():
        p = model.gauss_params[ref_name]
        opt.optimizers[ref_name].state[p] = {"step": torch.tensor(7.0), "exp_avg": state[ours][0].clone(),
                                             "exp_avg_sq": state[ours][1].clone()}
    model.xys_grad_norm, model.vis_counts, model.max_2Dsize = (t.clone() for t in stats)
    model.last_size = (64, 96)
    torch.manual_seed((SEED * 1_000_003 + step) & 0x7FFFFFFFFFFFFFFF)       # the stream Densifier draws from
    with refhost.cpu_as_cuda():
        model.refinement_after(opt, step)
    assert model.xys_grad_norm is None
    out = {"num_points": np.asarray(model.num_points, dtype=np.int64)}
    for ref_name, ours in REF2OURS.items():
        p = model.gauss_params[ref_name]
        st = opt.optimizers[ref_name].state[p]
        out[f"{ours}/param"] = p.detach().numpy().copy()
        out[f"{ours}/exp_avg"] = st["exp_avg"].numpy().copy()
        out[f"{ours}/exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
    return out


def _inputs() -> dict:
    """The arrays each output array's rows are copied from: {"<ours>/param|exp_avg|exp_avg_sq": numpy array}."""
    raw, state, _ = world()
    out = {}
    for k, v in raw.items():
        out[f"{k}/param"], out[f"{k}/exp_avg"], out[f"{k}/exp_avg_sq"] = v.numpy(), state[k][0].numpy(), state[k][1].numpy()
    return out


def encode(outcome: dict) -> dict:
    """{"num_points", "<key>/src", "<key>/new"}: src[i] = the input row output row i is a bit-exact copy of, or -1;
    new = the rows with src -1, in order."""
    inputs, enc = _inputs(), {"num_points": outcome["num_points"]}
    for key, a in outcome.items():
        if key == "num_points":
            continue
        first = {}
        for i, row in enumerate(inputs[key]):
            first.setdefault(row.tobytes(), i)
        src = np.array([first.get(row.tobytes(), -1) for row in a], dtype=np.int32)
        enc[f"{key}/src"], enc[f"{key}/new"] = src, a[src < 0]
    return enc


def decode(enc: dict) -> dict:
    inputs, out = _inputs(), {"num_points": enc["num_points"]}
    for key in inputs:
        src, new = enc[f"{key}/src"], enc[f"{key}/new"]
        a = np.empty((src.shape[0],) + inputs[key].shape[1:], dtype=inputs[key].dtype)
        a[src >= 0] = inputs[key][src[src >= 0]]
        a[src < 0] = new
        out[key] = a
    return out


def load(step) -> dict:
    """The frozen outcome of one step, in the form reference_outcome() returns."""
    with np.load(OUT) as z:
        pre = f"{step}/"
        return decode({k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})


if __name__ == "__main__":
    frozen = {}
    for s in STEPS:
        outcome = reference_outcome(s)
        enc = encode(outcome)
        back = decode(enc)
        assert all(np.array_equal(back[k], v) and back[k].dtype == v.dtype for k, v in outcome.items()), s
        frozen.update({f"{s}/{k}": v for k, v in enc.items()})
    np.savez_compressed(OUT, **frozen)
    print(OUT, os.path.getsize(OUT), "bytes")

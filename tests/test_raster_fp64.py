"""CPU: the float64 definition the per-row / per-pixel GPU test of the rasterizer compares against
(`tests/raster_fp64.py`) held to float64 autograd through the torch oracle on all four leaves and both images, the C
oracle — an independent float32 implementation — held to the very per-row bound the GPU gets, the derivation of that
bound's K from the float32 emulation, and the conditions the GPU comparison relies on, asserted and not measured."""
import numpy as np
import pytest
import torch

import raster_fp64 as R

BLOCKS = [16, 8, 5]


def _t(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dt is None else t.to(dt)


@pytest.mark.parametrize("block", BLOCKS)
def test_definition_is_the_oracles_autograd(block, torch_oracle):
    """Self-consistent clamp (0.999 both ways, autograd zeroes the gradient where it is active): image, alpha and the
    gradients of xys, conics, colours and opacities equal float64 autograd through the torch oracle — gradients to 1e-9
    of the ROW's absolute sum, images to 1e-12.  (Both sides are float64, as in test_absgrad_fp64.py.)"""
    sc, ref = R.reference(block, 0.999, clamp_zeroes_grad=True)
    D = torch.float64
    leaves = [_t(a, D).requires_grad_(True) for a in (sc.xys, sc.conics, sc.colors, sc.opacities)]
    img, alpha = torch_oracle.rasterize_gaussians(
        leaves[0], _t(sc.depths), _t(sc.radii), leaves[1], _t(sc.num_tiles_hit), leaves[2], leaves[3], sc.H, sc.W,
        block, background=_t(sc.background, D), return_alpha=True)
    ((img * _t(sc.w_img, D)).sum() + (alpha * _t(sc.w_alpha, D)).sum()).backward()
    assert np.abs(img.detach().numpy() - ref.val["img"]).max() <= 1e-12
    assert np.abs(alpha.detach().numpy() - ref.val["alpha"]).max() <= 1e-12
    for name, leaf in zip(("v_xy", "v_conic", "v_colors", "v_opacity"), leaves):
        got, exp, scale = leaf.grad.numpy().reshape(ref.val[name].shape), ref.val[name], ref.scale[name]
        assert np.isfinite(got).all()
        worst = float((np.abs(got - exp) / np.where(scale > 0, scale, 1.0))[scale > 0].max())
        print(f"[raster fp64] block {block}: {name} vs oracle autograd (both float64): worst |err| / row scale {worst:.2e}")
        assert worst <= 1e-9, (name, worst)
        assert (got[scale == 0] == 0).all() and (exp[scale == 0] == 0).all()


def _c_oracle_outputs(c_oracle, sc, clamp):
    xys, conics, colors, opac = _t(sc.xys), _t(sc.conics), _t(sc.colors), _t(sc.opacities)
    bg = _t(sc.background)
    _cum, _k, _v, _ks, ids, bins = c_oracle.bin_and_sort(xys, _t(sc.depths), _t(sc.radii), _t(sc.num_tiles_hit), sc.H,
                                                        sc.W, sc.block)
    img, fT, fi = c_oracle.raster_fwd(sc.H, sc.W, sc.block, ids, bins, xys, conics, colors, opac, bg)
    v_xy, v_conic, v_col, v_op = c_oracle.raster_bwd(sc.H, sc.W, sc.block, ids, bins, xys, conics, colors, opac, bg, fT,
                                                     fi, _t(sc.w_img), _t(sc.w_alpha), clamp)
    return dict(img=img.numpy(), alpha=(1 - fT).numpy(), v_xy=v_xy.numpy(), v_conic=v_conic.numpy(),
                v_colors=v_col.numpy(), v_opacity=v_op.numpy().reshape(-1))


def _worst(runs, ref, names):
    """{name: worst ratio over the runs} on the rows / pixels that are not threshold-adjacent; exact zeros asserted."""
    out = {}
    for name in names:
        keep = ~ref.adjacent_px if name in R.PIXEL_OUTPUTS else ~ref.adjacent
        res = [R.compare(run[name], ref, name, keep) for run in runs]
        assert all(nonzero == 0 for _r, nonzero in res), (name, "a row / pixel nothing reaches is not exactly 0.0")
        out[name] = max(r for r, _n in res)
    return out


C_NAMES = ("img", "alpha", "v_xy", "v_conic", "v_colors", "v_opacity")


@pytest.mark.parametrize("block", BLOCKS)
def test_c_oracle_is_within_the_per_row_bound(block, c_oracle):
    """Upstream's clamp (0.99 in the backward, not zeroing): the C oracle passes the GPU tests' bound, K included."""
    sc, ref = R.reference(block, 0.99)
    worst = _worst([_c_oracle_outputs(c_oracle, sc, 0.99)], ref, C_NAMES)
    print(f"[raster fp64] block {block}: C oracle worst ratios " + ", ".join(f"{k} {v:.1f}" for k, v in worst.items()))
    for name, r in worst.items():
        assert r <= R.K[name], (name, r, R.K[name])


@pytest.mark.parametrize("hw_exp", [False, True], ids=["exact-exp", "hardware-exp"])
def test_k_is_four_times_the_emulations_worst_ratio(hw_exp, c_oracle):
    """The derivation of K / K_HW: the float32 emulation (tree order + 8 random orders, blocks 16 / 8 / 5, and the logit
    route at block 16) and the C oracle; K = 4 x the worst ratio rounded up to a power of two."""
    worst = {}
    for block, logit in [(b, False) for b in BLOCKS] + [(16, True)]:
        sc, ref = R.reference(block, 0.99, None, logit)
        w = _worst(R.emulate(block, 0.99, hw_exp, logit), ref, R.PIXEL_OUTPUTS + R.ROW_OUTPUTS)
        print(f"[raster fp64] emulation, block {block}{', logits' if logit else ''}, "
              f"{'hardware' if hw_exp else 'exact'} exp: " + ", ".join(f"{k} {v:.1f}" for k, v in w.items()))
        if not logit:                       # (K_HW is never below K: the C oracle counts for both)
            c = _worst([_c_oracle_outputs(c_oracle, sc, 0.99)], ref, C_NAMES)
            w = {k: max(v, c.get(k, 0.0)) for k, v in w.items()}
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    table = R.K_HW if hw_exp else R.K
    for name, r in worst.items():
        k = 2.0 ** np.ceil(np.log2(4.0 * r))
        print(f"[raster fp64] {'K_HW' if hw_exp else 'K'}[{name}]: worst {r:.2f} -> {k:.0f} (constant {table[name]})")
        assert 4.0 * r <= table[name], (name, r, table[name])
        assert table[name] <= 2 * k, (name, "the constant is looser than its derivation", r, table[name])


@pytest.mark.parametrize("block", BLOCKS)
def test_conditions_of_the_gpu_comparison(block):
    """Few threshold-adjacent rows and pixels, a pixel that stops, the never-visible rows, scales that dominate — for
    every scene and clamp the GPU tests use."""
    cases = [("view 0", R.reference(block, 0.99)), ("view 0, clamp 0.999", R.reference(block, 0.999)),
             ("view 0, logits", R.reference(block, 0.99, None, True)),
             ("view 1, logits", R.reference(block, 0.99, None, True, False, R.SEED_VIEW2, R.SEED)),
             ("id range", R.reference(block, 0.99, R.ID_RANGE)), ("id window", R.reference(block, 0.99, R.ID_WINDOW))]
    for what, (sc, ref) in cases:
        n_vis, n_adj = int(ref.visible.sum()), int((ref.adjacent & ref.visible).sum())
        n_px = int(ref.adjacent_px.sum())
        print(f"[raster fp64] block {block}, {what}: {n_adj} adjacent of {n_vis} visible Gaussians, {n_px} adjacent "
              f"pixels of {sc.H * sc.W}, {ref.n_stopped} stopped, longest list {ref.list_len.max()}")
        assert n_adj <= 0.02 * n_vis and n_px <= 0.01 * sc.H * sc.W
        assert ref.n_stopped >= 1 or what == "id range"          # (a condition of the whole scenes)
        edge_vis = ref.visible[sc.n_base:]
        if not what.startswith("id "):
            assert n_vis >= 250 and (~edge_vis).sum() >= 5           # opacity < 1/255 (3 rows) and logit -12 (2 rows)
            assert not edge_vis[[4, 5, 6, 11, 12]].any() and edge_vis[[0, 1, 2, 3, 7, 9, 13, 15, 18, 19, 20, 21]].all()
        else:
            lo, hi = R.ID_RANGE if what == "id range" else R.ID_WINDOW
            assert not ref.visible[:lo].any() and not ref.visible[hi:].any() and n_vis >= 50
            assert (hi - lo < 0.5 * sc.n) == (what == "id window")          # the library's list-window threshold
        # scale: every absolute sum dominates its signed sum (a wrong scale would make the GPU bound vacuous), and
        # vanishes exactly where nothing is visible
        for name in R.PIXEL_OUTPUTS + R.ROW_OUTPUTS + ("moments", "v_colors_pre"):
            assert (ref.scale[name] >= np.abs(ref.val[name])).all(), name
            assert np.isfinite(ref.val[name]).all() and np.isfinite(ref.scale[name]).all(), name
        for name in ("moments", "v_xy", "v_conic", "v_colors", "v_opacity"):
            assert (ref.scale[name][~ref.visible] == 0).all() and (ref.scale[name][ref.visible].max(-1) > 0).all()
        # the last-pixel row: one valid pixel, so every sum IS its one term
        last = sc.n_base + 18
        if not what.startswith("id "):
            assert np.allclose(np.abs(ref.val["moments"][last]), ref.scale["moments"][last], rtol=1e-12)
    # the scene reaches the kernels' routes: lists past the thresholds the GPU tests set, colours clamped at 0
    sc, ref = cases[0][1]
    assert ref.list_len.max() >= 32 and (ref.walk_len >= 16).any() and ((ref.walk_len > 0) & (ref.walk_len < 16)).any()
    assert (sc.colors_pre < 0).any() and (sc.colors >= 0).all()
    assert sc.depths[sc.n_base + 19] == sc.depths[sc.n_base + 20]

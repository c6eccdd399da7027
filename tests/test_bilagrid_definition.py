"""CPU: the written-out float64 definition of the bilateral-grid slice (tests/bilagrid_fp64.py) is the textbook
formulation — ``F.grid_sample(align_corners=True, padding_mode="border")`` over the ``[1,12,L,Hg,Wg]`` volume on
(x, y, luma) in [0,1]^3, then the 3x4 affine — in value (1e-12) and in both gradients (float64 autograd of that
formulation), and ``total_variation`` is what a 2 x 2 x 2 grid gives by hand."""
import pytest
import torch
import torch.nn.functional as F

import bilagrid_fp64 as B

SHAPES = [(4, 3, 5, 13, 17), (1, 1, 1, 7, 9), (1, 3, 4, 11, 6), (5, 1, 1, 9, 8), (8, 16, 16, 19, 23)]


def textbook(grid, rgb):
    """float64, differentiable: grid [L,Hg,Wg,12], rgb [H,W,3] -> out [H,W,3]."""
    H, W, _ = rgb.shape
    x = ((torch.arange(W, dtype=torch.float64) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, dtype=torch.float64) + 0.5) / H)[:, None].expand(H, W)
    luma = B.LUMA[0] * rgb[..., 0] + B.LUMA[1] * rgb[..., 1] + B.LUMA[2] * rgb[..., 2]
    coords = torch.stack([x, y, luma], -1) * 2 - 1                               # grid_sample's [-1, 1]
    vol = grid.permute(3, 0, 1, 2)[None]                                         # [1,12,L,Hg,Wg]
    A = F.grid_sample(vol, coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] * rgb[..., None, :]).sum(-1) + A[..., 3]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_helper_is_grid_sample_plus_affine(shape):
    L, Hg, Wg, H, W = shape
    grid, rgb, v_out = B.make_case(L, Hg, Wg, H, W, seed=3)
    g64 = grid.double().requires_grad_(True)
    p64 = rgb.double().requires_grad_(True)
    ref = textbook(g64, p64)
    out = B.slice_fwd(grid, rgb)
    assert float((out - ref.detach()).abs().max()) <= 1e-12
    ref.backward(v_out.double())
    v_rgb, v_grid = B.slice_bwd(grid, rgb, v_out)
    assert float((v_rgb - p64.grad).abs().max()) <= 1e-12 * max(1.0, float(p64.grad.abs().max()))
    assert float((v_grid - g64.grad).abs().max()) <= 1e-12 * max(1.0, float(g64.grad.abs().max()))


def test_input_hits_both_clamps_and_keeps_off_the_kinks():
    grid, rgb, _ = B.make_case(8, 16, 16, 37, 53, seed=1)
    luma = (rgb.double() * torch.tensor(B.LUMA, dtype=torch.float64)).sum(-1)
    assert bool((luma == 0).any()) and bool((luma > 1).any()) and bool(((luma > 0) & (luma < 1)).any())
    gz = luma[luma > 0] * 7
    assert float((gz - gz.round()).abs().min()) >= 1e-3


def test_float32_evaluation_is_close_but_not_equal():
    grid, rgb, v_out = B.make_case(4, 3, 5, 13, 17, seed=5)
    err = float((B.slice_fwd(grid, rgb, torch.float32).double() - B.slice_fwd(grid, rgb)).abs().max())
    assert 0 < err < 1e-5


def test_identity_grid_is_exact_in_the_helper():
    _, rgb, _ = B.make_case(4, 3, 5, 13, 17, seed=5)
    eye = torch.tensor([1., 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]).expand(4, 3, 5, 12)
    assert torch.equal(B.slice_fwd(eye, rgb, torch.float32), rgb)


def test_total_variation_by_hand():
    from sgn_rast.appearance import BilateralGrids, total_variation
    g = torch.zeros(1, 2, 2, 2, 12)
    g[0, 1] += 1.0            # a step of 1 along L: every forward difference along L is 1, none along Hg or Wg
    assert float(total_variation(g)) == pytest.approx(1.0, abs=1e-7)
    g[0, :, 1] += 2.0         # and a step of 2 along Hg
    assert float(total_variation(g)) == pytest.approx(1.0 + 4.0, abs=1e-6)
    g = torch.randn(3, 2, 2, 2, 12, generator=torch.Generator().manual_seed(0))
    assert float(total_variation(g)) == pytest.approx(B.total_variation(g), rel=1e-5)
    # singleton axes drop out; the per-image affine has no prior at all
    g1 = torch.randn(2, 1, 3, 1, 12, generator=torch.Generator().manual_seed(1))
    assert float(total_variation(g1)) == pytest.approx(B.total_variation(g1), rel=1e-5)
    with torch.no_grad():
        assert float(total_variation(BilateralGrids(4, (1, 1, 1)))) == 0.0
        assert float(total_variation(BilateralGrids(2))) == 0.0    # identity everywhere


def test_module_layout_round_trip():
    from sgn_rast.appearance import BilateralGrids
    m = BilateralGrids(3, (5, 4, 2))                                 # (Wg, Hg, L), gsplat's order
    assert tuple(m.grids.shape) == (3, 2, 4, 5, 12) and m.grids.requires_grad
    eye = torch.tensor([1., 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    assert torch.equal(m.grids.detach(), eye.expand(3, 2, 4, 5, 12))
    t = torch.randn(3, 12, 2, 4, 5, generator=torch.Generator().manual_seed(2))
    back = BilateralGrids.from_channel_major(t)
    assert tuple(back.grids.shape) == (3, 2, 4, 5, 12)
    assert torch.equal(back.grids[1, 0, 2, 3].detach(), t[1, :, 0, 2, 3])
    assert torch.equal(back.to_channel_major(), t)

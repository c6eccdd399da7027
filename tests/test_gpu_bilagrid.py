"""GPU: the fused bilateral-grid slice (csrc/bilagrid.hip behind ``sgn_rast.appearance.slice_image``) per element against
the float64 definition (tests/bilagrid_fp64.py), forward and both gradients, on the smallest shapes at which each regime
of the backward's gather can go wrong; its exactness properties; and a fit through it.

TOLERANCE, for out, v_rgb and v_grid alike:  max|hip - f64| <= max(8 max|f32 - f64|, 4 * 2^-24 max|f64|), f32 being the
same written-out formulation evaluated in float32 on the same input.  The factor 8 is the project's precedent for a fused
kernel against the fp32 formulation's own error (tests/test_gpu_loss_per_pixel.py).  No pixel is left out: the inputs
are drawn away from the only discontinuity (``bilagrid_fp64.make_case``).  The measured ratios are in
profiles/bilagrid.md."""
import functools

import pytest
import torch

import bilagrid_fp64 as B

pytestmark = pytest.mark.gpu

# name -> (L, Hg, Wg, H, W)
SHAPES = {
    "a_fine_grid_partial_tiles": (8, 16, 16, 37, 53),       # grid finer than a wave's stride: supports of a few pixels
    "b_cells_larger_than_tiles": (4, 2, 3, 128, 160),       # supports of several bands, whole-image rows (Hg = 2), 4 levels
    "c_affine": (1, 1, 1, 37, 53),
    "d_single_level": (1, 5, 7, 37, 53),                    # L = 1 with Hg, Wg > 1
    "d_luma_only": (5, 1, 1, 37, 53),                       # Hg = Wg = 1 with L = 5
    "d_twelve_levels": (12, 2, 2, 37, 53),                  # more levels than one gather pass keeps: 8, then 4
    "e_production": (8, 16, 16, 1280, 1920),                # the production path: nine bands per cell, 8 levels in registers
}
EYE = torch.tensor([1., 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and both CPU evaluations of a shape, computed once and shared (never modified)."""
    L, Hg, Wg, H, W = SHAPES[name]
    grid, rgb, v_out = B.make_case(L, Hg, Wg, H, W, seed=11 + len(name))
    return grid, rgb, v_out, B.evaluate(grid, rgb, v_out), B.evaluate(grid, rgb, v_out, torch.float32)


def run_hip(grid, rgb, v_out, index=0, num=1):
    from sgn_rast import appearance
    grids = torch.zeros(num, *grid.shape)
    grids[index] = grid
    g = grids.cuda().requires_grad_(True)
    p = rgb.cuda().requires_grad_(True)
    out = appearance.slice_image(g, index, p)
    out.backward(v_out.cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), p.grad.cpu(), g.grad.cpu()


@pytest.mark.parametrize("name", list(SHAPES))
def test_per_element_against_fp64(name):
    grid, rgb, v_out, f64, f32 = case(name)
    out, v_rgb, v_grids = run_hip(grid, rgb, v_out)
    failures = []
    for what, hip, r64, r32 in zip(("out", "v_rgb", "v_grid"), (out, v_rgb, v_grids[0]), f64, f32):
        own = float((r32.double() - r64).abs().max())
        tol = max(8 * own, 4 * 2.0 ** -24 * float(r64.abs().max()))
        err = float((hip.double() - r64).abs().max())
        print(f"[bilagrid] {name} {what}: max|hip-f64| {err:.3e}  max|f32-f64| {own:.3e}  ratio {err / max(own, 1e-300):.2f}  "
              f"tol {tol:.3e}  max|f64| {float(r64.abs().max()):.3e}")
        if not err <= tol:
            failures.append((what, err, tol))
    assert not failures, failures


@pytest.mark.parametrize("name", ["a_fine_grid_partial_tiles", "e_production"])
def test_identity_grid_returns_rgb_bit_for_bit(name):
    from sgn_rast import appearance
    L, Hg, Wg, H, W = SHAPES[name]
    rgb = case(name)[1].cuda()
    m = appearance.BilateralGrids(2, (Wg, Hg, L)).cuda()
    with torch.no_grad():
        assert torch.equal(m(1, rgb), rgb)


def test_other_rows_are_never_read_and_get_exact_zeros():
    grid, rgb, v_out, f64, _ = case("b_cells_larger_than_tiles")
    from sgn_rast import appearance
    grids = torch.full((3, *grid.shape), float("nan"))
    grids[1] = grid
    g = grids.cuda().requires_grad_(True)
    p = rgb.cuda().requires_grad_(True)
    out = appearance.slice_image(g, 1, p)
    out.backward(v_out.cuda())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(p.grad).all()) and bool(torch.isfinite(g.grad).all())
    assert tuple(g.grad.shape) == tuple(grids.shape)
    assert float(g.grad[0].abs().max()) == 0.0 and float(g.grad[2].abs().max()) == 0.0
    assert float(g.grad[1].abs().max()) > 0.0
    ref = run_hip(grid, rgb, v_out)
    assert torch.equal(out.detach().cpu(), ref[0]) and torch.equal(p.grad.cpu(), ref[1])


@pytest.mark.parametrize("name", ["a_fine_grid_partial_tiles", "b_cells_larger_than_tiles"])
def test_forward_and_pixel_gradient_are_bit_identical_between_runs(name):
    grid, rgb, v_out = case(name)[:3]
    first, second = run_hip(grid, rgb, v_out), run_hip(grid, rgb, v_out)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])          # plain stores; v_grid's atomics carry no such promise


def test_no_incoming_gradient_launches_nothing():
    from sgn_rast import appearance

    class Untouched:                                 # any look at the saved tensors would raise AttributeError
        pass

    assert appearance._Slice.backward(Untouched(), None) == (None, None, None)
    grid, rgb, _ = case("c_affine")[:3]
    g = grid[None].cuda().requires_grad_(True)
    out = appearance.slice_image(g, 0, rgb.cuda())
    (out.sum() * 0.0 + g.sum()).backward()           # reaches the node with a materialised zero: finite, no NaN
    assert bool(torch.isfinite(g.grad).all())


def test_only_the_wanted_gradient_is_computed():
    grid, rgb, v_out, f64, f32 = case("b_cells_larger_than_tiles")
    from sgn_rast import appearance
    full = run_hip(grid, rgb, v_out)
    p = rgb.cuda().requires_grad_(True)                                  # pixels alone: the grid is a constant
    appearance.slice_image(grid[None].cuda(), 0, p).backward(v_out.cuda())
    assert torch.equal(p.grad.cpu(), full[1])
    g = grid[None].cuda().requires_grad_(True)                           # the grid alone
    appearance.slice_image(g, 0, rgb.cuda()).backward(v_out.cuda())
    tol = max(8 * float((f32[2].double() - f64[2]).abs().max()), 4 * 2.0 ** -24 * float(f64[2].abs().max()))
    assert float((g.grad[0].cpu().double() - f64[2]).abs().max()) <= tol


def test_non_contiguous_inputs_give_the_contiguous_result():
    grid, rgb, v_out, f64, f32 = case("a_fine_grid_partial_tiles")
    from sgn_rast import appearance
    ref = run_hip(grid, rgb, v_out)
    H, W, _ = rgb.shape
    wide = torch.zeros(H, W + 9, 3)
    wide[:, 4:4 + W] = rgb
    wide = wide.cuda().requires_grad_(True)
    view = wide[:, 4:4 + W]
    assert not view.is_contiguous()
    cm = grid.permute(3, 0, 1, 2).contiguous()[None].cuda().requires_grad_(True)       # channel-major storage
    g_view = cm.permute(0, 2, 3, 4, 1)
    assert not g_view.is_contiguous()
    out = appearance.slice_image(g_view, 0, view)
    out.backward(v_out.cuda())
    assert torch.equal(out.detach().cpu(), ref[0])
    assert torch.equal(wide.grad[:, 4:4 + W].cpu(), ref[1])
    assert float(wide.grad[:, :4].abs().max()) == 0.0 and float(wide.grad[:, 4 + W:].abs().max()) == 0.0
    tol = max(8 * float((f32[2].double() - f64[2]).abs().max()), 4 * 2.0 ** -24 * float(f64[2].abs().max()))
    got = cm.grad.permute(0, 2, 3, 4, 1)[0].cpu().double()
    assert float((got - f64[2]).abs().max()) <= tol


def test_cpu_tensors_fail_loudly():
    from sgn_rast import _lib, appearance
    grid, rgb, _ = case("c_affine")[:3]
    with pytest.raises(_lib.SgnRastError):
        appearance.slice_image(grid[None], 0, rgb)
    with pytest.raises(_lib.SgnRastError):
        appearance.slice_image(grid[None].cuda(), 0, rgb)


FIT_LR, FIT_STEPS = 0.05, 80      # chosen on the CPU: the fp64 loop ends at 1.3e-4 of its initial loss (float32: x 0.99998)


def _fit_problem():
    g = torch.Generator().manual_seed(0)
    img = torch.rand(48, 64, 3, generator=g)
    M = torch.tensor([[0.8, 0.15, -0.05], [0.1, 0.7, 0.1], [-0.1, 0.2, 1.1]])
    return img, img @ M.T + torch.tensor([0.05, -0.02, 0.1])


def test_fit_an_affine_through_the_kernels():
    """A 1 x 1 x 1 grid learns a fixed non-diagonal affine plus bias under Adam and MSE: the loop through the kernels ends
    where the float64 loop through the written-out definition ends, from the same start."""
    from sgn_rast import appearance
    img, tgt = _fit_problem()
    p64 = EYE.double().reshape(1, 1, 1, 12).clone().requires_grad_(True)
    opt = torch.optim.Adam([p64], lr=FIT_LR)
    mse64 = lambda: float(((B.slice_fwd(p64, img) - tgt.double()) ** 2).mean())
    first = mse64()
    for _ in range(FIT_STEPS):
        diff = B.slice_fwd(p64, img) - tgt.double()
        p64.grad = B.slice_bwd(p64, img, 2 * diff / diff.numel())[1]
        opt.step()
    last64 = mse64()
    assert last64 < 1e-2 * first, (first, last64)

    grids = appearance.BilateralGrids(1, (1, 1, 1)).cuda()
    opt = torch.optim.Adam(grids.parameters(), lr=FIT_LR)
    img_d, tgt_d = img.cuda(), tgt.cuda()
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        ((grids(0, img_d) - tgt_d) ** 2).mean().backward()
        opt.step()
    with torch.no_grad():
        last = float(((grids(0, img_d).double() - tgt_d.double()) ** 2).mean())
    print(f"[bilagrid fit] initial {first:.4e}  fp64 loop {last64:.4e}  kernels {last:.4e}  ratio {last / last64:.5f}")
    assert last <= 1.05 * last64, (last, last64)

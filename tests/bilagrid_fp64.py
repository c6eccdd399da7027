"""The bilateral-grid slice (include/sgn_rast.h "BILATERAL GRID") written out in torch ops: the forward and
both gradients by hand, with gathers and ``index_add_`` — not through autograd.  ``dtype=torch.float64`` is the
definition the kernels are held to; ``dtype=torch.float32`` is the same formulation at the kernels' precision, the
yardstick of the GPU tests' tolerance (what fp32 costs the formulation itself)."""
import torch

LUMA = (0.299, 0.587, 0.114)


def _axis(g, n):
    """x0, x1, f of a grid coordinate in [0, n - 1]."""
    i0 = torch.floor(g).long().clamp(0, n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, g - i0.to(g.dtype)


def _site(grid, rgb):
    """Per pixel (flattened): the eight cells' flat indices [8,P] (index = zbit + 2 xbit + 4 ybit), the axis weights and
    the unclamped luminance."""
    L, Hg, Wg, _ = grid.shape
    H, W, _ = rgb.shape
    dt = rgb.dtype
    jj = (torch.arange(W, dtype=dt) + 0.5) / W * (Wg - 1)
    ii = (torch.arange(H, dtype=dt) + 0.5) / H * (Hg - 1)
    gx = jj[None, :].expand(H, W).reshape(-1)
    gy = ii[:, None].expand(H, W).reshape(-1)
    p = rgb.reshape(-1, 3)
    luma = LUMA[0] * p[:, 0] + LUMA[1] * p[:, 1] + LUMA[2] * p[:, 2]
    gz = luma.clamp(0, 1) * (L - 1)
    x0, x1, fx = _axis(gx, Wg)
    y0, y1, fy = _axis(gy, Hg)
    z0, z1, fz = _axis(gz, L)
    cells = []
    for k in range(8):
        zz, xx, yy = (z1 if k & 1 else z0), (x1 if k & 2 else x0), (y1 if k & 4 else y0)
        cells.append((zz * Hg + yy) * Wg + xx)
    return torch.stack(cells), (fz, fx, fy), luma


def _mix(c, fz, fx, fy):
    """Nested lerps a + f * (b - a) of eight [P,12] cell tables: z innermost, then x, then y.  Returns (A, dA)."""
    fz, fx, fy = fz[:, None], fx[:, None], fy[:, None]
    d = [c[2 * m + 1] - c[2 * m] for m in range(4)]              # (x0,y0), (x1,y0), (x0,y1), (x1,y1)
    a = [c[2 * m] + fz * d[m] for m in range(4)]
    lerp2 = lambda v: (v[0] + fx * (v[1] - v[0])) + fy * ((v[2] + fx * (v[3] - v[2])) - (v[0] + fx * (v[1] - v[0])))
    return lerp2(a), lerp2(d)


def evaluate(grid, rgb, v_out=None, dtype=torch.float64):
    """(out, v_rgb, v_grid) of grid [L,Hg,Wg,12] on rgb [H,W,3] for the incoming v_out [H,W,3], evaluated in ``dtype`` on
    the CPU by the written-out formulas; the two gradients are None without a v_out."""
    grid, rgb = grid.detach().cpu().to(dtype), rgb.detach().cpu().to(dtype)
    L = grid.shape[0]
    cells, (fz, fx, fy), luma = _site(grid, rgb)
    flat = grid.reshape(-1, 12)
    A, dA = _mix([flat[cells[k]] for k in range(8)], fz, fx, fy)
    A, dA = A.reshape(-1, 3, 4), dA.reshape(-1, 3, 4)
    p = rgb.reshape(-1, 3)
    out = (A[:, :, 0] * p[:, 0:1] + A[:, :, 1] * p[:, 1:2] + A[:, :, 2] * p[:, 2:3] + A[:, :, 3]).reshape(rgb.shape)
    if v_out is None:
        return out, None, None
    v = v_out.detach().cpu().to(dtype).reshape(-1, 3)
    # v_p_k = sum_r v_r A[r,k] + lw_k (L - 1) [0 < luma < 1] sum_r v_r (dA[r,:] . (R,G,B,1))
    dot = dA[:, :, 0] * p[:, 0:1] + dA[:, :, 1] * p[:, 1:2] + dA[:, :, 2] * p[:, 2:3] + dA[:, :, 3]        # [P,3]
    guide = (v * dot).sum(1) * (L - 1) * ((luma > 0) & (luma < 1)).to(dtype)
    v_rgb = (v[:, :, None] * A[:, :, :3]).sum(1) + guide[:, None] * torch.tensor(LUMA, dtype=dtype)[None, :]
    # v_g[cell] += w_cell v_r (R,G,B,1)
    p4 = torch.cat([p, torch.ones_like(p[:, :1])], 1)
    outer = (v[:, :, None] * p4[:, None, :]).reshape(-1, 12)
    v_flat = torch.zeros_like(flat)
    for k in range(8):
        w = (fz if k & 1 else 1 - fz) * (fx if k & 2 else 1 - fx) * (fy if k & 4 else 1 - fy)
        v_flat.index_add_(0, cells[k], w[:, None] * outer)
    return out, v_rgb.reshape(rgb.shape), v_flat.reshape(grid.shape)


def slice_fwd(grid, rgb, dtype=torch.float64):
    """out [H,W,3] alone."""
    return evaluate(grid, rgb, None, dtype)[0]


def slice_bwd(grid, rgb, v_out, dtype=torch.float64):
    """(v_rgb [H,W,3], v_grid [L,Hg,Wg,12]) alone."""
    return evaluate(grid, rgb, v_out, dtype)[1:]


def total_variation(grids):
    """The prior by hand, in float64: sum over the axes of size > 1 of the mean squared forward difference, over num."""
    g = grids.detach().cpu().double()
    tv = 0.0
    for axis in (1, 2, 3):
        n = g.shape[axis]
        if n > 1:
            a, b = g.narrow(axis, 0, n - 1), g.narrow(axis, 1, n - 1)
            tv += float(((b - a) ** 2).sum()) / a.numel()
    return tv / g.shape[0]


def make_case(L, Hg, Wg, H, W, seed):
    """The GPU tests' inputs: grid = identity + N(0, 0.3); rgb uniform in [0, 1.5] with 5 % exact zeros (both clamps of
    the luminance are hit); v_out N(0, 1).  Pixels whose luma * (L - 1) lies within 1e-3 of an integer (float64) are
    redrawn — the guidance derivative is discontinuous only there — so no pixel is left out of any comparison."""
    g = torch.Generator().manual_seed(seed)
    eye = torch.tensor([1., 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    grid = eye.expand(L, Hg, Wg, 12) + 0.3 * torch.randn(L, Hg, Wg, 12, generator=g)
    rgb = 1.5 * torch.rand(H, W, 3, generator=g)
    zero = torch.rand(H, W, generator=g) < 0.05
    lw = torch.tensor(LUMA, dtype=torch.float64)

    def near_kink(t):
        gz = (t.double() * lw).sum(-1) * (L - 1)
        return ((gz - gz.round()).abs() < 1e-3) & ~zero

    for _ in range(64):
        bad = near_kink(rgb) if L > 1 else torch.zeros(H, W, dtype=torch.bool)
        if not bool(bad.any()):
            break
        rgb[bad] = 1.5 * torch.rand(int(bad.sum()), 3, generator=g)
    else:
        raise AssertionError("could not draw an input away from the luminance kinks")
    rgb[zero] = 0.0
    v_out = torch.randn(H, W, 3, generator=g)
    return grid.contiguous(), rgb.contiguous(), v_out

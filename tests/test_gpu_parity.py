"""GPU (-m gpu): every HIP kernel, called through the C ABI, against the CPU oracle on the same
seeded inputs.  Integer / index / key outputs must be bit-exact; floating point within the
tolerance written next to each assert."""
import pytest
import torch

from adversarial_scenes import sigma_kernel_order
from helpers import activated, rel_l2, small_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from sgn_rast import _lib, ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()  # raises if libsgnrast.so is missing: no fallback
    return ops


@pytest.fixture(autouse=True, params=[(0, 0), (1, 0), (0, 1), (1, 1)],
                ids=["scalar-chase", "ldsbatch", "scalar-chase-split", "ldsbatch-split"])
def raster_record_mode(request):
    """Every test in this module runs with each code path of the raster kernels (round 6: the surviving ones — the
    "stream" mode and the forced one- / four-wave shapes are gone): the scalar row chase or the LDS-batched long-list path
    (forced on / forbidden through the thresholds), and launch-order thresholds small enough that these small scenes have
    tiles on BOTH sides of them (four-wave forward tiles; the backward's long-walk kernel) or on one side only."""
    from sgn_rast import _lib as L
    batch, split = request.param
    thr = (24, 24) if batch else (1 << 30, 1 << 30)                  # force / forbid the LDS path
    kw = dict(batch_fwd=thr[0], batch_bwd=thr[1])
    if split:
        kw.update(adapt_fwd=96, adapt_bwd=48)                        # small scenes: make some tiles split, others not
    L.load()
    with L.options(**kw):
        yield request.param


def _project_args(cam, P, block=16, dev="cpu"):
    scales, quats, _, _ = activated(P)
    return (P["means"].to(dev), scales.to(dev), 1.0, quats.to(dev), cam.viewmat[:3, :].to(dev), cam.fx, cam.fy,
            cam.cx, cam.cy, cam.height, cam.width, block)


# --------------------------------------------------------------- projection
@pytest.mark.parametrize("block", [16, 8, 5])
@pytest.mark.parametrize("size", [(128, 128), (130, 70)])
def test_project_forward_bit_exact(hip, c_oracle, block, size):
    cam, P = small_scene(n=20000, w=size[0], h=size[1])
    P["means"][:50, 2] = 0.005   # near-plane culls
    P["means"][50:100, 0] = 1e4  # off-screen culls
    exp = c_oracle.project_fwd(*_project_args(cam, P, block))
    got = hip.project_gaussians(*_project_args(cam, P, block, DEV))
    for name, a, b in zip(["xys", "depths", "radii", "conics", "compensation", "num_tiles_hit", "cov3d"], got, exp):
        assert torch.equal(a.cpu(), b), f"{name} differs: {(a.cpu().float() - b.float()).abs().max()}"


def test_project_backward(hip, c_oracle):
    cam, P = small_scene(n=20000)
    args = _project_args(cam, P)
    xys, depths, radii, conics, comp, nth, cov3d = c_oracle.project_fwd(*args)
    g = torch.Generator().manual_seed(1)
    n = radii.numel()
    v_xy, v_d, v_con, v_comp = (torch.randn(n, 2, generator=g), torch.randn(n, generator=g),
                                torch.randn(n, 3, generator=g), torch.randn(n, generator=g))
    exp = c_oracle.project_bwd(args[0], args[1], 1.0, args[3], args[4], cam.fx, cam.fy, cov3d, radii, conics, comp,
                               v_xy, v_d, v_con, v_comp)
    dargs = list(_project_args(cam, P, 16, DEV))
    leaves = [dargs[0].requires_grad_(True), dargs[1].requires_grad_(True), dargs[3].requires_grad_(True)]
    out = hip.project_gaussians(*dargs)
    torch.autograd.backward([out[0], out[1], out[3], out[4]],
                            [v_xy.to(DEV), v_d.to(DEV), v_con.to(DEV), v_comp.to(DEV)])
    for name, leaf, e in zip(["v_mean", "v_scale", "v_quat"], leaves, exp[:3]):
        got = leaf.grad.cpu()
        assert rel_l2(got, e) < 1e-5, name                      # same formulas, fp32 both sides
        assert (got[radii == 0] == 0).all(), name               # culled rows get exact zeros
    # without a compensation gradient (the reference's case: output discarded)
    for l in leaves:
        l.grad = None
    out = hip.project_gaussians(*dargs)
    torch.autograd.backward([out[0], out[1], out[3]], [v_xy.to(DEV), v_d.to(DEV), v_con.to(DEV)])
    exp0 = c_oracle.project_bwd(args[0], args[1], 1.0, args[3], args[4], cam.fx, cam.fy, cov3d, radii, conics, comp,
                                v_xy, v_d, v_con, torch.zeros(n))
    for leaf, e in zip(leaves, exp0[:3]):
        assert rel_l2(leaf.grad.cpu(), e) < 1e-5


@pytest.mark.parametrize("parts", [(1, 1, 0), (0, 0, 1), (1, 1, 1)], ids=["xys+depths", "conics", "all"])
def test_viewmat_gradient_matches_autograd_through_the_torch_oracle(hip, torch_oracle, parts):
    """Upstream returns a viewmat gradient when `viewmat.requires_grad` (the reference never asks: its camera optimiser is
    off, sgn_config.py:44).  Assembled on the host from the backward kernel's per-Gaussian outputs; checked against
    fp64 autograd through the pure-PyTorch oracle (centres within 1.3x the frustum, where the forward's clamp is
    inactive), for a [3,4] and a [4,4] view matrix with a rolled camera; the other gradients stay what they were."""
    import math
    cam, P = small_scene(n=8000)
    args = _project_args(cam, P)
    g = torch.Generator().manual_seed(4)
    n = args[0].shape[0]
    w_xy, w_d, w_c = torch.randn(n, 2, generator=g), torch.randn(n, generator=g), torch.randn(n, 3, generator=g)
    c, s_ = math.cos(0.07), math.sin(0.07)
    roll = torch.tensor([[c, -s_, 0, 0], [s_, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]], dtype=torch.float64)
    V0 = torch.eye(4, dtype=torch.float64)
    V0[:3, :] = args[4].double()
    V0 = roll @ V0

    def run(fn, dev, dtype, full):
        a = [t.to(dev, dtype) if torch.is_tensor(t) and t.is_floating_point() else t for t in args]
        vm = (V0 if full else V0[:3, :]).detach().clone().to(dev, dtype).contiguous().requires_grad_(True)
        leaves = [a[0].clone().requires_grad_(True), a[1].clone().requires_grad_(True), a[3].clone().requires_grad_(True)]
        out = fn(leaves[0], leaves[1], 1.0, leaves[2], vm, *a[5:])
        live = out[2] > 0
        loss = (parts[0] * (out[0] * w_xy.to(dev, dtype))[live].sum() + parts[1] * (out[1] * w_d.to(dev, dtype))[live].sum()
                + parts[2] * (out[3] * w_c.to(dev, dtype))[live].sum())
        loss.backward()
        return vm.grad.detach().cpu().double(), [l.grad.detach().cpu().double() for l in leaves]
    for full in (False, True):
        exp_v, exp_l = run(torch_oracle.project_gaussians, "cpu", torch.float64, full)
        got_v, got_l = run(hip.project_gaussians, DEV, torch.float32, full)
        assert got_v.shape == exp_v.shape == ((4, 4) if full else (3, 4))
        assert rel_l2(got_v[:3], exp_v[:3]) < 1e-4, (full, got_v, exp_v)
        assert float(got_v[3:].abs().sum()) == 0.0
        for a_, b_ in zip(got_l, exp_l):
            assert rel_l2(a_, b_) < 1e-4


def test_without_a_viewmat_gradient_the_projection_node_returns_none_for_it(hip):
    cam, P = small_scene(n=2000)
    dargs = list(_project_args(cam, P, 16, DEV))
    dargs[0].requires_grad_(True)
    out = hip.project_gaussians(*dargs)
    out[0].sum().backward()
    assert dargs[4].grad is None and dargs[0].grad is not None


# ----------------------------------------------------------------------- SH
@pytest.mark.parametrize("k,deg", [(1, 0), (4, 1), (9, 2), (16, 3), (16, 0), (16, 2), (25, 4), (25, 3)])
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 4097])
def test_sh_forward_backward(hip, c_oracle, k, deg, n):
    g = torch.Generator().manual_seed(n * 31 + k)
    dirs = torch.randn(n, 3, generator=g) * 2
    coeffs = torch.randn(n, k, 3, generator=g)
    v_col = torch.randn(n, 3, generator=g)
    exp = c_oracle.sh_fwd(deg, dirs, coeffs)
    cd = coeffs.to(DEV).requires_grad_(True)
    got = hip.spherical_harmonics(deg, dirs.to(DEV), cd)
    assert (got.cpu() - exp).abs().max() < 2e-5                 # fp32 sum of <=25 products, |terms| ~ 1
    got.backward(v_col.to(DEV))
    expb = c_oracle.sh_bwd(deg, k, dirs, v_col)
    assert (cd.grad.cpu() - expb).abs().max() < 2e-6
    assert (cd.grad[:, (deg + 1) ** 2:, :] == 0).all()          # inactive bands: exact zeros


@pytest.mark.parametrize("k,deg,n", [(16, 3, 193), (1, 0, 193), (1, 0, 130)])
def test_sh_forward_of_coefficients_at_an_odd_storage_offset_equals_the_aligned_call(hip, k, deg, n):
    """A contiguous view 4 bytes into its storage takes the dword stage-in instead of the float4 one: same bits.
    193 rows: three full spans and a one-row span (k = 1: three floats, all tail, no float4); 130 rows, k = 1: a two-row
    last span, one float4 and a two-float tail in the aligned call."""
    g = torch.Generator().manual_seed(n * 31 + k)
    dirs = (torch.randn(n, 3, generator=g) * 2).to(DEV)
    store = torch.randn(n * k * 3 + 1, generator=g).to(DEV)
    odd = store[1:].reshape(n, k, 3)
    aligned = odd.clone()
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    assert torch.equal(hip.spherical_harmonics(deg, dirs, odd), hip.spherical_harmonics(deg, dirs, aligned))


# ------------------------------------------------------------------ binning
@pytest.mark.parametrize("n", [1, 5, 2047, 2048, 2049, 100_000, 1_000_003])
def test_scan_bit_exact(hip, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 40, (n,), generator=g, dtype=torch.int32)
    total, cum = hip.compute_cumulative_intersects(x.to(DEV))
    ref = torch.cumsum(x, 0, dtype=torch.int32)
    assert torch.equal(cum.cpu(), ref) and total == int(ref[-1])


def test_map_intersects_bit_exact_including_big_splats(hip, c_oracle):
    cam, P = small_scene(n=6000, w=320, h=200)
    P["log_scales"][:40] += 3.0       # a few huge splats: > 32 tiles -> wave-cooperative emission path
    xys, depths, radii, conics, comp, nth, cov3d = c_oracle.project_fwd(*_project_args(cam, P))
    assert int(nth.max()) > 64
    cum = c_oracle.scan_i32(nth)
    tx, ty = (cam.width + 15) // 16, (cam.height + 15) // 16
    ek, ev = c_oracle.map_isect(xys, depths, radii, cum, tx, ty, 16)
    gk, gv = hip.map_gaussian_to_intersects(xys.shape[0], int(cum[-1]), xys.to(DEV), depths.to(DEV),
                                            radii.to(DEV), cum.to(DEV), (tx, ty, 1), 16)
    assert torch.equal(gk.cpu(), ek) and torch.equal(gv.cpu(), ev)


@pytest.mark.parametrize("n", [1, 2, 100, 4095, 4096, 4097, 12289, 300_000])
def test_sort_bit_exact_and_stable(hip, n):
    from sgn_rast import ops
    g = torch.Generator().manual_seed(n)
    n_tiles = 9600
    tile = torch.randint(0, n_tiles, (n,), generator=g, dtype=torch.int64)
    # few distinct depths -> many (tile, depth) ties: stability decides the payload order
    depth = torch.randint(0, 50, (n,), generator=g, dtype=torch.int64) * 1_000_003 + 0x3F000000
    keys = (tile << 32) | depth
    vals = torch.arange(n, dtype=torch.int32)
    ks, vs = ops.sort_intersects(keys.to(DEV), vals.to(DEV), n_tiles)
    rk, order = torch.sort(keys, stable=True)
    assert torch.equal(ks.cpu(), rk)
    assert torch.equal(vs.cpu(), vals[order])


def test_sort_full_key_range_bits(hip):
    """sgn_sort_pairs over an explicit bit range equals a full sort when the other bits are equal."""
    from sgn_rast import _lib as L
    n = 50_000
    g = torch.Generator().manual_seed(9)
    keys = torch.randint(0, 2 ** 40, (n,), generator=g, dtype=torch.int64)
    vals = torch.arange(n, dtype=torch.int32)
    kd, vd = keys.to(DEV), vals.to(DEV)
    ko, vo = torch.empty_like(kd), torch.empty_like(vd)
    lib = L.load()
    ws = L.workspace(lib.sgn_sort_workspace_bytes(n), kd.device)
    for end_bit in (40, 41, 47, 64):      # 5, 6, 6, 8 passes: both ping-pong parities
        L.check(lib.sgn_sort_pairs(n, 0, end_bit, L.ptr(kd), L.ptr(vd), L.ptr(ko), L.ptr(vo), L.ptr(ws),
                                   ws.numel(), L.sort_rank_mode(), L.stream_ptr()), "sort")
        rk, order = torch.sort(keys, stable=True)
        assert torch.equal(ko.cpu(), rk) and torch.equal(vo.cpu(), vals[order]), end_bit


def test_bin_and_sort_pipeline_bit_exact(hip, c_oracle):
    cam, P = small_scene(n=30000, w=640, h=360, focal=500.0)
    xys, depths, radii, conics, comp, nth, cov3d = c_oracle.project_fwd(*_project_args(cam, P))
    cum, keys, vals, ks, vs, bins = c_oracle.bin_and_sort(xys, depths, radii, nth, cam.height, cam.width, 16)
    tb = ((cam.width + 15) // 16, (cam.height + 15) // 16, 1)
    I, cum_d = hip.compute_cumulative_intersects(nth.to(DEV))
    assert I == keys.numel() and torch.equal(cum_d.cpu(), cum)
    gk, gv, gks, gvs, gbins = hip.bin_and_sort_gaussians(
        xys.shape[0], I, xys.to(DEV), depths.to(DEV), radii.to(DEV), cum_d, tb, 16)
    assert torch.equal(gk.cpu(), keys) and torch.equal(gv.cpu(), vals)
    assert torch.equal(gks.cpu(), ks), "sorted (tile|depth) keys must be bit-exact"
    assert torch.equal(gvs.cpu(), vs), "gaussian_ids_sorted must be bit-exact (stable ties)"
    assert torch.equal(gbins.cpu(), bins)


@pytest.mark.parametrize("n,size,focal", [(30000, (640, 360), 500.0), (5000, (130, 70), 100.0), (1, (64, 64), 64.0),
                                          (20000, (4208, 4208), 3000.0)])   # 263 x 263 tiles > 65536: 32-bit tile keys
def test_fused_rank_binning_equals_upstream_shaped_path(hip, c_oracle, n, size, focal):
    """The rank-order emission + tile-only stable sort that rasterize_gaussians runs must give
    the same gaussian_ids_sorted / tile_bins, bit for bit, as the upstream-shaped 64-bit pair sort
    (and as the oracle) — including depth ties, which fall back to Gaussian-id order in both."""
    from sgn_rast import ops
    cam, P = small_scene(n=n, w=size[0], h=size[1], focal=focal)
    if n > 100:
        P["means"][100:140] = P["means"][60:100]      # exact depth ties between different Gaussians
        P["log_scales"][:20] += 3.0                   # huge splats (wave-cooperative emission)
    xys, depths, radii, conics, comp, nth, cov3d = c_oracle.project_fwd(*_project_args(cam, P))
    cum, keys, vals, ks, vs, bins = c_oracle.bin_and_sort(xys, depths, radii, nth, cam.height, cam.width, 16)
    tb = ((cam.width + 15) // 16, (cam.height + 15) // 16, 1)
    I, ids, tbins = ops.bin_gaussians_fused(xys.shape[0], xys.to(DEV), depths.to(DEV), radii.to(DEV), nth.to(DEV),
                                            tb, 16)
    assert I == keys.numel()
    assert torch.equal(ids.cpu(), vs), "gaussian_ids_sorted must be bit-exact"
    assert torch.equal(tbins.cpu(), bins)
    # exact tile culling: the kept list is a sub-sequence of upstream's, tile by tile, and every dropped
    # (tile, Gaussian) pair has no pixel centre with alpha >= 1/255 (checked against the definition)
    opac = torch.sigmoid(P["opacity_logits"]).reshape(-1)
    Ic, idc, binc = ops.bin_gaussians_fused(xys.shape[0], xys.to(DEV), depths.to(DEV), radii.to(DEV), nth.to(DEV), tb,
                                            16, conics=conics.to(DEV), opacity=opac.to(DEV), cull=True)
    idc, binc = idc.cpu(), binc.cpu()
    assert Ic <= I and (n < 100 or Ic < 0.9 * I)
    rng = torch.Generator().manual_seed(0)
    for t in torch.randperm(tb[0] * tb[1], generator=rng)[:40].tolist():
        full = vs[int(bins[t, 0]):int(bins[t, 1])].tolist()
        kept = idc[int(binc[t, 0]):int(binc[t, 1])].tolist()
        it = iter(full)
        assert all(g in it for g in kept), "culled list must be a sub-sequence of the upstream list"
        dropped = sorted(set(full) - set(kept))
        if dropped:
            g = torch.tensor(dropped)
            px = (t % tb[0]) * 16 + torch.arange(16) + 0.5
            py = (t // tb[0]) * 16 + torch.arange(16) + 0.5
            dx = xys[g, 0][:, None, None] - px[None, None, :]
            dy = xys[g, 1][:, None, None] - py[None, :, None]
            # the kernels' own evaluation (fp32, their operation order, single-rounding fmas): near the margin a
            # differently ordered sum can pass or fail for the wrong reason
            sig = sigma_kernel_order(conics[g, 0][:, None, None], conics[g, 1][:, None, None],
                                     conics[g, 2][:, None, None], dx, dy)
            alpha = torch.clamp(opac[g][:, None, None] * torch.exp(-sig), max=0.999)
            assert not bool(((sig >= 0) & (alpha >= 1.0 / 255.0)).any()), "a dropped pair had a valid pixel"


# ---------------------------------------------------------------- rasterize
def _raster_inputs(c_oracle, cam, P, block=16, seed=2):
    scales, quats, opac, coeffs = activated(P)
    xys, depths, radii, conics, comp, nth, cov3d = c_oracle.project_fwd(*_project_args(cam, P, block))
    _, _, _, _, vs, bins = c_oracle.bin_and_sort(xys, depths, radii, nth, cam.height, cam.width, block)
    rgb = torch.clamp(c_oracle.sh_fwd(3, P["means"], coeffs) + 0.5, min=0)
    g = torch.Generator().manual_seed(seed)
    v_img = torch.randn(cam.height, cam.width, 3, generator=g)
    v_alpha = torch.randn(cam.height, cam.width, generator=g)
    return dict(xys=xys, depths=depths, radii=radii, conics=conics, nth=nth, rgb=rgb, opac=opac, ids=vs,
                bins=bins, v_img=v_img, v_alpha=v_alpha)


def _hip_raster(hip, cam, R, block, bg, need_grad=True):
    d = {k: v.to(DEV) for k, v in R.items()}
    leaves = dict(xys=d["xys"].clone().requires_grad_(need_grad), conics=d["conics"].clone().requires_grad_(need_grad),
                  rgb=d["rgb"].clone().requires_grad_(need_grad), opac=d["opac"].clone().requires_grad_(need_grad))
    img, alpha = hip.rasterize_gaussians(leaves["xys"], d["depths"], d["radii"], leaves["conics"], d["nth"],
                                         leaves["rgb"], leaves["opac"], cam.height, cam.width, block,
                                         background=bg.to(DEV), return_alpha=True)
    return img, alpha, leaves, d


@pytest.mark.parametrize("block,size", [(16, (128, 128)), (16, (130, 70)), (8, (100, 60)), (5, (64, 37)), (2, (20, 12)),
                                        (2, (600, 500))])                   # 300 x 250 tiles > 65536: 32-bit tile keys
def test_rasterize_forward_fast_exp(hip, c_oracle, block, size):
    cam, P = small_scene(n=3000, w=size[0], h=size[1], focal=float(size[0]))
    R = _raster_inputs(c_oracle, cam, P, block)
    bg = torch.tensor([0.1, 0.2, 0.3])
    exp_img, exp_T, exp_idx = c_oracle.raster_fwd(cam.height, cam.width, block, R["ids"], R["bins"], R["xys"],
                                                  R["conics"], R["rgb"], R["opac"], bg)
    img, alpha, _, _ = _hip_raster(hip, cam, R, block, bg, need_grad=False)
    err = (img.cpu() - exp_img).abs()
    # hardware v_exp_f32 vs libm expf differ by ~1 ulp: ordinary pixels agree to 1e-5; a pixel whose
    # alpha >= 1/255 or T <= 1e-4 test sits on the threshold may flip one Gaussian (<= 1/255 * colour)
    assert float(err.mean()) < 1e-6
    assert float((err > 1e-5).float().mean()) < 2e-3
    assert float(err.max()) < 2e-2
    assert float((alpha.cpu() - (1 - exp_T)).abs().max()) < 2e-2
    assert float(((alpha.cpu() - (1 - exp_T)).abs() > 1e-5).float().mean()) < 2e-3


@pytest.mark.parametrize("block,size", [(16, (128, 128)), (16, (130, 70)), (7, (64, 37))])
def test_rasterize_forward_exact_exp_mode_is_bit_exact(hip, c_oracle, block, size):
    """With both sides on the portable polynomial exp, the whole forward (image, final T, index of
    the last contributing Gaussian) must agree bit for bit: same op order, same decisions."""
    from sgn_rast import _lib as L
    cam, P = small_scene(n=3000, w=size[0], h=size[1], focal=float(size[0]))
    R = _raster_inputs(c_oracle, cam, P, block)
    bg = torch.tensor([0.1, 0.2, 0.3])
    c_oracle.set_exp_mode(1)
    L.set_options(exact_exp=1)
    try:
        exp_img, exp_T, exp_idx = c_oracle.raster_fwd(cam.height, cam.width, block, R["ids"], R["bins"], R["xys"],
                                                      R["conics"], R["rgb"], R["opac"], bg)
        d = {k: v.to(DEV) for k, v in R.items()}
        from sgn_rast import ops
        tb = ((cam.width + block - 1) // block, (cam.height + block - 1) // block, 1)
        lib = L.load()
        I = R["ids"].numel()
        out_img = torch.empty(cam.height, cam.width, 3, device=DEV)
        fT = torch.empty(cam.height, cam.width, device=DEV)
        fi = torch.empty(cam.height, cam.width, dtype=torch.int32, device=DEV)
        n = R["xys"].shape[0]
        recs = L.workspace(lib.sgn_raster_workspace_bytes(n, I, L.opts_ptr()), out_img.device)
        L.check(lib.sgn_raster_fwd(cam.height, cam.width, block, n, I, L.ptr(d["ids"]), L.ptr(d["bins"]),
                                   L.ptr(d["xys"]), L.ptr(d["conics"]), L.ptr(d["rgb"]),
                                   L.ptr(d["opac"].reshape(-1).contiguous()), 0, 0, n, 0, L.ptr(bg.to(DEV)),
                                   L.ptr(out_img), L.ptr(fT), L.ptr(fi), L.ptr(recs), recs.numel(), 0, None, None,
                                   None, None, None, L.opts_ptr(), L.stream_ptr()), "raster_fwd")
        assert torch.equal(fi.cpu(), exp_idx)
        assert torch.equal(fT.cpu(), exp_T)
        assert torch.equal(out_img.cpu(), exp_img)
    finally:
        c_oracle.set_exp_mode(0)
        L.set_options(exact_exp=0)


@pytest.mark.parametrize("block,size", [(16, (128, 128)), (16, (130, 70)), (8, (100, 60))])
@pytest.mark.parametrize("clamp", [0.99, 0.999])
@pytest.mark.parametrize("reduce_mode", [0, 1])
def test_rasterize_backward(hip, c_oracle, block, size, clamp, reduce_mode):
    from sgn_rast import _lib as L, ops
    L.set_options(reduce_mode=reduce_mode)   # 0: butterfly shuffles, 1: transposed permlane-swap reduction
    cam, P = small_scene(n=3000, w=size[0], h=size[1], focal=float(size[0]))
    P["opacity_logits"][:200] = 9.0   # opacity ~0.9999: exercises the 0.999 (fwd) / 0.99 (bwd) clamps
    R = _raster_inputs(c_oracle, cam, P, block)
    bg = torch.tensor([0.1, 0.2, 0.3])
    ops.set_alpha_clamp_bwd(clamp)
    try:
        img, alpha, leaves, d = _hip_raster(hip, cam, R, block, bg)
        torch.autograd.backward([img, alpha], [d["v_img"], d["v_alpha"]])
    finally:
        ops.set_alpha_clamp_bwd(ops.UPSTREAM_ALPHA_CLAMP_BWD)
        L.set_options(reduce_mode=1)
    # oracle backward from the oracle's own forward state
    exp_img, exp_T, exp_idx = c_oracle.raster_fwd(cam.height, cam.width, block, R["ids"], R["bins"], R["xys"],
                                                  R["conics"], R["rgb"], R["opac"], bg)
    e_xy, e_con, e_col, e_op = c_oracle.raster_bwd(
        cam.height, cam.width, block, R["ids"], R["bins"], R["xys"], R["conics"], R["rgb"], R["opac"], bg,
        exp_T, exp_idx, R["v_img"], R["v_alpha"], clamp)
    # fp32 atomics in arbitrary order + 1-ulp exp vs a double-accumulating oracle: rel-L2 <= 1e-4
    # (SURVEY.md §8c); threshold flips of single pixels stay far below that in the norm
    assert rel_l2(leaves["xys"].grad.cpu(), e_xy) < 1e-4
    assert rel_l2(leaves["conics"].grad.cpu(), e_con) < 1e-4
    assert rel_l2(leaves["rgb"].grad.cpu(), e_col) < 1e-4
    assert rel_l2(leaves["opac"].grad.cpu(), e_op) < 1e-4
    assert leaves["opac"].grad.shape == R["opac"].shape   # [N,1] like the input


def test_rasterize_v_conic_is_the_true_derivative(hip, c_oracle, torch_oracle):
    """the rasterizer's public `v_conics` output, on its own, against the only externally
    checkable definition — fp64 autograd through the torch restatement of `_torch_impl.rasterize_forward` — column
    by column (so a factor on the off-diagonal entry cannot hide in the norm).  Opacities stay <= 0.98 so the
    0.999 / 0.99 clamp quirk is inactive (self-consistent clamp)."""
    from sgn_rast import ops
    cam, P = small_scene(n=2000, w=96, h=64, focal=96.0)
    R = _raster_inputs(c_oracle, cam, P, 16)
    bg = torch.tensor([0.1, 0.2, 0.3])
    ops.set_alpha_clamp_bwd(0.999)
    try:
        img, alpha, leaves, d = _hip_raster(hip, cam, R, 16, bg)
        torch.autograd.backward([img, alpha], [d["v_img"], d["v_alpha"]])
    finally:
        ops.set_alpha_clamp_bwd(ops.UPSTREAM_ALPHA_CLAMP_BWD)
    D = torch.float64
    t = {k: R[k].to(D).requires_grad_(True) for k in ("xys", "conics", "rgb", "opac")}
    img64, alpha64 = torch_oracle.rasterize_gaussians(t["xys"], R["depths"].to(D), R["radii"], t["conics"], R["nth"],
                                                      t["rgb"], t["opac"], cam.height, cam.width, 16, bg.to(D), True)
    torch.autograd.backward([img64, alpha64], [R["v_img"].to(D), R["v_alpha"].to(D)])
    got, exp = leaves["conics"].grad.cpu().double(), t["conics"].grad
    for col in range(3):
        assert rel_l2(got[:, col], exp[:, col]) < 1e-4, (col, rel_l2(got[:, col], exp[:, col]))
    assert rel_l2(leaves["xys"].grad.cpu().double(), t["xys"].grad) < 1e-4


def test_rasterize_no_intersections(hip):
    n = 16
    bg = torch.tensor([0.3, 0.6, 0.9], device=DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    col = torch.rand(n, 3, device=DEV, requires_grad=True)
    img, alpha = hip.rasterize_gaussians(z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32), col,
                                         torch.rand(n, 1, device=DEV), 40, 50, 16, background=bg, return_alpha=True)
    assert torch.equal(img, bg.expand(40, 50, 3)) and float(alpha.abs().max()) == 0.0
    img.sum().backward()
    assert float(col.grad.abs().max()) == 0.0
    img1 = hip.rasterize_gaussians(z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32), col.detach(),
                                   torch.rand(n, 1, device=DEV), 40, 50, 16)     # default background = ones
    assert torch.equal(img1, torch.ones(40, 50, 3, device=DEV))


def test_uint8_colors_and_single_output(hip, c_oracle):
    cam, P = small_scene(n=1500)
    R = _raster_inputs(c_oracle, cam, P)
    col8 = (R["rgb"].clamp(0, 1) * 255).to(torch.uint8)
    bg = torch.zeros(3)
    exp_img, _, _ = c_oracle.raster_fwd(cam.height, cam.width, 16, R["ids"], R["bins"], R["xys"], R["conics"],
                                        col8.float() / 255, R["opac"], bg)
    d = {k: v.to(DEV) for k, v in R.items()}
    img = hip.rasterize_gaussians(d["xys"], d["depths"], d["radii"], d["conics"], d["nth"], col8.to(DEV), d["opac"],
                                  cam.height, cam.width, 16, bg.to(DEV))
    assert isinstance(img, torch.Tensor) and img.shape == (cam.height, cam.width, 3)
    assert float((img.cpu() - exp_img).abs().mean()) < 1e-6


@pytest.mark.usefixtures("library_defaults")       # asserts WHICH mechanism served the calls: the defaults'
@pytest.mark.parametrize("channels", [1, 2, 5, 7])
def test_n_channel_colours_match_the_channel_generic_oracle(hip, c_oracle, torch_oracle, channels):
    """upstream's N-D rasterize path (D != 3): image, alpha and the gradients of every input against the channel-generic
    pure-PyTorch oracle; served by the 3-channel kernels three channels at a time over ONE binning."""
    from sgn_rast import ops
    cam, P = small_scene(n=1200)
    R = _raster_inputs(c_oracle, cam, P)
    g = torch.Generator().manual_seed(channels)
    cols = torch.rand(R["xys"].shape[0], channels, generator=g)
    bg = torch.rand(channels, generator=g)
    w_img = torch.rand(cam.height, cam.width, channels, generator=g)
    w_a = torch.rand(cam.height, cam.width, generator=g)

    def run(fn, dev):
        leaves = [R[k].to(dev).clone().requires_grad_(True) for k in ("xys", "conics")] + [
            cols.to(dev).clone().requires_grad_(True), R["opac"].to(dev).clone().requires_grad_(True)]
        img, alpha = fn(leaves[0], R["depths"].to(dev), R["radii"].to(dev), leaves[1], R["nth"].to(dev), leaves[2],
                        leaves[3], cam.height, cam.width, 16, bg.to(dev), True)
        ((img * w_img.to(dev)).sum() + (alpha * w_a.to(dev)).sum()).backward()
        return img.detach().cpu(), alpha.detach().cpu(), [l.grad.cpu() for l in leaves]
    ops.clear_binning_cache()
    b0 = ops.binning_stats["binnings"]
    ops.set_alpha_clamp_bwd(0.999)              # autograd through the oracle's forward clamps where the forward does
    try:
        got = run(hip.rasterize_gaussians, DEV)
    finally:
        ops.set_alpha_clamp_bwd(ops.UPSTREAM_ALPHA_CLAMP_BWD)
    assert ops.binning_stats["binnings"] == b0 + 1                  # every 3-channel pass after the first reuses the list
    exp = run(torch_oracle.rasterize_gaussians, "cpu")
    assert got[0].shape == (cam.height, cam.width, channels)
    assert float((got[0] - exp[0]).abs().mean()) < 1e-6 and float((got[1] - exp[1]).abs().mean()) < 1e-6
    for a, b in zip(got[2], exp[2]):
        assert rel_l2(a, b) < 1e-4
    # a single output without alpha, and a background of the wrong length is refused like upstream
    img = hip.rasterize_gaussians(R["xys"].to(DEV), R["depths"].to(DEV), R["radii"].to(DEV), R["conics"].to(DEV),
                                  R["nth"].to(DEV), cols.to(DEV), R["opac"].to(DEV), cam.height, cam.width, 16, bg.to(DEV))
    assert isinstance(img, torch.Tensor) and torch.equal(img.cpu(), got[0])
    with pytest.raises(AssertionError):
        hip.rasterize_gaussians(R["xys"].to(DEV), R["depths"].to(DEV), R["radii"].to(DEV), R["conics"].to(DEV),
                                R["nth"].to(DEV), cols.to(DEV), R["opac"].to(DEV), cam.height, cam.width, 16,
                                torch.zeros(3, device=DEV))


def test_tile_order_is_a_permutation_longest_first_and_changes_nothing(hip):
    """sgn_tile_order: a permutation of the tiles, non-increasing in half-octave length class; rendering with and
    without it gives bit-identical images (forward) and equal gradients."""
    from sgn_rast import _lib as L, ops, scenes, step
    g = torch.Generator().manual_seed(0)
    lens = torch.cat([torch.randint(0, 5000, (700,), generator=g), torch.zeros(100, dtype=torch.int64)])
    lens = lens[torch.randperm(lens.numel(), generator=g)]
    start = torch.cumsum(lens, 0) - lens
    bins = torch.stack([start, start + lens], 1).to(torch.int32).to(DEV)
    lib = L.load()
    nt = bins.shape[0]
    scratch = torch.zeros(int(lib.sgn_tile_order_scratch_bytes(nt)) // 4, dtype=torch.int32, device=DEV)
    # forward's statistics for the backward order: walk depth = half of each list, (entry, quadrant) pairs = 4 per entry
    kmax = torch.stack([start + lens // 2 - 1, 4 * (lens // 2)], 1).to(torch.int32).to(DEV)
    walked = torch.where(lens > 0, torch.minimum(lens, (lens // 2).clamp_min(0)), torch.zeros_like(lens))
    for sc in (None, scratch, scratch):               # single-workgroup form, multi-workgroup form (twice: self-cleaning)
        for stats in (None, kmax):
            order = torch.empty(nt + 2, dtype=torch.int32, device=DEV)
            L.check(lib.sgn_tile_order(nt, L.ptr(bins), L.ptr(stats), 512, 0, L.ptr(order), L.ptr(sc),
                                       0 if sc is None else 4 * sc.numel(), L.stream_ptr()), "sgn_tile_order")
            ln = lens if stats is None else walked
            assert int(order[-2]) == int((ln >= 512).sum())                  # n_long (512 is a class boundary)
            if stats is None:
                assert int(order[-1]) == 0
            else:
                assert abs(int(order[-1]) - int(1000 * walked.sum() // lens.sum())) <= 1   # walked / listed permille
            o = order[:-2].cpu().long()
            assert torch.equal(torch.sort(o).values, torch.arange(nt))
            cls = torch.where(ln[o] > 0, 1 + 2 * torch.floor(torch.log2(ln[o].clamp_min(1).double())).long(), 0)
            assert bool((cls[1:] <= cls[:-1] + 1).all()) and int(ln[o][0]) >= int(ln.max()) // 2
            if sc is not None:
                assert int(sc[:72].abs().sum()) == 0                       # left zero-filled for the next launch
    cam, raw = scenes.make_scene("c1", device=DEV)
    w_img, w_a = step.loss_weights(cam, seed=7, device=DEV)
    res = []
    for enabled, mb in ((True, True), (True, False), (False, True)):
        ops.tile_order_enabled, ops.tile_order_multiblock = enabled, mb
        ops.clear_binning_cache()
        try:
            P = step.leaf_params(raw)
            out = step.train_step(P, cam, w_img, w_a)
            res.append((out.rgb.detach().clone(), out.alpha.detach().clone(), {k: v.grad.clone() for k, v in P.items()}))
        finally:
            ops.tile_order_enabled = ops.tile_order_multiblock = True
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
        for k in res[0][2]:
            assert rel_l2(res[0][2][k], other[2][k]) < 1e-5, k

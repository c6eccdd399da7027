"""GPU (-m gpu): the rasterizer's shortcuts against the C oracle's full upstream walk on adversarial splat geometry.

Exact tile culling, the emission's quadrant masks and the raster rows' ex / ey extents each claim to change no image and
no gradient.  The C oracle (`bin_and_sort` + `raster_fwd` / `raster_bwd`) is upstream's definition — every tile of the
3-sigma square, every pixel of the tile — so in exact-exp mode the HIP forward must equal it BIT FOR BIT whatever
shortcut runs.  The scenes (tests/adversarial_scenes.py: needles, threshold opacities, near plane and frustum clamp,
huge splats, border placement, deep stacks, a 45 x 13 image) are built where those shortcuts' margins are thinnest;
tests/test_adversarial_scenes.py shows on the CPU that each family does what it is built for.
"""
import pytest
import torch

import adversarial_scenes as A
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BG = torch.tensor([0.1, 0.2, 0.3])
QMASK = (1 << 28) - 1

FAMILY_BLOCKS = [(name, blk) for name, fn in A.FAMILIES.items() for blk in fn().blocks]

# option combinations of the drop-in surface: culling off (the upstream-shaped list; masks need the culling) or on with
# quadrant masks off / on / auto; each under the default thresholds, the LDS-batched path forced on, and launch-order
# thresholds small enough that these scenes have tiles on both sides of the four-wave / long-walk split
SHORTCUTS = {"nocull": dict(tile_culling=False, quadrant_masks="off"),
             "cull": dict(tile_culling=True, quadrant_masks="off"),
             "cull-masks": dict(tile_culling=True, quadrant_masks="on"),
             "cull-auto": dict(tile_culling=True, quadrant_masks="auto")}
PATHS = {"default": dict(), "ldsbatch": dict(batch_fwd=24, batch_bwd=24),
         "split": dict(adapt_fwd=96, adapt_bwd=48, batch_fwd=1 << 30, batch_bwd=1 << 30)}


@pytest.fixture(scope="module")
def hip():
    from sgn_rast import _lib, ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return ops


@pytest.fixture(autouse=True)
def _fresh_binning():
    from sgn_rast import ops
    ops.clear_binning_cache()
    yield
    ops.clear_binning_cache()


_CACHE = {}


def _scene(name, block, c_oracle):
    """(scene, raster inputs, oracle list) — the oracle's projection and its full upstream binning, cached per module."""
    key = (name, block)
    if key not in _CACHE:
        sc = A.FAMILIES[name]()
        R = sc.raster_inputs(c_oracle, block)
        total = int(R["nth"].long().sum())
        assert 0 < total < 50_000_000, total          # host-side check of the list size before anything is launched
        _cum, _k, _v, _ks, vs, bins = c_oracle.bin_and_sort(R["xys"], R["depths"], R["radii"], R["nth"], sc.cam.height,
                                                            sc.cam.width, block)
        R["ids"], R["bins"] = vs, bins
        _CACHE[key] = (sc, R, {})
    return _CACHE[key]


def _oracle_fwd(c_oracle, sc, R, block, exact, opac=None, tag="drop-in"):
    memo = _CACHE[(sc.name, block)][2]
    k = ("fwd", exact, tag)
    if k not in memo:
        c_oracle.set_exp_mode(1 if exact else 0)
        try:
            memo[k] = c_oracle.raster_fwd(sc.cam.height, sc.cam.width, block, R["ids"], R["bins"], R["xys"], R["conics"],
                                          R["rgb"], R["opac"] if opac is None else opac, BG)
        finally:
            c_oracle.set_exp_mode(0)
    return memo[k]


def _hip_forward(sc, R, block, opts, grad=False, fused_logits=False, seed=3):
    """Drop-in (or fused, logit opacities) forward under `opts`; returns img, alpha, final T, final index, the Gaussian id
    of the last contributor per pixel (-1: none) and the leaves.  The leaves always require grad (the pass's saved state
    is read from its autograd node); `grad` runs the backward."""
    from sgn_rast import config, fused, ops
    d = {k: v.to(DEV) for k, v in R.items() if torch.is_tensor(v)}
    leaves = dict(xys=d["xys"].clone().requires_grad_(True), conics=d["conics"].clone().requires_grad_(True),
                  rgb=d["rgb"].clone().requires_grad_(True),
                  opac=(d["logits"] if fused_logits else d["opac"]).clone().requires_grad_(True))
    with config.override(**opts):
        ops.clear_binning_cache()
        if fused_logits:
            img, alpha = fused.rasterize_gaussians_fused(leaves["xys"], d["depths"], d["radii"], leaves["conics"],
                                                         d["nth"], leaves["rgb"], leaves["opac"], sc.cam.height,
                                                         sc.cam.width, block, BG.to(DEV), True)
        else:
            img, alpha = ops.rasterize_gaussians(leaves["xys"], d["depths"], d["radii"], leaves["conics"], d["nth"],
                                                 leaves["rgb"], leaves["opac"], sc.cam.height, sc.cam.width, block,
                                                 background=BG.to(DEV), return_alpha=True)
        node = img.grad_fn
        ids, fT, fi = node.saved_tensors[0], node.saved_tensors[7], node.saved_tensors[8]
        if grad:
            g = torch.Generator().manual_seed(seed)
            v_img = torch.randn(sc.cam.height, sc.cam.width, 3, generator=g)
            v_a = torch.randn(sc.cam.height, sc.cam.width, generator=g)
            torch.autograd.backward([img, alpha], [v_img.to(DEV), v_a.to(DEV)])
    torch.cuda.synchronize()
    ids = (ids & QMASK).cpu()
    fT, fi = fT.detach().cpu(), fi.detach().cpu()
    last = torch.where(fT < 1, ids[fi.long().clamp(0, max(ids.numel() - 1, 0))] if ids.numel() else fi, -1)
    return img.detach().cpu(), alpha.detach().cpu(), fT, fi, last, leaves


def _oracle_last(R, fT, fi):
    return torch.where(fT < 1, R["ids"][fi.long().clamp(0, max(R["ids"].numel() - 1, 0))] if R["ids"].numel() else fi,
                       -1)


# ------------------------------------------------------------------------------ forward, bit for bit (exact exp)
FWD_CASES = [(n, b, s) for n, b in FAMILY_BLOCKS for s in SHORTCUTS
             if b == 16 or SHORTCUTS[s]["quadrant_masks"] == "off"]          # (quadrant masks ride on 16x16 tiles only)


@pytest.mark.parametrize("path", list(PATHS), ids=list(PATHS))
@pytest.mark.parametrize("name,block,shortcut", FWD_CASES, ids=[f"{n}-b{b}-{s}" for n, b, s in FWD_CASES])
def test_forward_is_the_full_upstream_walk_bit_for_bit(hip, c_oracle, name, block, shortcut, path):
    from sgn_rast import ops
    sc, R, _ = _scene(name, block, c_oracle)
    e_img, e_T, e_idx = _oracle_fwd(c_oracle, sc, R, block, exact=True)
    if shortcut == "cull-auto":
        ops._S().walked_permille = 1000          # "auto" with the statistic of a translucent previous step: masks on
    try:
        img, alpha, fT, fi, last, _ = _hip_forward(sc, R, block, dict(SHORTCUTS[shortcut], exact_exp=1, **PATHS[path]))
    finally:
        ops._S().walked_permille = None
    assert torch.equal(fT, e_T), f"final T differs at {int((fT != e_T).sum())} pixels"
    assert torch.equal(img, e_img), f"image differs at {int((img != e_img).any(-1).sum())} pixels"
    assert torch.equal(alpha, 1 - e_T)
    if shortcut == "nocull":
        assert torch.equal(fi, e_idx)            # same list: the raw list positions agree too
    assert torch.equal(last, _oracle_last(R, e_T, e_idx)), "last contributing Gaussian differs"
    assert float((1 - e_T).sum()) > 0


@pytest.mark.parametrize("name", list(A.FAMILIES))
def test_fused_logit_forward_is_the_full_upstream_walk_bit_for_bit(hip, c_oracle, name):
    """The fused surface (sigmoid in the row build and in the culling threshold) with logit opacities, culling and masks
    on; the oracle is given the sigmoid the row build computes, 1 / (1 + expf(-x)) in fp32 on the device."""
    sc, R, _ = _scene(name, 16, c_oracle)
    lg = R["logits"].to(DEV)
    o_dev = (1.0 / (1.0 + torch.exp(-lg))).cpu()
    e_img, e_T, e_idx = _oracle_fwd(c_oracle, sc, R, 16, exact=True, opac=o_dev, tag="fused")
    img, alpha, fT, fi, last, _ = _hip_forward(sc, R, 16, dict(tile_culling=True, quadrant_masks="on", exact_exp=1),
                                               fused_logits=True)
    assert torch.equal(fT, e_T), f"final T differs at {int((fT != e_T).sum())} pixels"
    assert torch.equal(img, e_img)
    assert torch.equal(last, _oracle_last(R, e_T, e_idx))


# ------------------------------------------------------------------------ forward at production settings
@pytest.mark.parametrize("name", list(A.FAMILIES))
def test_production_forward_flips_stay_scattered(hip, c_oracle, name):
    """Hardware exp, library defaults (culling on, masks auto).  v_exp_f32 and libm's expf differ by ~1 ulp, so pixels
    whose walk puts the 1/255 or 1e-4 test between the two may composite one entry more or less (the oracle's
    threshold-adjacency test names them); every other pixel agrees to 1e-5.  A shortcut that drops a tile or a
    quadrant shows up as a CLUSTER of differing pixels: no 8x8 quadrant may hold more than 4 flips."""
    sc, R, _ = _scene(name, 16, c_oracle)
    e_img, e_T, _ = _oracle_fwd(c_oracle, sc, R, 16, exact=False)
    img, alpha, fT, fi, last, _ = _hip_forward(sc, R, 16, dict())
    adj = c_oracle.raster_threshold_adjacent(sc.cam.height, sc.cam.width, 16, R["ids"], R["bins"], R["xys"],
                                             R["conics"], R["opac"])
    err = torch.maximum((img - e_img).abs().amax(-1), (fT - e_T).abs())
    flips = err > 1e-5
    H, W = err.shape
    q = torch.nn.functional.pad(flips.float(), (0, (-W) % 8, 0, (-H) % 8)).reshape((H + 7) // 8, 8, (W + 7) // 8, 8)
    per_q = q.sum(dim=(1, 3))
    print(f"[flips] {name}: {int(flips.sum())} of {H * W} pixels (threshold-adjacent {int(adj.sum())}), "
          f"max per 8x8 quadrant {int(per_q.max())}, max|err| off the thresholds "
          f"{float(err[~adj].max()) if bool((~adj).any()) else 0.0:.1e}")
    assert not bool((flips & ~adj).any()), "a pixel away from every threshold differs"
    assert int(per_q.max()) <= 4
    assert float(err.max()) < 2e-2


# ---------------------------------------------------------------------------------------------- backward
# Per Gaussian: |g - e| <= RTOL |e| + ATOL max|e| (per column).  Same decisions on both sides (exact exp), so what is
# left is the order of the fp32 sums: the kernels reduce per wave and add with atomics in arbitrary order, the oracle
# sums pixel by pixel — a few hundred to ~1e5 terms per row, each rounding by 2^-24 of the running sum; with the
# cancellation of signed pixel weights that is < 1e-3 of |e| for every row here, and the ATOL term covers rows whose
# gradient cancels to ~0.  A dropped tip quadrant moves a row by the whole contribution of up to 64 pixels.
RTOL, ATOL = 2e-3, 2e-6


def _per_row_close(got, exp, what):
    got, exp = got.double().reshape(got.shape[0], -1), exp.double().reshape(exp.shape[0], -1)
    scale = exp.abs().amax(dim=0, keepdim=True)
    bad = (got - exp).abs() > RTOL * exp.abs() + ATOL * scale
    rows = torch.nonzero(bad.any(dim=1)).reshape(-1)
    assert rows.numel() == 0, (what, rows[:10].tolist(), got[rows[:3]].tolist(), exp[rows[:3]].tolist())


@pytest.mark.parametrize("name", list(A.FAMILIES))
def test_backward_per_gaussian_against_the_oracle(hip, c_oracle, name):
    sc, R, _ = _scene(name, 16, c_oracle)
    e_img, e_T, e_idx = _oracle_fwd(c_oracle, sc, R, 16, exact=True)
    g = torch.Generator().manual_seed(3)
    v_img = torch.randn(sc.cam.height, sc.cam.width, 3, generator=g)
    v_a = torch.randn(sc.cam.height, sc.cam.width, generator=g)
    from sgn_rast import ops
    clamp = ops.semantics().alpha_clamp_bwd
    c_oracle.set_exp_mode(1)
    try:
        exp = c_oracle.raster_bwd(sc.cam.height, sc.cam.width, 16, R["ids"], R["bins"], R["xys"], R["conics"], R["rgb"],
                                  R["opac"], BG, e_T, e_idx, v_img, v_a, clamp)
    finally:
        c_oracle.set_exp_mode(0)
    got = {}
    for cull in (True, False):
        *_, leaves = _hip_forward(sc, R, 16, dict(tile_culling=cull, quadrant_masks="on" if cull else "off",
                                                  exact_exp=1), grad=True, seed=3)
        got[cull] = [leaves[k].grad.cpu() for k in ("xys", "conics", "rgb", "opac")]
    for k, (a, b, e) in enumerate(zip(got[True], got[False], exp)):
        what = ("xys", "conics", "rgb", "opac")[k]
        assert float(e.abs().sum()) > 0, what
        assert rel_l2(a, e) < 1e-4, (what, rel_l2(a, e))
        _per_row_close(a, e, f"{name} {what} (culled, masks) vs oracle")
        _per_row_close(a, b, f"{name} {what} culled vs not")


# ------------------------------------------------------------------------- projection on the frustum family
def _project_hip(sc, semantics_clamped, with_grad):
    from sgn_rast import ops
    args = [t.to(DEV) if torch.is_tensor(t) else t for t in sc.project_args(16)]
    if with_grad:
        for i in (0, 1, 3):
            args[i] = args[i].clone().requires_grad_(True)
    with ops.upstream_variant(ewa_vjp_clamped=semantics_clamped):
        out = ops.project_gaussians(*args)
    return args, out


@pytest.mark.parametrize("name", ["frustum", "needles", "huge"])
def test_projection_forward_bit_exact(hip, c_oracle, name):
    sc = A.FAMILIES[name]()
    exp = c_oracle.project_fwd(*sc.project_args(16))
    _, got = _project_hip(sc, False, False)
    for what, a, b in zip(["xys", "depths", "radii", "conics", "compensation", "num_tiles_hit", "cov3d"], got, exp):
        assert torch.equal(a.cpu(), b), f"{what} differs: {(a.cpu().float() - b.float()).abs().max()}"


@pytest.mark.parametrize("clamped", [False, True], ids=["upstream-vjp", "clamped-vjp"])
def test_projection_backward_per_gaussian_on_the_frustum_family(hip, c_oracle, torch_oracle, clamped):
    """Rows whose centre lies past 1.3 tan(fov/2) (the forward clamps it, `clx` / `cly` in the vjp), on the near plane
    and behind the camera: the backward per row against the C oracle under both semantics, and under the clamped one
    against fp64 autograd through the torch oracle (whose forward clamps) too."""
    sc = A.FAMILIES["frustum"]()
    pa = sc.project_args(16)
    xys, depths, radii, conics, comp, nth, cov3d = c_oracle.project_fwd(*pa)
    n = radii.numel()
    g = torch.Generator().manual_seed(5)
    v_xy, v_d, v_con = torch.randn(n, 2, generator=g), torch.randn(n, generator=g), torch.randn(n, 3, generator=g)
    zeros = torch.zeros(n)
    sem = c_oracle.SEM_EWA_VJP_CLAMPED if clamped else 0
    exp = c_oracle.project_bwd(pa[0], pa[1], 1.0, pa[3], pa[4], sc.cam.fx, sc.cam.fy, cov3d, radii, conics, comp,
                               v_xy, v_d, v_con, zeros, sem, sc.cam.height, sc.cam.width)
    args, out = _project_hip(sc, clamped, True)
    torch.autograd.backward([out[0], out[1], out[3]], [v_xy.to(DEV), v_d.to(DEV), v_con.to(DEV)])
    live = radii > 0
    for what, leaf, e in zip(["v_mean", "v_scale", "v_quat"], (args[0], args[1], args[3]), exp[:3]):
        got = leaf.grad.cpu()
        assert (got[~live] == 0).all(), what
        # same formulas, fp32 both sides: per row to rounding of a chain of ~100 operations
        bad = (got - e).abs() > 1e-4 * e.abs() + 1e-6 * e.abs().amax(dim=0, keepdim=True)
        assert not bool(bad[live].any()), (what, torch.nonzero(bad.any(-1))[:5].reshape(-1).tolist())
    if clamped:
        D = torch.float64
        leaves = [pa[0].to(D).clone().requires_grad_(True), pa[1].to(D).clone().requires_grad_(True),
                  pa[3].to(D).clone().requires_grad_(True)]
        o = torch_oracle.project_gaussians(leaves[0], leaves[1], 1.0, leaves[2], pa[4].to(D), *pa[5:])
        lv = o[2] > 0
        ((o[0] * v_xy.to(D))[lv].sum() + (o[1] * v_d.to(D))[lv].sum() + (o[3] * v_con.to(D))[lv].sum()).backward()
        for what, leaf, ref in zip(["v_mean", "v_scale"], (args[0], args[1]), leaves[:2]):
            got = leaf.grad.cpu().double()[live]
            assert rel_l2(got, ref.grad[live]) < 2e-4, (what, rel_l2(got, ref.grad[live]))
    pv = pa[0]
    lim_x, lim_y = 1.3 * 0.5 * sc.cam.width / sc.cam.fx, 1.3 * 0.5 * sc.cam.height / sc.cam.fy
    clamped_rows = live & (((pv[:, 0] / pv[:, 2]).abs() > lim_x) | ((pv[:, 1] / pv[:, 2]).abs() > lim_y))
    assert int(clamped_rows.sum()) > 100


# ------------------------------------------------------------- dropped pairs and cleared bits: no valid pixel
@pytest.mark.parametrize("name", list(A.FAMILIES))
def test_dropped_pairs_and_cleared_quadrants_have_no_valid_pixel(hip, c_oracle, name):
    """The culled, masked list the emission writes against the truth: every (tile, Gaussian) pair of the upstream box
    with a pixel centre that passes the kernels' own fp32 validity test (kernel operation order, explicit fmas) is kept,
    with that quadrant's bit set; rows whose 255 o e^0.011 < 1 (nothing can ever be valid) are not listed at all."""
    from sgn_rast import ops
    sc, R, _ = _scene(name, 16, c_oracle)
    W, H = sc.cam.width, sc.cam.height
    d = {k: v.to(DEV) for k, v in R.items() if torch.is_tensor(v)}
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    old = ops.quadrant_masks
    ops.quadrant_masks = "on"
    try:
        st = ops._bin_prepare_async(sc.n, d["xys"], d["depths"], d["radii"], d["nth"], tb, 16, d["conics"], d["opac"],
                                    False, True)
        I, ids, bins = ops._bin_finish(st)
    finally:
        ops.quadrant_masks = old
    assert ids._sgn_qmask
    ids, bins = ids.cpu().long(), bins.cpu().long()
    gid, bits = ids & QMASK, (ids >> 28) & 0xF
    tile_of = torch.repeat_interleave(torch.arange(bins.shape[0]), bins[:, 1] - bins[:, 0])
    kept_key = tile_of * sc.n + gid
    Rd = dict(xys=d["xys"], conics=d["conics"], opac=d["opac"], radii=R["radii"])
    tg, tt, tbits = A.valid_pairs(Rd, W, H, 16, torch.nonzero(R["radii"] > 0).reshape(-1))
    tg, tt, tbits = tg.cpu(), tt.cpu(), tbits.cpu()
    truth_key = tt * sc.n + tg
    need = tbits != 0
    order = torch.argsort(kept_key)
    pos = torch.searchsorted(kept_key[order], truth_key[need]).clamp(max=max(kept_key.numel() - 1, 0))
    found = kept_key[order][pos] == truth_key[need]
    assert bool(found.all()), f"{int((~found).sum())} pairs with a valid pixel were dropped"
    kbits = bits[order][pos]
    missed = tbits[need] & ~kbits
    assert int((missed != 0).sum()) == 0, f"{int((missed != 0).sum())} cleared quadrant bits hide a valid pixel"
    never = (255.0 * R["opac"].reshape(-1).double() * torch.exp(torch.tensor(0.011, dtype=torch.float64))) < 1
    assert not bool(never[gid].any()), "a row that can never be visible was listed"
    n_box, n_kept, n_true = truth_key.numel(), kept_key.numel(), int(need.sum())
    print(f"[culling] {name}: box pairs {n_box}, kept {n_kept}, with a valid pixel {n_true}; quadrant bits set "
          f"{int(sum(((bits >> q) & 1).sum() for q in range(4)))}, needed {int(sum(((tbits >> q) & 1).sum() for q in range(4)))}")
    assert n_kept <= n_box and n_kept >= n_true

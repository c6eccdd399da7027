"""GPU (-m gpu): depth lists whose lengths sit on the boundaries of the rasterizers' walks (raster_common.h: walk_chase,
walk_staged; raster_features.hip: walk_uniform) — one entry, two, and one below / at / one above a multiple of the
64-entry batch — with every entry of the list reached.  The random scenes of the other modules reach the staged path
with whatever lengths their tiles happen to have.

Scene: a stack of N isotropic Gaussians (sigma 6 px) on one point, at increasing depth, activated opacity 0.02 each:
alpha = 0.02 >= 1/255 at the centre and 0.98^193 ~ 0.02 > 1e-4, so no pixel near the centre terminates and the walk
must reach the LAST entry — asserted on the C oracle's own final index, so that a changed scene cannot silently stop
short of the boundary.  Either one 16x16 tile with the stack in its middle, or two tiles (32x16) with the stack on the
seam between them.  `batch_fwd = batch_bwd` = 1 (every list staged through LDS) or 2^30 (every list chased); with
adapt_* = 64 the lists from 64 entries on also take the four-waves-per-tile kernels.  With and without quadrant masks in
the id words."""
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 193]
SCENES = {"one-tile": (16, 16, 8.0), "seam": (32, 16, 16.0)}       # W, H, x of the stack (y = 8)
BG = torch.tensor([0.1, 0.2, 0.3])
CLAMP_BWD = 0.99
_REF = {}


def _stack(scene, n):
    W, H, cx = SCENES[scene]
    g = torch.Generator().manual_seed(1000 * n + W)
    xys = torch.tensor([cx, 8.0]).repeat(n, 1)
    conics = torch.tensor([1.0 / 36.0, 0.0, 1.0 / 36.0]).repeat(n, 1)
    return dict(W=W, H=H, n=n, xys=xys, conics=conics, depths=1.0 + 0.01 * torch.arange(n, dtype=torch.float32),
                radii=torch.full((n,), 18, dtype=torch.int32), nth=torch.full((n,), W // 16, dtype=torch.int32),
                rgb=torch.rand(n, 3, generator=g), opac=torch.full((n, 1), 0.02),
                v_img=torch.randn(H, W, 3, generator=g), v_alpha=torch.randn(H, W, generator=g))


def _reference(c_oracle, scene, n):
    """The C oracle (portable exp) on the stack, once per (scene, N), left unchanged."""
    if (scene, n) not in _REF:
        S = _stack(scene, n)
        W, H = S["W"], S["H"]
        ids, bins = c_oracle.bin_and_sort(S["xys"], S["depths"], S["radii"], S["nth"], H, W, 16)[4:6]
        c_oracle.set_exp_mode(1)
        try:
            img, T, idx = c_oracle.raster_fwd(H, W, 16, ids, bins, S["xys"], S["conics"], S["rgb"], S["opac"], BG)
            grads = c_oracle.raster_bwd(H, W, 16, ids, bins, S["xys"], S["conics"], S["rgb"], S["opac"], BG, T, idx,
                                        S["v_img"], S["v_alpha"], CLAMP_BWD)
        finally:
            c_oracle.set_exp_mode(0)
        # the condition of the whole module: in every tile, some pixel composited the LAST entry of the list
        assert bins.shape[0] == W // 16 and int(ids.numel()) == n * (W // 16)
        for t in range(W // 16):
            lo, hi = int(bins[t, 0]), int(bins[t, 1])
            assert hi - lo == n
            assert int(idx[:, 16 * t:16 * t + 16].max()) == hi - 1, (scene, n, t)
        S.update(ids=ids, bins=bins, img=img, T=T, idx=idx, grads=grads)
        _REF[(scene, n)] = S
    return _REF[(scene, n)]


@pytest.fixture
def masks(request):
    from sgn_rast import ops
    old = ops.quadrant_masks
    ops.quadrant_masks = "on" if request.param else "off"
    ops.clear_binning_cache()
    yield bool(request.param)
    ops.quadrant_masks = old
    ops.clear_binning_cache()


@pytest.mark.parametrize("masks", [0, 1], ids=["box-test", "qmask"], indirect=True)
@pytest.mark.parametrize("adapt", [None, 64], ids=["two-waves", "four-waves-from-64"])
@pytest.mark.parametrize("batch", [1, 1 << 30], ids=["staged", "chase"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_lists_at_the_walk_boundaries_match_the_oracle(c_oracle, scene, batch, adapt, masks):
    from sgn_rast import _lib as L, ops
    L.load()
    kw = dict(exact_exp=1, batch_fwd=batch, batch_bwd=batch)
    if adapt:
        kw.update(adapt_fwd=adapt, adapt_bwd=adapt)
    ops.set_alpha_clamp_bwd(CLAMP_BWD)
    try:
        with L.options(**kw):
            for n in LENGTHS:
                R = _reference(c_oracle, scene, n)
                d = {k: v.to(DEV) for k, v in R.items() if torch.is_tensor(v)}
                leaves = {k: d[k].clone().requires_grad_(True) for k in ("xys", "conics", "rgb", "opac")}
                ops.clear_binning_cache()
                img, alpha = ops.rasterize_gaussians(leaves["xys"], d["depths"], d["radii"], leaves["conics"], d["nth"],
                                                     leaves["rgb"], leaves["opac"], R["H"], R["W"], 16,
                                                     background=BG.to(DEV), return_alpha=True)
                node = img.grad_fn
                assert bool(node.ro.ids_qmask) == masks
                ids, bins, final_T, final_idx = (node.saved_tensors[i] for i in (0, 1, 7, 8))
                # the list the kernels walked is the oracle's (quadrant bits on top of the ids)
                assert torch.equal(bins.cpu(), R["bins"]), n
                assert torch.equal((ids & ((1 << 28) - 1)).cpu(), R["ids"]), n
                assert torch.equal(final_idx.cpu(), R["idx"]), n
                assert torch.equal(final_T.cpu(), R["T"]), n
                assert torch.equal(img.detach().cpu(), R["img"]), n
                torch.autograd.backward([img, alpha], [d["v_img"], d["v_alpha"]])
                # the bound of test_gpu_parity.py::test_rasterize_backward
                for name, e in zip(("xys", "conics", "rgb", "opac"), R["grads"]):
                    err = rel_l2(leaves[name].grad.cpu(), e)
                    print(f"{scene} n={n} {name}: rel_l2 {err:.2e}")
                    assert err < 1e-4, (n, name, err)
    finally:
        ops.set_alpha_clamp_bwd(ops.UPSTREAM_ALPHA_CLAMP_BWD)


@pytest.mark.parametrize("masks", [0, 1], ids=["box-test", "qmask"], indirect=True)
@pytest.mark.parametrize("K", [5, 17])
@pytest.mark.parametrize("scene", list(SCENES))
def test_feature_walk_at_the_same_lengths_equals_the_three_channel_passes(c_oracle, scene, K, masks):
    from sgn_rast import _lib as L, features as F, ops
    L.load()
    for exact in (1, 0):
        for n in LENGTHS:
            R = _reference(c_oracle, scene, n)
            d = {k: v.to(DEV) for k, v in R.items() if torch.is_tensor(v)}
            g = torch.Generator().manual_seed(100 * K + n)
            feats, bg = torch.randn(n, K, generator=g).to(DEV), (torch.rand(K, generator=g) + 0.1).to(DEV)
            geo = (d["xys"], d["depths"], d["radii"], d["conics"], d["nth"])
            with L.options(exact_exp=exact), torch.no_grad():
                out, alpha = F.rasterize_features(*geo, feats, d["opac"], R["H"], R["W"], background=bg,
                                                  return_alpha=True)
                ref, ref_alpha = ops.rasterize_gaussians(*geo, feats, d["opac"], R["H"], R["W"], 16, bg, True)
            assert torch.equal(alpha, ref_alpha), (n, exact)
            assert torch.equal(out, ref), (n, exact, float((out - ref).abs().max()))
            if exact:     # ... and the transmittance is the oracle's, so the whole stack was walked here too
                assert torch.equal(alpha.cpu(), 1 - R["T"]), n

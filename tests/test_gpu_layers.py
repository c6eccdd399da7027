"""GPU (-m gpu): the layered evaluation forward (`sgn_raster_layers_fwd`, `sgn_rast.layers.rasterize_layers`) against
what it replaces — three calls of the existing forward over the same list with `id_range` None, (0, s) and (s, n) — and
the finishing launch (`sgn_layers_finish`) against the eager torch expressions of the reference's eval mode.

Forward: BIT-EQUAL images (`C + T * background`, a non-zero background), accumulations `1 - T` and depth channel, with
the hardware exp and the portable one, on short lists (scalar chase, two waves per tile) and on lists that cross several
64-entry batches (LDS-batched walk, four waves per tile), with the objects layer on its own compacted list and on the
shared one, at 328x200 (partial tiles on both edges)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, FOCAL = 328, 200, 260.0
BG = (0.3, 0.55, 0.8)


def _raw(kind, n, seed):
    """Raw Gaussians + split.  Ids below the split are the background ("head"), the others the objects ("tail")."""
    from sgn_rast import scenes
    cam = scenes.make_camera(W, H, FOCAL)
    z = (1.5, 9.0) if n <= 6000 else (1.0, 3.0)       # close-up: lists of several hundred entries per tile
    if kind in ("random", "split0", "splitn"):
        raw = scenes.make_gaussians(n, cam, seed=seed, z_range=z)
        return cam, raw, {"random": int(0.85 * n), "split0": 0, "splitn": n}[kind]
    s = int(0.8 * n)
    if kind == "wall":
        # an opaque wall at the back, translucent objects in front of it: the objects take part of the all-layer's
        # transmittance, so the all-layer saturates on the wall BEFORE the head layer does
        head = scenes.make_gaussians(s, cam, seed=seed, z_range=(z[1], 1.2 * z[1]))
        head["opacity_logits"].fill_(5.0); head["log_scales"] += 0.7
        tail = scenes.make_gaussians(n - s, cam, seed=seed + 1, z_range=(z[0], 0.9 * z[1]))
        tail["opacity_logits"].fill_(-1.0)
    elif kind == "occluders":
        # opaque objects in front of an ordinary background: the all-layer dies on them, the head layer is alive behind
        head = scenes.make_gaussians(s, cam, seed=seed, z_range=(0.6 * z[1], 1.2 * z[1]))
        tail = scenes.make_gaussians(n - s, cam, seed=seed + 1, z_range=(z[0], 1.5 * z[0]))
        tail["opacity_logits"].fill_(5.0); tail["log_scales"] += 0.7
    else:
        raise ValueError(kind)
    return cam, {k: torch.cat([head[k], tail[k]]) for k in head}, s


_CACHE = {}


def _inputs(kind, n):
    """Projected geometry, colours and logits on the device; computed once per (scene, size) and left unchanged."""
    if (kind, n) not in _CACHE:
        from sgn_rast import fused
        cam, raw, split = _raw(kind, n, seed=n % 97)
        P = {k: v.to(DEV) for k, v in raw.items()}
        with torch.no_grad():
            xys, depths, radii, conics, _c, nth, _cov = fused.project_gaussians_fused(
                P["means"], P["log_scales"], P["quats"], cam.viewmat[:3, :].to(DEV), cam.fx, cam.fy, cam.cx, cam.cy, H, W, 16)
        colors = torch.rand(n, 3, generator=torch.Generator().manual_seed(n + 1)).to(DEV) * 1.3
        _CACHE[(kind, n)] = ((xys, depths, radii, conics, nth), colors, P["opacity_logits"], split)
    return _CACHE[(kind, n)]


def _separate(geo, colors, logits, bg, id_range):
    from sgn_rast import fused
    with torch.no_grad():
        out = fused.rasterize_gaussians_fused(*geo, colors, logits, H, W, 16, background=bg, return_alpha=True,
                                              id_range=id_range, depth_channel=id_range is None)
    return out


SIZES = [
    # n, kernel options                             what the walks look like
    (6000, dict()),                                 # production thresholds: scalar chase, two waves per tile
    (20000, dict(adapt_fwd=192, batch_fwd=64)),     # several 64-entry batches per list; the longest get four waves
]
SCENES = [("random", True), ("random", False), ("wall", True), ("wall", False), ("occluders", True),
          ("occluders", False), ("split0", True), ("splitn", True)]


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("n,kw", SIZES)
@pytest.mark.parametrize("kind,own", SCENES)
def test_layers_equal_the_separate_passes_bit_for_bit(kind, own, n, kw, exact):
    from sgn_rast import _lib as L, layers, ops
    geo, colors, logits, split = _inputs(kind, n)
    bg = torch.tensor(BG, device=DEV)
    ops.clear_binning_cache()
    with L.options(exact_exp=exact, **kw):
        before = dict(layers.stats)
        img, Ts, D = layers.rasterize_layers(*geo, colors, logits, H, W, 16, bg, split, own_list=own)
        assert layers.stats["calls"] == before["calls"] + 1
        assert layers.stats["own_lists"] == before["own_lists"] + int(own and 0 < split < n)
        ranges = [None, (0, split), (split, n)]
        sep = [_separate(geo, colors, logits, bg, r) if (r is None or r[1] > r[0]) else None for r in ranges]
    torch.cuda.synchronize()
    assert img.shape == (3, H, W, 3) and Ts.shape == (3, H, W) and D.shape == (H, W)
    acc = 1 - Ts
    for l, (name, ref) in enumerate(zip(("all", "head", "tail"), sep)):
        if ref is None:                      # an empty id range: nothing composited, the background shows through
            assert torch.equal(Ts[l], torch.ones_like(Ts[l])) and torch.equal(img[l], bg.expand(H, W, 3)), name
            continue
        assert torch.equal(img[l], ref[0]), (name, "img", float((img[l] - ref[0]).abs().max()))
        assert torch.equal(acc[l], ref[1]), (name, "T", float((acc[l] - ref[1]).abs().max()))
        assert float(acc[l].max()) > 0.2, name          # not a comparison of blank images
    assert torch.equal(D, sep[0][2]), float((D - sep[0][2]).abs().max())
    assert float(D.max()) > 0.2
    if kind == "wall":         # the wall saturates its pixels, and objects stand in front of some of them
        assert bool(((acc[1] > 0.99) & (acc[2] > 0.2)).any())
    if kind == "occluders":    # the all-layer is finished on the objects; the background behind them is still rendered
        assert bool(((acc[2] > 0.999) & (acc[1] > 0.2)).any())


def test_layers_over_a_list_that_carries_quadrant_masks():
    """Quadrant masks in the top bits of the id words: layer membership is decided on the id bits alone."""
    from sgn_rast import layers, ops
    geo, colors, logits, split = _inputs("random", 6000)
    bg = torch.tensor(BG, device=DEV)
    saved = ops.quadrant_masks
    ops.quadrant_masks = "on"
    try:
        ops.clear_binning_cache()
        before = ops.quadrant_mask_stats["binnings_with_masks"]
        img, Ts, D = layers.rasterize_layers(*geo, colors, logits, H, W, 16, bg, split)
        assert ops.quadrant_mask_stats["binnings_with_masks"] == before + 1
        sep = [_separate(geo, colors, logits, bg, r) for r in (None, (0, split), (split, 6000))]
    finally:
        ops.quadrant_masks = saved
        ops.clear_binning_cache()
    for l in range(3):
        assert torch.equal(img[l], sep[l][0]) and torch.equal(1 - Ts[l], sep[l][1]), l
    assert torch.equal(D, sep[0][2])


def test_other_tile_sizes_are_refused():
    from sgn_rast import _lib as L, layers
    geo, colors, logits, split = _inputs("random", 6000)
    with pytest.raises(L.SgnRastError):
        layers.rasterize_layers(*geo, colors, logits, H, W, 8, torch.tensor(BG, device=DEV), split)


@pytest.mark.parametrize("with_sky", [True, False])
def test_finishing_launch_equals_the_eager_expressions(with_sky):
    """`sgn_layers_finish` against sgn_splatfacto.py:968-996 (eval mode) written in eager torch on the same inputs.
    BIT equality, not 1 ulp: the kernel's translation unit is built with floating-point contraction off and spells no
    fma, and the eager expressions are separate kernels (product, product, sum), so neither side contracts."""
    from sgn_rast import layers
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(3, H, W, 3, generator=g) * 1.9 - 0.3).to(DEV)       # raster values above 1 (and below 0)
    Ts = torch.rand(3, H, W, generator=g)
    # accumulations on both sides of the 1e-3 depth threshold, constructed: a = 0, just below, at, just above, 1
    for row, a in enumerate((0.0, 5e-4, 9.99e-4, 1e-3, 1.001e-3, 2e-3, 1.0)):
        Ts[:, row, :] = 1.0 - a
    Ts = Ts.to(DEV)
    D = (torch.rand(H, W, generator=g) * 30).to(DEV)
    sky = (torch.rand(H, W, 3, generator=g) * 1.2).to(DEV) if with_sky else None
    rgb, acc, depth = layers.finish(img, Ts, D, sky)
    torch.cuda.synchronize()
    a = (1 - Ts)[..., None]
    assert bool((a[0] > 1e-3).any()) and bool(((a[0] <= 1e-3) & (a[0] > 0)).any()) and float(img.max()) > 1
    for l in range(3):
        want = torch.clamp(img[l], max=1.0)                                            # :969
        if with_sky and l < 2:                                                         # the objects get no sky (:371)
            want = want * a[l] + sky * (1 - a[l])                                      # :972
        want = want.clamp(0.0, 1.0)                                                    # :975
        assert torch.equal(rgb[l], want), (l, float((rgb[l] - want).abs().max()))
        assert torch.equal(acc[l], 1 - Ts[l]), l
    want_depth = torch.where(a[0] > 1e-3, D[..., None] / a[0], 10)                     # :995
    assert torch.equal(depth[..., None], want_depth), float((depth[..., None] - want_depth).abs().max())
    assert bool((depth == 10).any()) and bool((depth != 10).any())

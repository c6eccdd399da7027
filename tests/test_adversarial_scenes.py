"""CPU: the adversarial scene families (tests/adversarial_scenes.py) are not vacuous.

Each family is meant to put a shortcut of the rasterizer where its margins are thinnest; measured here with the C
oracle's projection and the kernels' own fp32 validity test, so that the GPU comparisons in
tests/test_gpu_adversarial_geometry.py cannot pass because a scene quietly missed its target.
"""
import math

import pytest
import torch

import adversarial_scenes as A

BINREC_RAD_MAX = (1 << 30) - 1


def _truth(sc, R, block=16, rows=None):
    live = torch.nonzero(R["radii"] > 0).reshape(-1)
    if rows is not None:
        live = live[:rows]
    return A.valid_pairs(R, sc.cam.width, sc.cam.height, block, live)


@pytest.mark.parametrize("name", list(A.FAMILIES))
def test_family_is_deterministic_finite_and_bounded(c_oracle, name):
    a, b = A.FAMILIES[name](), A.FAMILIES[name]()
    for k in a.raw:
        assert torch.equal(a.raw[k], b.raw[k]), k
        assert bool(torch.isfinite(a.raw[k]).all()), k
    assert torch.equal(a.opacity, b.opacity) and bool(((a.opacity > 0) & (a.opacity <= 1)).all())
    for block in a.blocks:
        R = a.raster_inputs(c_oracle, block)
        total = int(R["nth"].long().sum())
        assert 0 < total < (1 << 31) // 16, total          # the intersection count stays far inside int32
        assert int(R["radii"].min()) >= 0 and bool(torch.isfinite(R["conics"]).all())
        # the snapped tile counts are the projection's own (tile_boxes restates its arithmetic)
        if a.snap_xy is None:
            assert torch.equal(A.tile_count(R["xys"], R["radii"], a.cam.width, a.cam.height, block)[R["radii"] > 0],
                               R["nth"][R["radii"] > 0])


@pytest.mark.parametrize("name", [n for n in A.FAMILIES if n != "huge"])
def test_culling_and_masks_have_something_to_drop(c_oracle, name):
    """Every family except `huge` (whose rows cover the image) has upstream box pairs without a valid pixel (the culling
    can drop them) and listed-and-valid pairs with an empty quadrant (the masks can clear a bit)."""
    sc = A.FAMILIES[name]()
    R = sc.raster_inputs(c_oracle, 16)
    g, t, bits = _truth(sc, R, rows=300)
    assert int((bits == 0).sum()) >= 20, (int((bits == 0).sum()), bits.numel())
    partial = (bits != 0) & (bits != 0xF)
    assert int(partial.sum()) > 20, int(partial.sum())


def test_needles(c_oracle):
    sc = A.needles()
    R = sc.raster_inputs(c_oracle, 16)
    live = R["radii"] > 0
    an = A.anisotropy(R["conics"])
    g, t, bits = _truth(sc, R)
    tiles_valid = torch.bincount(g[bits != 0], minlength=sc.n)
    long_thin = live & (an >= 100) & (tiles_valid >= 3)
    assert int(long_thin.sum()) >= 100, int(long_thin.sum())
    # (long, thin AND at the opacity edge: the valid region is a sliver of the ellipse)
    o255 = 255 * R["opac"].reshape(-1)
    assert int((long_thin & (o255 < 1.5)).sum()) >= 20
    assert int((long_thin & (R["opac"].reshape(-1) >= 0.999)).sum()) >= 20
    # long: valid regions spanning tens of tiles; the 3-sigma boxes of the longest reach thousands of tiles
    assert int(tiles_valid.max()) >= 60 and int(R["nth"].max()) >= 2000
    # in-plane angles of the long axis: every listed one occurs among the rows
    q = sc.quats()
    theta = 2 * torch.atan2(q[:, 3], q[:, 0])
    for ang in (0.0, 0.3, math.pi / 4, 1.0, math.pi / 2):
        assert int(((theta.abs() - ang).abs() < 1e-4).sum()) >= 10, ang
    # some tips leave the image: the valid region reaches the border tiles
    tx, ty = (sc.cam.width + 15) // 16, (sc.cam.height + 15) // 16
    edge = ((t % tx == 0) | (t % tx == tx - 1) | (t // tx == 0) | (t // tx == ty - 1)) & (bits != 0)
    assert int(torch.unique(g[edge]).numel()) >= 10


def test_thresholds(c_oracle):
    sc = A.thresholds()
    R = sc.raster_inputs(c_oracle, 16)
    live = R["radii"] > 0
    o = R["opac"].reshape(-1)
    g, t, bits = _truth(sc, R)
    has_valid = torch.bincount(g[bits != 0], minlength=sc.n) > 0
    edge = live & (255 * o >= 1) & (255 * o <= 1.05)
    assert int(edge.sum()) >= 100 and int((edge & has_valid).sum()) >= 30, (int(edge.sum()), int((edge & has_valid).sum()))
    below = live & (255 * o < 1)
    assert int(below.sum()) >= 100 and not bool((below & has_valid).any())
    assert int((live & (o >= 0.999)).sum()) >= 100
    lg = R["logits"].reshape(-1)
    for v in (8.0, -8.0, 20.0, -20.0):
        assert int((lg == v).sum()) >= 5, v
    one = torch.tensor(A.LOGIT_1_255)
    near = (lg == one) | (lg == torch.nextafter(one, torch.tensor(1.0))) | (lg == torch.nextafter(one, torch.tensor(-1.0)))
    assert int(near.sum()) >= 15


def test_frustum(c_oracle):
    sc = A.frustum()
    R = sc.raster_inputs(c_oracle, 16)
    live = R["radii"] > 0
    pv = sc.raw["means"]
    z = pv[:, 2]
    lim_x, lim_y = 1.3 * 0.5 * sc.cam.width / sc.cam.fx, 1.3 * 0.5 * sc.cam.height / sc.cam.fy
    clamped = live & (((pv[:, 0] / z).abs() > lim_x) | ((pv[:, 1] / z).abs() > lim_y))
    assert int(clamped.sum()) > 100, int(clamped.sum())
    near = (z > 0.01) & (z <= 0.05)
    assert int((near & live).sum()) >= 50
    assert int((z == 0.01).sum()) >= 10 and not bool(live[z == 0.01].any())           # the clip: culled
    nxt = torch.nextafter(torch.tensor(0.01), torch.tensor(1.0))
    assert int((z == nxt).sum()) >= 10 and bool(live[z == nxt].all())                 # the next float: live
    assert int((z < 0).sum()) >= 100 and not bool(live[z < 0].any())
    g, t, bits = _truth(sc, R)
    reach = torch.bincount(g[bits != 0], minlength=sc.n) > 0
    assert int((clamped & reach).sum()) > 100                                         # ... and they do reach the image


def test_huge(c_oracle):
    sc = A.huge()
    R = sc.raster_inputs(c_oracle, 16)
    W, H = sc.cam.width, sc.cam.height
    assert int((R["radii"] > max(W, H)).sum()) >= 0.9 * sc.n                          # larger than the image
    assert int((R["radii"] > BINREC_RAD_MAX).sum()) >= 5
    assert int(R["nth"].long().sum()) < (1 << 31) // 16
    full = ((W + 15) // 16) * ((H + 15) // 16)
    assert int((R["nth"] == full).sum()) >= 100                                       # whole-image tile rows
    g, t, bits = _truth(sc, R, rows=24)
    assert int((bits == 0xF).sum()) > 0.5 * bits.numel()


@pytest.mark.parametrize("name", ["placement", "placement_small"])
def test_placement(c_oracle, name):
    sc = A.FAMILIES[name]()
    W, H = sc.cam.width, sc.cam.height
    assert (W < 16 or H < 16 or name == "placement") and (name == "placement" or (W % 8 and H % 8))
    for block in sc.blocks:
        R = sc.raster_inputs(c_oracle, block)
        live = R["radii"] > 0
        x, y = R["xys"][:, 0], R["xys"][:, 1]
        on = lambda v, m: (v % m == 0)
        assert int((live & on(x, 16) & on(y, 16)).sum()) >= (5 if name == "placement_small" else 30)
        assert int((live & on(x, 8) & ~on(x, 16)).sum()) >= 5
        assert int((live & (x % 1 == 0.5) & (y % 1 == 0.5)).sum()) >= 10
        assert int((live & (x < 0)).sum()) >= 10 and int((live & ((x > W) | (y > H))).sum()) >= 10
        g, t, bits = _truth(sc, R, block)
        has_valid = torch.bincount(g[bits != 0], minlength=sc.n) > 0
        sub = live & (R["conics"][:, 0] > 3.0)                 # cov2d at the 0.3 floor: conic ~ 1/0.3
        assert int(sub.sum()) >= 30
        assert int((sub & ~has_valid).sum()) >= 5              # slipped between the pixel centres: listed, never valid
        assert int((sub & has_valid).sum()) >= 5


def test_stacks(c_oracle):
    sc = A.stacks()
    for block in sc.blocks:
        R = sc.raster_inputs(c_oracle, block)
        _c, _k, _v, _ks, vs, bins = c_oracle.bin_and_sort(R["xys"], R["depths"], R["radii"], R["nth"], sc.cam.height,
                                                          sc.cam.width, block)
        lens = bins[:, 1] - bins[:, 0]
        assert int(lens.max()) >= 250 and int((lens > 64).sum()) >= 4 and int((lens < 24).sum()) >= 1
        d = R["depths"][R["radii"] > 0]
        assert d.numel() - torch.unique(d).numel() >= 100                     # exact depth ties
        c_oracle.set_exp_mode(1)
        try:
            img, T, idx = c_oracle.raster_fwd(sc.cam.height, sc.cam.width, block, vs, bins, R["xys"], R["conics"],
                                              R["rgb"], R["opac"], torch.zeros(3))
        finally:
            c_oracle.set_exp_mode(0)
        # saturation (the walk stops at T <= 1e-4) reached inside the list, past the first 64-entry batch somewhere
        tiles_x = (sc.cam.width + block - 1) // block
        py, px = torch.meshgrid(torch.arange(sc.cam.height), torch.arange(sc.cam.width), indexing="ij")
        start = bins[(py // block) * tiles_x + px // block, 0]
        depth_in_list = idx - start
        assert int((T < 1e-3).sum()) > 0 and int(((T < 1e-3) & (depth_in_list > 64)).sum()) > 0
        assert int(((T > 0.5) & (depth_in_list > 64)).sum()) > 0              # ... and lists walked to the end unsaturated

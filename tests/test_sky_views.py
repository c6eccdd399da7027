"""CPU: the sky view families (tests/sky_views.py) reach the TileAcc paths they are built for, and the C oracle's
kernel-order exports (cube_taps, sky_dirs, cube_texture_f32, sky_blend_f32) agree with the independent restatements.

The targets are measured with the oracle's taps and a numpy model of the window routing (sky_views.routing), so that
tests/test_gpu_sky_per_texel.py cannot pass because a family quietly stopped covering its path.
"""
import numpy as np
import pytest
import torch

import sky_views as SV
from oracle import torch_oracle as O

VIEWS = SV.all_views()


def _taps(c_oracle, v, b=0):
    if v.dirs is None:
        d = c_oracle.sky_dirs(v.h, v.w, v.fx, v.fy, v.cx, v.cy, v.c2w(), v.jitter)
    else:
        d = v.dirs[b].reshape(-1, 3)
    off, w = c_oracle.cube_taps(d, v.R)
    return d.numpy(), off.numpy(), w.numpy()


def _stats(c_oracle, v, b=0):
    d, off, w = _taps(c_oracle, v, b)
    h, wd = v.grid()
    r = SV.routing(off, h, wd, v.R, v.C)
    lf = SV.face_of(d)
    valid_dir = lf >= 0
    taps = (off >= 0).sum()
    edge = (r["face"] >= 0) & (r["face"] != lf[:, None])
    tf = (r["tile"][:, None] * 8 + r["face"]).reshape(-1)
    tf = np.unique(tf[r["face"].reshape(-1) >= 0])
    faces_per_tile = np.bincount(tf // 8, minlength=len(r["anchor_face"]))
    return dict(d=d, off=off, w=w, r=r, valid_dir=valid_dir, taps=int(taps), lds=int(r["lds"].sum()),
                glob=int(r["glob"].sum()), edge=edge, corner=(off < 0) & valid_dir[:, None],
                faces_per_tile=faces_per_tile, runs=SV.row_runs(off, h, wd))


@pytest.mark.parametrize("name", list(VIEWS))
def test_view_is_deterministic_and_its_taps_are_sane(c_oracle, name):
    a = VIEWS[name]
    b = {v.name: v for v in SV.FAMILIES[name.split("/")[0]]()}[name]
    assert torch.equal(a.c2w(), b.c2w()) or bool(torch.isnan(a.c2w()).any())
    for x, y in ((a.jitter, b.jitter), (a.dirs, b.dirs)):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(torch.nan_to_num(x, 7.0), torch.nan_to_num(y, 7.0))
    for bi in range(a.batch):
        d, off, w = _taps(c_oracle, a, bi)
        ok = SV.face_of(d) >= 0
        assert int(off.max()) < 6 * a.R * a.R and int(off.min()) >= -1
        assert (off[~ok] == -1).all() and (w[~ok] == 0).all()
        assert (off[ok] >= 0).sum(1).min() >= 3                   # at most the corner tap is dropped
        s = w[ok].astype(np.float64).sum(1)
        assert np.abs(s - 1).max() < 4e-7                          # renormalised to one
        assert ((w >= 0) & (w <= 1)).all()
    if a.dirs is None:
        assert len(a.c2w().shape) == 2 and a.c2w().stride(-1) == 1


def test_production_taps_go_through_the_window(c_oracle):
    glob = 0
    for v in SV.production():
        assert (v.h, v.w, v.fx, v.fy, v.R, v.C) == (1280, 1920, 2000.0, 2000.0, 1024, 3)
        s = _stats(c_oracle, v)
        assert s["lds"] >= 0.99 * s["taps"], (v.name, s["lds"] / s["taps"])
        glob += s["glob"]
        assert (s["runs"] >= 2).sum() > 0.2 * (s["runs"] > 0).sum(), v.name   # real runs for the scan to sum
    assert glob > 0                                                 # a few seam tiles still take the global path
    poses = {v.name.split("/")[1] for v in SV.production()}
    assert poses == set(SV.PROD_POSES) and any(v.jitter is None for v in SV.production())
    assert any(v.jitter is not None for v in SV.production())


def test_magnified_views_have_full_row_runs_and_edge_taps(c_oracle):
    for v in SV.magnified():
        s = _stats(c_oracle, v)
        emit = s["runs"] > 0
        assert (s["runs"] == 16).sum() > 0.5 * emit.sum(), v.name  # most pixel rows of a tile are one run
        if v.R > 1:
            assert s["lds"] >= 0.5 * s["taps"], v.name
        else:                                                       # the two edge taps are on other faces: global
            assert s["lds"] > 0.3 * s["taps"] and s["glob"] > 0.6 * s["taps"]
        tiles = s["faces_per_tile"]
        assert (tiles >= 2).sum() > 0, v.name
        if v.R == 1:                                                # one on-face tap, two edge taps, one dropped corner
            assert (s["corner"].sum(1) == 1).all() and (s["edge"].sum(1) == 2).all()
            assert ((s["off"] >= 0) & ~s["edge"]).sum(1).tolist() == [1] * (v.h * v.w)


def test_minified_views_take_the_global_path(c_oracle):
    for v in SV.minified():
        s = _stats(c_oracle, v)
        assert v.w % 16 and v.h % 16                                # ragged last tiles in both directions
        assert s["glob"] > 0.6 * s["taps"], (v.name, s["glob"] / s["taps"])
        assert s["lds"] > 0, v.name                                 # the corner pixels' own taps


def test_seam_views_span_faces_and_drop_corner_taps(c_oracle):
    dropped = 0
    for v in SV.seams():
        s = _stats(c_oracle, v)
        tiles = s["faces_per_tile"]
        assert (tiles >= 2).sum() >= 10 and (tiles >= 3).sum() >= 1, (v.name, np.bincount(tiles))
        assert s["edge"].sum() >= 100, v.name
        lds_edge = (s["edge"] & s["r"]["lds"]).sum()
        glob_onface = (~s["edge"] & s["r"]["glob"]).sum()
        assert lds_edge > 0 and glob_onface > 0, v.name             # both arms of the face check, both ways round
        dropped += int(s["corner"].sum())
    assert dropped >= 50, dropped                                   # dropped corner taps, renormalised lookups


def test_invalid_views_put_invalid_directions_on_tile_corners(c_oracle):
    for v in SV.invalid():
        s = _stats(c_oracle, v)
        a = s["r"]["anchor_face"]
        assert (a < 0).sum() >= 2 and (a >= 0).sum() >= 2, v.name  # hdr[0] = -1 tiles and normal ones
        bad = ~s["valid_dir"]
        assert bad.sum() > len(a) and bad.sum() < 0.2 * bad.size
        dead = a[s["r"]["tile"]] < 0
        assert ((s["off"] >= 0) & dead[:, None]).sum() > 100        # valid taps of anchor-less tiles: all global
        assert s["r"]["glob"][dead].sum() == (s["off"][dead] >= 0).sum()


def test_channel_views_cover_the_window_and_the_bypass(c_oracle):
    Cs = set()
    for v in SV.channels():
        s = _stats(c_oracle, v)
        Cs.add(v.C)
        if v.C > SV.SKY_CMAX:
            assert s["lds"] == 0 and s["glob"] == s["taps"]
        else:
            assert s["lds"] > 0.5 * s["taps"], (v.name, s["lds"] / s["taps"])
    assert Cs == {1, 2, 4, 5, 8} and SV.SKY_CMAX in Cs


def test_layout_views(c_oracle):
    L = {v.name: v for v in SV.layouts()}
    assert L["layouts/flat"].grid() == (1, 40 * 130) and L["layouts/flat"].dirs.dim() == 3
    s = _stats(c_oracle, L["layouts/flat"])
    assert (s["runs"] >= 2).sum() > 0                               # a 16-lane row of the flat grid: 16 pixels of a row
    assert L["layouts/batch2"].batch == 2 and L["layouts/batch2"].dirs.shape == (2, 72, 100, 3)
    strides = sorted(v.c2w().stride(0) for v in L.values() if "c2w" in v.name)
    assert strides == [3, 4, 8]


# ---------------------------------------------------------------- the oracle's kernel-order exports
def test_sky_dirs_restate_env_light_directions(c_oracle):
    """sgo_sky_dirs (the kernel's fmaf order) against the torch restatement of EnvLight (matmul): a few ulps."""
    for name in ("layouts/c2w-3x3-of-4x4", "layouts/c2w-3x4-of-3x8", "minified/200x120", "seams/corner/R6"):
        v = VIEWS[name]
        got = c_oracle.sky_dirs(v.h, v.w, v.fx, v.fy, v.cx, v.cy, v.c2w(), v.jitter)
        m = v.c2w()[:, :3].contiguous()
        want = O.env_light_directions(v.h, v.w, v.fx, v.fy, v.cx, v.cy, m, v.jitter).reshape(-1, 3)
        assert bool(torch.isfinite(got).all())
        assert float((got - want).abs().max()) < 4e-7, name
        assert float((got.double().norm(dim=1) - 1).abs().max()) < 4e-7


def test_kernel_order_forward_matches_the_fp64_lookup(c_oracle):
    g = torch.Generator().manual_seed(3)
    for name in ("seams/corner/R6", "invalid/160x96/R64", "channels/corner/C5"):
        v = VIEWS[name]
        d = v.texture_dirs(c_oracle)[0].reshape(-1, 3)
        tex = torch.rand(6, v.R, v.R, v.C, generator=g)
        gout = torch.randn(d.shape[0], v.C, generator=g)
        f32 = c_oracle.cube_texture_f32(tex, d)
        f64, v_tex = c_oracle.cube_texture(tex, d, gout)
        assert float((f32 - f64).abs().max()) < 4e-7, name
        # the taps reproduce the lookup's own (sequential fp32) gradient scatter within the per-texel bound the GPU
        # test applies: (n + 2) 2^-24 sum |w g|
        off, w = c_oracle.cube_taps(d, v.R)
        ok = off.reshape(-1) >= 0
        pix = torch.arange(d.shape[0]).repeat_interleave(4)[ok]
        idx = off.reshape(-1)[ok].long()
        contrib = w.reshape(-1)[ok].double()[:, None] * gout[pix].double()
        ref = torch.zeros(6 * v.R * v.R, v.C, dtype=torch.float64).index_add_(0, idx, contrib)
        M = torch.zeros_like(ref).index_add_(0, idx, contrib.abs())
        n = torch.bincount(idx, minlength=6 * v.R * v.R).double()
        err = (v_tex.reshape(-1, v.C).double() - ref).abs()
        assert bool((err <= (n[:, None] + 2) * 2.0 ** -24 * M).all()), name
        assert float(n.max()) > 100, name


def test_sky_blend_f32_is_the_composite(c_oracle):
    g = torch.Generator().manual_seed(4)
    sky, rgb, a = torch.rand(500, 3, generator=g), torch.rand(500, 3, generator=g) * 1.5, torch.rand(500, generator=g)
    out = c_oracle.sky_blend_f32(sky, rgb, a)
    want = rgb.clamp(max=1) * a[:, None] + sky * (1 - a[:, None])
    assert float((out - want).abs().max()) < 3e-7

"""GPU: LiDAR seeding (csrc/seed.hip through sgn_rast.seed) against the float32 restatement of its contract
(tests/seed_oracle.py): every output — coordinates, colour bytes, source indices, offsets, totals — by bit equality, no
tolerance, on 1 / 63 / 65 / 4 099 / 20 000 points against 1 / 0 / 7 / 7 / 64 boxes and on a sweep whose every row is
dropped; a second run is bit-identical; the Python validation errors; SeedAccumulator over 3 sweeps x 2 cameras; and the
parameter tensors of init_gaussians."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import seed_oracle as SO
from sgn_rast import knn, seed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _scene(n, nb, s):
    sc = dict(SO.scene(n, nb, s))
    if n == 1:                                      # the single point is box 0's centre: live, visible, inside
        sc["points"] = sc["centers_lidar"][:1].copy()
    return sc


@functools.lru_cache(maxsize=None)
def _oracle(n, nb, s, img_seed=7):
    return SO.seed_sweep(_scene(n, nb, s), SO.image(img_seed))


def _cam(sc):
    return seed.SeedCamera(sc["w2c"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["width"], sc["height"])


def _run(sc, img):
    return seed.seed_sweep(torch.from_numpy(sc["points"]).cuda(), sc["l2w"], sc["boxes"], _cam(sc),
                           torch.from_numpy(img).cuda(), min_z=sc["min_z"])


def _assert_equal(got, exp):
    obj, bg = got
    assert obj.offsets == exp["offsets"]
    totals = [obj.offsets[b + 1] - obj.offsets[b] for b in range(len(obj.offsets) - 1)] + [bg.world.shape[0], bg.n_live]
    assert totals == exp["totals"]
    assert obj.local.dtype == torch.float32 and obj.rgb.dtype == torch.uint8 and obj.src.dtype == torch.int64
    assert bg.world.dtype == torch.float32 and bg.rgb.dtype == torch.uint8 and bg.src.dtype == torch.int64
    assert torch.equal(obj.src.cpu(), torch.from_numpy(exp["obj_src"]))
    assert torch.equal(bg.src.cpu(), torch.from_numpy(exp["bg_src"]))
    assert torch.equal(obj.rgb.cpu(), torch.from_numpy(exp["obj_rgb"]))
    assert torch.equal(bg.rgb.cpu(), torch.from_numpy(exp["bg_rgb"]))
    # bit equality of the coordinates (torch.equal on the float32 bit patterns: -0.0 and 0.0 are told apart)
    assert torch.equal(obj.local.cpu().view(torch.int32), torch.from_numpy(exp["local"]).view(torch.int32))
    assert torch.equal(bg.world.cpu().view(torch.int32), torch.from_numpy(exp["world"]).view(torch.int32))
    assert torch.equal(obj.local.cpu(), torch.from_numpy(exp["local"]))
    assert torch.equal(bg.world.cpu(), torch.from_numpy(exp["world"]))


@pytest.mark.parametrize("n,nb,s", SO.SCENES)
def test_every_output_equals_the_float32_oracle_bit_for_bit(n, nb, s):
    sc, exp = _scene(n, nb, s), _oracle(n, nb, s)
    if n == 1:
        assert exp["totals"] == [1, 0, 1]
    if n >= 4099:                                   # every destination is exercised, and the overlap of boxes 0 and 1
        assert all(t > 0 for t in exp["totals"]) and len(set(exp["obj_src"].tolist())) < exp["obj_src"].size
    got = _run(sc, SO.image(7))
    _assert_equal(got, exp)
    again = _run(sc, SO.image(7))
    for a, b in zip(got[0][:3] + got[1][:3], again[0][:3] + again[1][:3]):
        assert torch.equal(a, b)
    assert torch.equal(got[0].local.view(torch.int32), again[0].local.view(torch.int32))
    assert torch.equal(got[1].world.view(torch.int32), again[1].world.view(torch.int32))
    assert got[0].offsets == again[0].offsets and got[1].n_live == again[1].n_live


@pytest.mark.parametrize("why", ["nan", "below_min_z", "behind_camera"])
def test_a_sweep_whose_every_row_is_dropped_gives_empty_outputs(why):
    sc = dict(_scene(4099, 7, 14))
    pts = sc["points"].copy()
    if why == "nan":
        pts[:, 1] = np.nan
    elif why == "below_min_z":
        pts[:, 2] = -2.0                            # z == min_z is dropped: the test is strict
    else:
        pts[:, 0] = -np.abs(pts[:, 0]) - 1.0        # live, but behind the camera
    sc["points"] = pts
    exp = SO.seed_sweep(sc, SO.image(7))
    assert exp["offsets"] == [0] * 8 and exp["totals"][:8] == [0] * 8
    assert (exp["totals"][8] > 0) == (why == "behind_camera")
    obj, bg = _run(sc, SO.image(7))
    _assert_equal((obj, bg), exp)
    assert obj.local.shape == (0, 3) and obj.rgb.shape == (0, 3) and obj.src.shape == (0,) and bg.world.shape == (0, 3)


def test_validation_errors():
    sc = _scene(65, 7, 13)
    pts, img, cam = torch.from_numpy(sc["points"]).cuda(), torch.from_numpy(SO.image(7)).cuda(), _cam(sc)
    ok = lambda **kw: seed.seed_sweep(**{**dict(points=pts, l2w=sc["l2w"], boxes=sc["boxes"], cam=cam, image=img), **kw})
    ok()
    bad = [dict(points=pts.double()), dict(points=pts[:, :2]), dict(points=pts.reshape(-1)), dict(points=pts[:0]),
           dict(points=pts.cpu()), dict(points=sc["points"]), dict(image=img.cpu()), dict(image=img.float()),
           dict(image=img[:, :, :2]), dict(image=img[:-1]), dict(image=img.transpose(0, 1)),
           dict(image=torch.from_numpy(SO.image(7, 96, 320)).cuda()[:, ::2]),          # right shape, not contiguous
           dict(boxes=np.zeros((65, 15), np.float32)), dict(boxes=np.zeros((3, 14), np.float32)),
           dict(l2w=np.eye(3)), dict(cam=dict(width=160)),
           dict(cam=seed.SeedCamera(sc["w2c"], 120.0, 120.0, 79.3, 47.6, 0, 96), image=img[:, :0])]
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
    none = ok(boxes=None)[0]
    assert none.offsets == [0] and none.local.shape == (0, 3)


def test_accumulator_over_three_sweeps_and_two_cameras():
    acc = seed.SeedAccumulator()
    tracks = ["car_a", "car_b", 17, "car_d", "car_e"]
    exp_obj = {t: ([], []) for t in tracks}
    exp_bg = ([], [])
    for call, (n, nb, s) in enumerate(SO.ACC_SCENES):           # call = sweep * 2 + camera
        sc, img = _scene(n, nb, s), SO.image(20 + call % 2)
        exp = SO.seed_sweep(sc, img)
        ids = tracks if call % 3 else tracks[::-1]              # box order differs between calls: ids, not positions
        obj, bg = _run(sc, img)
        acc.add(ids, obj, bg)
        for b, t in enumerate(ids):
            lo, hi = exp["offsets"][b], exp["offsets"][b + 1]
            exp_obj[t][0].append(exp["local"][lo:hi]); exp_obj[t][1].append(exp["obj_rgb"][lo:hi])
        exp_bg[0].append(exp["world"]); exp_bg[1].append(exp["bg_rgb"])
    as_loaded = lambda u8: (np.concatenate(u8).astype(np.float64) / 255.0).astype(np.float32) * np.float32(255.0)
    sizes = sorted(sum(p.shape[0] for p in exp_obj[t][0]) for t in tracks)
    min_points = sizes[2]                                       # two tracks fall below, three stay
    assert sizes[1] < min_points
    objects, background = acc.finish(scale_factor=0.25, min_points=min_points)
    assert list(objects) == tracks[::-1]                        # first-seen order
    for t in tracks:
        xyz = np.concatenate(exp_obj[t][0])
        if xyz.shape[0] < min_points:
            assert objects[t] is None
            continue
        got_xyz, got_rgb = objects[t]
        assert got_xyz.dtype == torch.float32 and got_rgb.dtype == torch.float32
        assert torch.equal(got_xyz.cpu(), torch.from_numpy(xyz * np.float32(0.25)))
        assert torch.equal(got_rgb.cpu(), torch.from_numpy(as_loaded(exp_obj[t][1])))
    assert torch.equal(background[0].cpu(), torch.from_numpy(np.concatenate(exp_bg[0])))
    assert torch.equal(background[1].cpu(), torch.from_numpy(as_loaded(exp_bg[1])))
    # the reference's default: fewer than 10 000 points is no seed
    assert all(v is None for v in acc.finish()[0].values())
    with pytest.raises(ValueError):
        acc.add(tracks[:3], *_run(_scene(*SO.ACC_SCENES[0]), SO.image(20)))


def _rgb_fixture():
    """Rows of tests/golden/known_rgb2sh.npz whose rgb has a float32 `rgb255` with rgb255 / 255 == rgb exactly (the
    named rows and all but a few of the random ones), so that init_gaussians is asked for exactly the fixture's input."""
    g = np.load(os.path.join(HERE, "golden", "known_rgb2sh.npz"))
    rgb, want = g["rgb"], g["RGB2SH_of_rgb"]
    x = rgb * np.float32(255.0)
    pre = np.full_like(rgb, np.nan)
    for cand in (x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
        pre = np.where(np.isnan(pre) & (cand / np.float32(255.0) == rgb), cand, pre)
    rows = ~np.isnan(pre).any(axis=1)
    assert rows[:7].all() and rows.sum() > 2048
    return pre[rows], want[rows]


def test_init_gaussians():
    rgb255, want_dc = _rgb_fixture()
    n = rgb255.shape[0]
    xyz = (torch.rand(n, 3, generator=torch.Generator().manual_seed(5)) * 20.0).cuda()
    p = seed.init_gaussians(xyz, torch.from_numpy(rgb255).cuda(), sh_degree=3, fourier_features_dim=4,
                            generator=torch.Generator().manual_seed(9))
    assert set(p) == {"means", "scales", "quats", "features_dc", "features_rest", "opacities"}
    assert all(v.is_cuda and v.dtype == torch.float32 for v in p.values())
    assert torch.equal(p["means"], xyz)
    assert p["scales"].shape == (n, 3) and torch.equal(p["scales"], knn.init_log_scales(xyz))
    assert p["features_dc"].shape == (n, 4, 3) and p["features_rest"].shape == (n, 15, 3)
    assert torch.equal(p["features_dc"][:, 0].cpu(), torch.from_numpy(want_dc))
    assert not p["features_dc"][:, 1:].any() and not p["features_rest"].any()
    assert p["opacities"].shape == (n, 1)
    assert torch.equal(p["opacities"].cpu(), torch.logit(0.1 * torch.ones(n, 1)))
    assert abs(float(p["opacities"][0]) - math.log(0.1 / 0.9)) < 1e-6
    assert p["quats"].shape == (n, 4) and float((p["quats"].norm(dim=-1) - 1).abs().max()) < 1e-6
    q2 = seed.init_gaussians(xyz, torch.from_numpy(rgb255).cuda(), generator=torch.Generator().manual_seed(9))["quats"]
    assert torch.equal(p["quats"], q2)
    q3 = seed.init_gaussians(xyz, torch.from_numpy(rgb255).cuda(), generator=torch.Generator().manual_seed(10))["quats"]
    assert not torch.equal(p["quats"], q3)
    # the reference's formula on the same draws
    g = torch.Generator().manual_seed(9)
    u, v, w = torch.rand(n, generator=g), torch.rand(n, generator=g), torch.rand(n, generator=g)
    ref = torch.stack([torch.sqrt(1 - u) * torch.sin(2 * math.pi * v), torch.sqrt(1 - u) * torch.cos(2 * math.pi * v),
                       torch.sqrt(u) * torch.sin(2 * math.pi * w), torch.sqrt(u) * torch.cos(2 * math.pi * w)], dim=-1)
    assert torch.equal(p["quats"].cpu(), ref)
    # sh_degree 0: colours through the logit, no higher bands
    # (random rows only: a colour of exactly 1 has logit = inf in float32).  Both sides evaluate the same formula on the
    # same float32 input and may differ by the rounding of one division and one log: a few ulp of the largest value
    p0 = seed.init_gaussians(xyz[8:72], torch.from_numpy(rgb255[8:72]).cuda(), sh_degree=0)
    assert p0["features_rest"].shape == (64, 0, 3) and p0["features_dc"].shape == (64, 1, 3)
    want0 = torch.logit(torch.from_numpy(rgb255[8:72]) / 255, eps=1e-10)
    assert bool(torch.isfinite(want0).all())
    assert float((p0["features_dc"][:, 0].cpu() - want0).abs().max()) <= 4 * 2.0 ** -23 * max(float(want0.abs().max()), 1.0)

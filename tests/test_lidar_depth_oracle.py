"""CPU: the numpy restatement of the LiDAR depth contract (tests/lidar_depth_oracle.py) against plainer statements of the
same thing — a Python loop over points, a brute-force window loop, central differences — and the conditions the GPU
tests' tolerances rest on, checked on the GPU tests' own inputs with the float64 oracle alone."""
import numpy as np
import pytest

import lidar_depth_oracle as LO
import seed_oracle as SO

F32 = np.float32


def test_the_splat_oracle_equals_a_python_loop_over_points():
    sc, _ = LO.splat_scene(5000)
    assert (sc["width"], sc["height"]) == (160, 96)
    counted, u, v, z, _ = LO.counted_points(sc, LO.MAX_DEPTH)
    exp = np.full((96, 160), np.inf, dtype=F32)
    for i in range(sc["points"].shape[0]):
        if counted[i] and z[i] < exp[v[i], u[i]]:
            exp[v[i], u[i]] = z[i]
    got = LO.splat(sc, LO.begin(96, 160), LO.MAX_DEPTH)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    # positive floats order as their bit patterns: the integer minimum of the kernel is this minimum
    bits = np.full((96, 160), 0x7f800000, dtype=np.uint32)
    np.minimum.at(bits, (v[counted], u[counted]), z[counted].view(np.uint32))
    assert np.array_equal(bits, exp.view(np.uint32))


@pytest.mark.parametrize("shape,radius", [((37, 53), 0), ((37, 53), 1), ((37, 53), 3), ((37, 53), 8), ((16, 16), 2),
                                          ((5, 3), 8)])
def test_the_filter_oracle_equals_a_brute_force_window_loop(shape, radius):
    rng = np.random.default_rng(3)
    H, W = shape
    d = np.where(rng.random(shape) < 0.4, rng.uniform(2.0, 60.0, shape), np.inf).astype(F32)
    d[rng.random(shape) < 0.1] = F32(2.5)              # a foreground that occludes what lies behind it
    rel_tol = 0.05
    keep = F32(1) - F32(rel_tol)
    exp = np.zeros(shape, F32)
    for y in range(H):
        for x in range(W):
            if not np.isfinite(d[y, x]):
                continue
            m = min(d[yy, xx] for yy in range(max(0, y - radius), min(H, y + radius + 1))
                    for xx in range(max(0, x - radius), min(W, x + radius + 1)))
            if F32(d[y, x] * keep) <= m:
                exp[y, x] = d[y, x]
    got = LO.filter_returns(d, radius, rel_tol)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    if radius == 0:
        assert np.array_equal(got, np.where(np.isfinite(d), d, 0))      # radius 0 keeps every return
    else:
        assert 0 < (got > 0).sum() < np.isfinite(d).sum()                # the filter drops some, not all
    assert not LO.filter_returns(np.full(shape, np.inf, F32), radius, rel_tol).any()    # no return at all


@pytest.mark.parametrize("kind", ["l1", "inverse"])
def test_the_float64_gradient_equals_central_differences(kind):
    d = LO.loss_inputs(37, 53)
    o = LO.loss64(d["dsum"], d["alpha"], d["target"], d["mask"], kind)
    rows = np.argwhere(o["counted"] & ~d["equal"])[[0, 7, 100, 250, -1]]
    f = lambda s, a: LO.loss64(s, a, d["target"], d["mask"], kind)["loss"]
    for y, x in rows:
        for name, grad in (("dsum", o["v_dsum"]), ("alpha", o["v_alpha"])):
            # float32-representable steps (loss64 reads float32 inputs), small against the residual |r| >= 1e-3
            lo, hi = d[name].copy(), d[name].copy()
            lo[y, x] = lo[y, x] * F32(1 - 2.0 ** -13)
            hi[y, x] = hi[y, x] * F32(1 + 2.0 ** -13)
            args = (lambda t: (t, d["alpha"])) if name == "dsum" else (lambda t: (d["dsum"], t))
            num = (f(*args(hi)) - f(*args(lo))) / (float(hi[y, x]) - float(lo[y, x]))
            assert abs(num - grad[y, x]) <= 1e-6 * abs(grad[y, x]), (kind, name, y, x, num, grad[y, x])


def test_the_float32_restatement_of_the_loss_is_within_the_gpu_bound_of_float64():
    d = LO.loss_inputs(37, 53)
    for kind in LO.KINDS:
        for mask in (None, d["mask"]):
            o = LO.loss64(d["dsum"], d["alpha"], d["target"], mask, kind)
            l32, n = LO.loss32(d["dsum"], d["alpha"], d["target"], mask, kind)
            scale = o["D"][o["counted"]] if kind == "l1" else 1.0 / o["D"][o["counted"]]
            assert n == o["count"] and abs(float(l32) - o["loss"]) <= 2.0 ** -22 * scale.mean()


def test_the_gpu_loss_inputs_keep_their_conditions():
    d = LO.loss_inputs(37, 53)
    s, a, z, eq = d["dsum"], d["alpha"], d["target"], d["equal"]
    assert s.size == 1961 and s.size % 64 and s.size % 256 and s.size > 256         # a partial wave, a partial block
    assert all(t.dtype == F32 for t in (s, a, z)) and d["mask"].dtype == np.uint8
    band = a <= LO.ALPHA_MIN
    assert band.sum() > 20 and (a == LO.ALPHA_MIN).any() and a[~band].min() >= 0.05 and a.max() <= 1
    assert abs((z == 0).mean() - 1 / 3) < 0.05 and z[z > 0].min() >= 1 and z.max() <= 80
    assert (s <= 0).sum() > 5 and 0 < (d["mask"] == 0).mean() < 0.5
    for kind in LO.KINDS:
        for mask in (None, d["mask"]):
            o = LO.loss64(s, a, z, mask, kind)
            c = o["counted"]
            assert 300 < o["count"] < s.size and not (c & band).any() and not (c & (z == 0)).any()
            r = o["D"][c & ~eq] / z[c & ~eq].astype(np.float64) - 1.0
            assert np.abs(r).min() >= 1e-3 * (1 - 1e-6) and np.abs(r).max() <= 0.4 * (1 + 1e-6)
            assert not ((np.abs(r - 0.25) < 1e-3) | (np.abs(r + 0.2) < 1e-3)).any()   # clear of the delta1 thresholds
            assert 0.5 < o["metrics"]["delta1"] < 1.0
            # the exact-equality pixels: counted ones exist, their residual and gradient are exactly zero
            assert (c & eq).sum() >= 10 and set(a[eq].tolist()) == {0.5, 0.25}
            assert not o["residual"][c & eq].any() and not o["v_dsum"][c & eq].any() and not o["v_alpha"][c & eq].any()
            assert np.array_equal((s[eq] / a[eq]).astype(F32), z[eq])                    # exactly, in float32 too
            # sign-ambiguous pixels: the cap is 1 %, the construction gives none
            amb = LO.sign_ambiguous(o, z)
            assert amb.sum() == 0 and amb.mean() <= 0.01
            assert o["v_dsum"][c & ~eq].all() and not o["v_dsum"][~c].any() and not o["v_alpha"][~c].any()
    one = LO.loss_inputs(1, 1)
    assert LO.loss64(one["dsum"], one["alpha"], one["target"], one["mask"])["count"] == 1
    u = LO.uncounted_inputs()
    o = LO.loss64(u["dsum"], u["alpha"], u["target"], None)
    assert o["count"] == 0 and o["loss"] == 0.0 and not o["v_dsum"].any() and o["metrics"]["rmse"] == 0.0


def test_the_gpu_splat_scenes_keep_their_conditions():
    for n in LO.SPLAT_SIZES:
        sc, planted = LO.splat_scene(n)
        assert sc["points"].shape == (n, 3) and sc["points"].dtype == F32
        counted, u, v, z, c = LO.counted_points(sc, LO.MAX_DEPTH)
        if n == 1:
            assert counted.all()
            continue
        fu = c["fu"][planted["fu_neg"]]
        assert ((fu > -1) & (fu < 0)).all() and counted[planted["fu_neg"]].all() and not u[planted["fu_neg"]].any()
        a, b = planted["twin"]
        assert counted[a] and counted[b] and z[a] == z[b] and (u[a], v[a]) == (u[b], v[b])
    pts = sc["points"]
    with np.errstate(invalid="ignore"):
        assert np.isnan(pts).any(axis=1).sum() > 20 and (pts[:, 2] <= sc["min_z"]).sum() > 50
        assert (c["ok"] & ~counted).sum() > 50                         # live and visible, but past MAX_DEPTH
        assert (c["live"] & ~(c["pcz"] > 0)).sum() > 50                # behind the camera
    hits = np.zeros((sc["height"], sc["width"]), int)
    np.add.at(hits, (v[counted], u[counted]), 1)
    assert (hits[hits > 0] > 1).mean() > 0.05 and hits.max() >= 3      # pixels that receive several returns
    # two sweeps in turn equal their concatenation
    half = dict(sc, points=pts[:2500]), dict(sc, points=pts[2500:])
    both = LO.splat(half[1], LO.splat(half[0], LO.begin(96, 160), LO.MAX_DEPTH), LO.MAX_DEPTH)
    assert np.array_equal(both, LO.splat(sc, LO.begin(96, 160), LO.MAX_DEPTH))
    full = LO.splat_depth([sc], 2, 0.05, LO.MAX_DEPTH)
    assert 0 < (full > 0).sum() < np.isfinite(both).sum()

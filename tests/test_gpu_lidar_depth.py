"""GPU (-m gpu): LiDAR depth supervision (csrc/lidar_depth.hip through sgn_rast.lidar and step.train_step) against
tests/lidar_depth_oracle.py.

Target: the splat and the occlusion filter BIT FOR BIT against the float32 oracle, no tolerance.

Loss, gradient, metrics against the float64 oracle, every bound derived (tests/test_lidar_depth_oracle.py holds the
inputs to the conditions used here):
* per-pixel v_dsum / v_alpha: relative 1e-6 — at most six fp32 roundings of 2^-24 each lie between inputs and output
  (the quotient D, D * D, g, two divisions, the product with D) and nothing cancels: only the SIGN of the residual
  enters.  Sign-ambiguous pixels (0 < |D64 - z| <= 2^-22 z) may be left out, at most 1 % of the counted ones; the inputs
  have none.  Uncounted pixels and the exact-equality pixels: exact zeros.
* loss, l1: |loss - loss64| <= 2^-22 mean(D over counted) — the division's rounding (2^-24 D), the subtraction's
  (2^-24 |D - z| <= 2^-24 D) and the fp32 mean's (2^-24 loss) stay below 4 * 2^-24 of the mean D; inverse: the same with
  1 / D (two roundings for 1 / D, one for 1 / z <= 1.4 / D, one for the difference).
* metrics: the same per-term bound — mae as l1; abs_rel with D / z for D; rmse: the term e^2 carries 2 e de + 2^-24 e^2
  with de <= 2^-24 (D + e), so the root moves by at most 2^-24 max(D + e) + 2^-24 rmse < 2^-22 max(D); delta1: the
  inputs keep clear of its thresholds, so only the rounding of the share, 2^-23; count exact.

End to end: train_step(lidar_depth=) against the same step with the depth term written as the eager torch chain over
features.expected_depth, parameter gradients rel-L2 <= 1e-4 per tensor (the project's gradient tolerance)."""
import functools

import numpy as np
import pytest
import torch

import lidar_depth_oracle as LO
from helpers import rel_l2
from sgn_rast import _lib as L
from sgn_rast import features, lidar, seed

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _cam(sc):
    return seed.SeedCamera(sc["w2c"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["width"], sc["height"])


def _sweep(sc, rows=slice(None)):
    return torch.from_numpy(np.ascontiguousarray(sc["points"][rows])).to(DEV), sc["l2w"]


@functools.lru_cache(maxsize=None)
def _target_oracle(n, radius):
    return LO.splat_depth([LO.splat_scene(n)[0]], radius, 0.05, LO.MAX_DEPTH)


# ---------------------------------------------------------------- target

@pytest.mark.parametrize("n", LO.SPLAT_SIZES)
def test_splat_equals_the_float32_oracle_bit_for_bit(n):
    sc, _ = LO.splat_scene(n)
    for radius in (0, 2):
        exp = _target_oracle(n, radius)
        got = lidar.splat_depth(_sweep(sc), _cam(sc), min_z=sc["min_z"], max_depth=LO.MAX_DEPTH, radius=radius)
        assert got.dtype == torch.float32 and tuple(got.shape) == (sc["height"], sc["width"])
        assert (exp > 0).sum() >= 1
        assert np.array_equal(_bits(got), _bits(exp)), int((_bits(got) != _bits(exp)).sum())
        again = lidar.splat_depth([_sweep(sc)], _cam(sc), min_z=sc["min_z"], max_depth=LO.MAX_DEPTH, radius=radius)
        assert np.array_equal(_bits(got), _bits(again))                 # run to run
    if n > 1:       # without max_depth the far returns land too
        far = lidar.splat_depth(_sweep(sc), _cam(sc), min_z=sc["min_z"], radius=0)
        assert np.array_equal(_bits(far), _bits(LO.splat_depth([sc], 0, 0.05)))
        assert (far > LO.MAX_DEPTH).any()


def test_two_sweeps_in_turn_equal_their_concatenation():
    sc, _ = LO.splat_scene(5000)
    for radius in (0, 2):
        whole = lidar.splat_depth(_sweep(sc), _cam(sc), sc["min_z"], LO.MAX_DEPTH, radius)
        parts = lidar.splat_depth([_sweep(sc, slice(0, 1777)), _sweep(sc, slice(1777, None))], _cam(sc), sc["min_z"],
                                  LO.MAX_DEPTH, radius)
        swapped = lidar.splat_depth([_sweep(sc, slice(1777, None)), _sweep(sc, slice(0, 1777))], _cam(sc), sc["min_z"],
                                    LO.MAX_DEPTH, radius)
        assert np.array_equal(_bits(whole), _bits(parts)) and np.array_equal(_bits(whole), _bits(swapped))
        assert np.array_equal(_bits(whole), _bits(_target_oracle(5000, radius)))


def test_a_sweep_without_a_counted_point_gives_an_all_zero_target():
    sc = dict(LO.splat_scene(257)[0])
    pts = sc["points"].copy()
    pts[:, 0] = -np.abs(pts[:, 0]) - 1.0                # live, but behind the camera
    pts[::3, 1] = np.nan
    sc["points"] = pts
    got = lidar.splat_depth(_sweep(sc), _cam(sc), min_z=sc["min_z"])
    assert not LO.splat_depth([sc]).any() and not got.any().item()


def _finish(depth_np, radius, rel_tol=0.05):
    d = torch.from_numpy(depth_np).to(DEV)
    out = torch.full_like(d, -1.0)
    H, W = depth_np.shape
    L.check(L.load().sgn_lidar_depth_finish(L.ptr(d), H, W, radius, rel_tol, L.ptr(out), L.stream_ptr()),
            "sgn_lidar_depth_finish")
    return out


def _returns(shape, seed_=3):
    rng = np.random.default_rng(seed_)
    d = np.where(rng.random(shape) < 0.4, rng.uniform(2.0, 60.0, shape), np.inf).astype(np.float32)
    d[rng.random(shape) < 0.1] = np.float32(2.5)
    return d


@pytest.mark.parametrize("shape,radius", [((37, 53), 0), ((37, 53), 1), ((37, 53), 3), ((37, 53), 8), ((16, 16), 2),
                                          ((16, 16), 8), ((5, 3), 8), ((33, 17), 5)])
def test_filter_equals_the_float32_oracle_bit_for_bit(shape, radius):
    d = _returns(shape)
    exp = LO.filter_returns(d, radius, 0.05)
    got = _finish(d, radius)
    assert np.array_equal(_bits(got), _bits(exp)), int((_bits(got) != _bits(exp)).sum())
    if radius:
        assert 0 < (exp > 0).sum() < np.isfinite(d).sum()
    # another tolerance, and a tolerance of 0: only the window's minima survive
    for tol in (0.3, 0.0):
        assert np.array_equal(_bits(_finish(d, radius, tol)), _bits(LO.filter_returns(d, radius, tol)))


def test_filter_of_an_image_without_a_return_is_all_zero():
    for shape, radius in (((37, 53), 3), ((5, 3), 8), ((16, 16), 0)):
        got = _finish(np.full(shape, np.inf, np.float32), radius)
        assert not got.any().item() and np.array_equal(_bits(got), np.zeros(shape, np.uint32))


# ---------------------------------------------------------------- loss, gradient, metrics

V_LOSS = 0.37


def _dev(d, with_mask):
    t = {k: torch.from_numpy(d[k]).to(DEV) for k in ("dsum", "alpha", "target")}
    return t, (torch.from_numpy(d["mask"]).to(DEV) if with_mask else None)


def _run_loss(d, kind, with_mask):
    t, mask = _dev(d, with_mask)
    dsum, alpha = t["dsum"].clone().requires_grad_(True), t["alpha"].clone().requires_grad_(True)
    target = t["target"].clone().requires_grad_(True)          # gradients go to dsum and alpha only
    loss = lidar.depth_loss(dsum, alpha, target, kind, mask)
    (loss * V_LOSS).backward()
    assert target.grad is None and loss.dim() == 0 and loss.dtype == torch.float32
    return float(loss.detach()), dsum.grad.cpu().numpy(), alpha.grad.cpu().numpy()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("kind", ["l1", "inverse"])
@pytest.mark.parametrize("shape", LO.LOSS_SHAPES)
def test_loss_and_gradient_against_float64(shape, kind, with_mask):
    d = LO.loss_inputs(*shape)
    mask_np = d["mask"] if with_mask else None
    o = LO.loss64(d["dsum"], d["alpha"], d["target"], mask_np, kind, v_loss=float(np.float32(V_LOSS)))
    c = o["counted"]
    loss, v_dsum, v_alpha = _run_loss(d, kind, with_mask)
    Dc = o["D"][c]
    bound = 2.0 ** -22 * float((Dc if kind == "l1" else 1.0 / Dc).mean())
    amb = LO.sign_ambiguous(o, d["target"])
    chk = c & ~amb
    rel = lambda got, exp: float((np.abs(got[chk] - exp[chk]) / np.maximum(np.abs(exp[chk]), 1e-300)).max())
    print(f"[depth loss] {shape} {kind} mask={with_mask}: count {o['count']}  loss {loss:.9g} vs {o['loss']:.9g} "
          f"(err {abs(loss - o['loss']):.2e}, bound {bound:.2e})  ambiguous {int(amb.sum())}  "
          f"v_dsum rel {rel(v_dsum, o['v_dsum']):.2e}  v_alpha rel {rel(v_alpha, o['v_alpha']):.2e}")
    assert o["count"] >= 1 and amb.sum() <= 0.01 * o["count"]
    assert abs(loss - o["loss"]) <= bound
    assert (np.abs(v_dsum[chk] - o["v_dsum"][chk]) <= 1e-6 * np.abs(o["v_dsum"][chk])).all()
    assert (np.abs(v_alpha[chk] - o["v_alpha"][chk]) <= 1e-6 * np.abs(o["v_alpha"][chk])).all()
    # exact zeros: uncounted pixels, and the counted pixels where D == z exactly (a zero bound above already says so)
    assert not v_dsum[~c].any() and not v_alpha[~c].any()
    assert not v_dsum[c & d["equal"]].any() and not v_alpha[c & d["equal"]].any()
    if shape != (1, 1):
        assert (c & d["equal"]).sum() >= 10 and v_dsum[c & ~d["equal"]].all()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("shape", LO.LOSS_SHAPES)
def test_metrics_against_float64(shape, with_mask):
    d = LO.loss_inputs(*shape)
    o = LO.loss64(d["dsum"], d["alpha"], d["target"], d["mask"] if with_mask else None)
    t, mask = _dev(d, with_mask)
    got = lidar.depth_metrics(t["dsum"], t["alpha"], t["target"], mask)
    exp, c = o["metrics"], o["counted"]
    D, z = o["D"][c], d["target"][c].astype(np.float64)
    bounds = {"mae": 2.0 ** -22 * D.mean(), "abs_rel": 2.0 ** -22 * (D / z).mean(), "rmse": 2.0 ** -22 * D.max(),
              "delta1": 2.0 ** -23}
    print(f"[depth metrics] {shape} mask={with_mask}: " + "  ".join(
        f"{k} {got[k]:.9g} vs {exp[k]:.9g} (err {abs(got[k] - exp[k]):.2e}, bound {b:.2e})" for k, b in bounds.items())
        + f"  count {got['count']} vs {exp['count']}")
    assert got["count"] == exp["count"] and isinstance(got["count"], int) and set(got) == set(exp)
    for k, b in bounds.items():
        assert abs(got[k] - exp[k]) <= b, k
    # [H,W,1] inputs are the same image
    assert lidar.depth_metrics(t["dsum"][..., None], t["alpha"], t["target"][..., None], mask)["count"] == exp["count"]


@pytest.mark.parametrize("kind", ["l1", "inverse"])
def test_an_image_without_a_counted_pixel_gives_zero_loss_and_zero_gradients(kind):
    d = LO.uncounted_inputs()
    for with_mask in (False, True):
        loss, v_dsum, v_alpha = _run_loss(d, kind, with_mask)
        assert loss == 0.0 and not v_dsum.any() and not v_alpha.any()          # zeros, not NaN
        t, mask = _dev(d, with_mask)
        assert lidar.depth_metrics(t["dsum"], t["alpha"], t["target"], mask) == \
            {"abs_rel": 0.0, "rmse": 0.0, "mae": 0.0, "delta1": 0.0, "count": 0}
    # a mask of zeros uncounts every pixel of an image that has counted ones
    full = LO.loss_inputs(37, 53)
    t, _ = _dev(full, False)
    zero = torch.zeros(37, 53, dtype=torch.bool, device=DEV)
    dsum = t["dsum"].clone().requires_grad_(True)
    loss = lidar.depth_loss(dsum, t["alpha"], t["target"], kind, zero)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not dsum.grad.any().item()


def test_nan_and_inf_inputs_are_uncounted():
    d = {k: v.copy() for k, v in LO.loss_inputs(37, 53).items()}
    ref = LO.loss64(d["dsum"], d["alpha"], d["target"], None)
    rows = np.argwhere(ref["counted"] & ~d["equal"])[:3]
    d["dsum"][tuple(rows[0])] = np.nan
    d["alpha"][tuple(rows[1])] = np.nan
    d["target"][tuple(rows[2])] = np.nan
    o = LO.loss64(d["dsum"], d["alpha"], d["target"], None)
    loss, v_dsum, v_alpha = _run_loss(d, "l1", False)
    assert o["count"] == ref["count"] - 3
    assert abs(loss - o["loss"]) <= 2.0 ** -22 * o["D"][o["counted"]].mean()
    assert np.isfinite(v_dsum).all() and np.isfinite(v_alpha).all()
    for r in rows:
        assert v_dsum[tuple(r)] == 0 and v_alpha[tuple(r)] == 0


# ---------------------------------------------------------------- end to end

def _e2e_scene():
    from sgn_rast import scenes
    cam, raw = scenes.make_scene("c1", seed=2, n_override=500, device=DEV)
    gt = torch.rand(cam.height, cam.width, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    # points on the scene's own surfaces — the Gaussians' centres — pushed 5 % deeper along their rays, world frame
    pos = cam.cam_pos.to(DEV)
    pts = (pos + 1.05 * (raw["means"] - pos)).to(torch.float32).contiguous()
    sc = seed.SeedCamera(cam.viewmat.cpu(), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    target = lidar.splat_depth((pts, torch.eye(4)), sc, min_z=-1e30)
    return cam, raw, gt, target


def _eager_term(dsum, acc, z, kind, dtype=torch.float32):
    dsum, acc, z = dsum.to(dtype), acc.to(dtype), z.to(dtype)
    valid = (z > 0) & (acc > 1e-3) & (dsum > 0)
    D, zc = dsum[valid] / acc[valid], z[valid]
    return ((D - zc) if kind == "l1" else (1 / D - 1 / zc)).abs().mean(), D


@pytest.mark.parametrize("kind", ["l1", "inverse"])
@pytest.mark.parametrize("fused", [False, True])
def test_train_step_with_lidar_depth_matches_the_eager_chain(fused, kind):
    from sgn_rast import ops, step
    from sgn_rast.loss import photometric_loss
    cam, raw, gt, target = _e2e_scene()
    assert (cam.height, cam.width) == (128, 128) and int((target > 0).sum()) > 100
    w_img, w_a = (t.to(DEV) for t in step.loss_weights(cam, seed=7))
    mult = 0.1
    P = step.leaf_params(raw)
    ops.clear_binning_cache()
    b0 = ops.binning_stats["binnings"]
    got = step.train_step(P, cam, w_img, w_a, gt=gt, fused=fused, lidar_depth=target, depth_loss_mult=mult,
                          depth_loss_kind=kind)
    assert ops.binning_stats["binnings"] == b0 + 1          # the depth pass walks the RGB pass's list
    Pe = step.leaf_params(raw)
    out = step.render_fused(Pe, cam) if fused else step.render(Pe, cam, caller_syncs=False)
    opac = Pe["opacity_logits"] if fused else out.opacities
    dsum, acc = features.expected_depth(out.xys, out.depths, out.radii, out.conics, out.num_tiles_hit, opac, cam.height,
                                        cam.width, 16, opacity_is_logit=fused)
    term, _ = _eager_term(dsum, acc, target, kind)
    loss = photometric_loss(out.rgb, gt, 0.2, clamp_max=1.0) + (out.alpha * w_a).sum() / (cam.height * cam.width)
    (loss + mult * term).backward()
    term64, D64 = _eager_term(dsum.detach(), acc.detach(), target, kind, torch.float64)
    bound = 2.0 ** -22 * float((D64 if kind == "l1" else 1 / D64).mean())
    rels = {k: rel_l2(P[k].grad, Pe[k].grad) for k in P}
    print(f"[depth step] fused={fused} {kind}: counted {D64.numel()}  depth_loss {float(got.depth_loss):.9g} vs "
          f"{float(term64):.9g} (err {abs(float(got.depth_loss) - float(term64)):.2e}, bound {bound:.2e})  "
          + "  ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    assert D64.numel() > 100 and float(term64) > 0
    assert got.depth_loss.dim() == 0 and not got.depth_loss.requires_grad
    assert abs(float(got.depth_loss) - float(term64)) <= bound
    assert abs(float(got.loss) - float((loss + mult * term).detach())) <= 1e-6 * max(1.0, abs(float(got.loss)))
    for k, v in rels.items():
        assert v <= 1e-4, k
    # the term reached the parameters: without it the means' gradient differs
    Pn = step.leaf_params(raw)
    step.train_step(Pn, cam, w_img, w_a, gt=gt, fused=fused)
    assert rel_l2(Pn["means"].grad, P["means"].grad) > 1e-3


@pytest.mark.parametrize("fused", [False, True])
def test_lidar_depth_none_is_the_step_without_the_keyword(fused):
    from sgn_rast import step
    cam, raw, gt, _ = _e2e_scene()
    w_img, w_a = (t.to(DEV) for t in step.loss_weights(cam, seed=7))
    a = step.train_step(step.leaf_params(raw), cam, w_img, w_a, gt=gt, fused=fused)
    b = step.train_step(step.leaf_params(raw), cam, w_img, w_a, gt=gt, fused=fused, lidar_depth=None)
    assert torch.equal(a.rgb, b.rgb) and torch.equal(a.alpha, b.alpha) and torch.equal(a.loss, b.loss)
    assert not hasattr(b, "depth_loss")


def test_train_step_refuses_a_wrong_target_before_anything_is_launched():
    from sgn_rast import step
    cam, raw, gt, target = _e2e_scene()
    w_img, w_a = (t.to(DEV) for t in step.loss_weights(cam, seed=7))
    P = step.leaf_params(raw)
    for bad in (target[:-1], target.double(), target[None]):
        with pytest.raises(ValueError, match="lidar_depth"):
            step.train_step(P, cam, w_img, w_a, gt=gt, lidar_depth=bad)
    with pytest.raises(ValueError, match="depth_loss_kind"):
        step.train_step(P, cam, w_img, w_a, gt=gt, lidar_depth=target, depth_loss_kind="huber")
    assert all(p.grad is None for p in P.values())

"""GPU (-m gpu): rolling-shutter rendering (`sgn_rast.shutter`, csrc/rolling_shutter.hip) — the kernel pair per element
against float64, zero motion as the identity, the compensated render against the time-sliced truth, and the pass
through every layer that takes `rolling_shutter=` against the oracle composition (tests/rolling_shutter_oracle.py)."""
import pytest
import torch

import rolling_shutter_oracle as RO
from helpers import rel_l2
from test_rolling_shutter_oracle import MARGIN_GAIN_DB, MOTION_GAIN_DB

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 255, 256, 257, 1000]


def _dev_cam(cam):
    from sgn_rast import scenes
    return scenes.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat.to(DEV), cam.cam_pos.to(DEV))


def _to_dev(raw):
    return {k: v.to(DEV) for k, v in raw.items()}


# ---------------------------------------------------------------- 1. the kernel pair

_PROJ = {}


def _projection():
    """The projection's outputs of the 64x48 scene on the CPU oracle, float32 (computed once)."""
    if not _PROJ:
        from oracle import torch_oracle as O
        cam, raw = RO.scene()
        means, scales, quats, _ = RO._activated(raw)
        xys, depths, radii, conics, _, nth, _ = O.project_gaussians(means, scales, 1, quats, cam.viewmat[:3], cam.fx,
                                                                    cam.fy, cam.cx, cam.cy, cam.height, cam.width, RO.BLOCK)
        _PROJ["v"] = (cam, xys, depths, radii, conics, nth)
    return _PROJ["v"]


def _pair_case(n, axis, sign, with_table):
    """Rows of the real projection tiled / truncated to n (n = 1: a visible row); every 17th row from the 5th has its
    radius cleared as the projection clears a culled row.  The motion is fast along the shutter axis in the direction
    that makes near points keep pace with the shutter (k < 0.5 on those; shifts of up to ~13 px push border rows off
    the image); with a table, object 1 moves moderately and object 2 carries that fast motion instead of the camera."""
    from sgn_rast import shutter
    cam, xys, depths, radii, conics, nth = _projection()
    first = int(torch.nonzero((radii > 0) & (depths > 8))[0])
    idx = torch.tensor([first]) if n == 1 else torch.arange(n) % xys.shape[0]
    xys, depths, radii, conics, nth = (t[idx].clone() for t in (xys, depths, radii, conics, nth))
    dead = torch.arange(5, max(n, 6), 17)[: (n > 5)]
    xys[dead], depths[dead], radii[dead], nth[dead] = 0.0, 0.0, 0, 0
    T = 0.03 * sign
    fast = [0.0, 0.0, 0.0]
    fast[1 if axis == "rows" else 0] = -60.0 * sign
    # (the slow part keeps the sign of both screen velocities over the whole image: a row whose velocity crosses zero
    # has sigma = 1 + 1e-6 or so, and its ceil(r sigma) is not a question float32 can answer)
    slow = (0.5, -0.3, 0.5)
    ang = (0.8, 0.9, -0.3)
    if with_table:
        rs = shutter.RollingShutter(slow, ang, T, axis, margin=0)
        obj_vel = torch.tensor([[0.0, 0.0, 0.0], [-1.5, 0.5, -1.0], [-f for f in fast]])
        ids = (torch.arange(n) % 3).to(torch.int32)
    else:
        rs = shutter.RollingShutter(tuple(s + f for s, f in zip(slow, fast)), ang, T, axis, margin=0)
        obj_vel = ids = None
    g = torch.Generator().manual_seed(7 * n + 1)
    v = (torch.randn(n, 2, generator=g), torch.randn(n, generator=g), torch.randn(n, 3, generator=g))
    return cam, rs, (xys, depths, radii, conics, nth), ids, obj_vel, v


def _oracle_pair(cam, rs, inputs, ids, obj_vel, v, dtype):
    xys, depths, radii, conics, _ = inputs
    x, d, q = (t.detach().clone().to(dtype).requires_grad_(True) for t in (xys, depths, conics))
    table = None
    if obj_vel is not None:                     # l_k = R (v_cam - v_obj[k]) with R = I, formed in float32 as the host does
        table = torch.tensor(rs.lin_vel, dtype=torch.float32)[None, :] - obj_vel
    out = RO.apply(x, d, radii, q, cam, rs, object_ids=ids, lin_table=table, dtype=dtype)
    (out[0] * v[0].to(dtype)).sum().add((out[1] * v[1].to(dtype)).sum()).add((out[3] * v[2].to(dtype)).sum()).backward()
    return [t.detach() for t in out[:5]], (x.grad, d.grad, q.grad), out[5]


def _kernel_pair(cam, rs, inputs, ids, obj_vel, v):
    from sgn_rast import shutter
    xys, depths, radii, conics, nth = inputs
    x, d, q = (t.detach().to(DEV).requires_grad_(True) for t in (xys, depths, conics))
    out = shutter.apply(x, d, radii.to(DEV), q, nth.to(DEV), cam, rs, RO.BLOCK,
                        object_ids=None if ids is None else ids.to(DEV),
                        object_velocities=None if obj_vel is None else obj_vel.to(DEV))
    assert type(out[0].grad_fn).__name__ == "_ShearBackward"                       # the kernel ran
    assert out[2].dtype == torch.int32 and out[4].dtype == torch.int32 and not out[2].requires_grad
    ((out[0] * v[0].to(DEV)).sum() + (out[1] * v[1].to(DEV)).sum() + (out[3] * v[2].to(DEV)).sum()).backward()
    return [t.detach().cpu() for t in out], (x.grad.cpu(), d.grad.cpu(), q.grad.cpu())


@pytest.mark.parametrize("with_table", [False, True], ids=["camera", "objects"])
@pytest.mark.parametrize("sign", [1, -1], ids=["T>0", "T<0"])
@pytest.mark.parametrize("axis", ["rows", "cols"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_pair_per_element_against_float64(n, axis, sign, with_table):
    """Integer outputs and the culled set: equal to the float32 oracle's, except on rows where a value under a ceil or a
    trunc lies within 1e-5 relative of an integer in float64 (at most 1 % of the rows).  xys', depths', conics': every
    element within 8x the float32 oracle's own largest error against float64 on these inputs; the three gradients: rel-L2
    within 8x the float32 oracle's.  Culled rows hold exact zeros, in the outputs and in the gradients.
    Measured (profiles/rolling_shutter.md): the kernel's errors EQUAL the float32 oracle's on the forward (same bits);
    the gradients' worst ratio to the oracle's own error is 4.1 (v_conics, an n = 1 case), below 1.8 from 255 rows on."""
    case = _pair_case(n, axis, sign, with_table)
    o32, g32, aux32 = _oracle_pair(*case, torch.float32)
    o64, g64, aux64 = _oracle_pair(*case, torch.float64)
    got, gg = _kernel_pair(*case)
    pre = aux64.pre_int
    near = ((pre - pre.round()).abs() <= 1e-5 * pre.abs().clamp(min=1.0)).any(dim=-1) & aux64.valid
    assert int(near.sum()) <= 0.01 * n, int(near.sum())
    keep = ~near
    alive = got[2] > 0
    assert torch.equal(alive[keep], aux32.alive[keep])
    assert torch.equal(got[2][keep], o32[2][keep]) and torch.equal(got[4][keep], o32[4][keep])
    assert torch.equal(aux32.alive[keep], aux64.alive[keep])                       # (the oracles themselves agree)
    if n >= 255:                                                                   # the case holds what it claims to
        inputs = case[2]
        assert int((inputs[2] == 0).sum()) > 0 and int((aux64.valid & (aux64.k < 0.5)).sum()) > 0
        assert int((aux64.valid & ~(aux64.k < 0.5) & ~aux64.alive).sum()) > 0 and int(alive.sum()) > n // 4
    # culled rows: exact zeros
    dead = ~alive
    for t in (got[0], got[1], got[2], got[4], gg[0], gg[1], gg[2]):
        assert bool((t[dead] == 0).all())
    names = ("xys'", "depths'", "conics'")
    line = []
    assert torch.equal(_bits(got[3][~aux64.valid]), _bits(case[2][3][~aux64.valid]))   # a row the projection culled keeps its conic
    for name, k in zip(names, (0, 1, 3)):
        sel = keep & (aux64.valid if k == 3 else alive)            # (the conic is written on the rows the pass culls, too)
        own = float((o32[k].double() - o64[k])[sel].abs().max()) if bool(sel.any()) else 0.0
        err = float((got[k].double() - o64[k])[sel].abs().max()) if bool(sel.any()) else 0.0
        line.append(f"{name} {err:.2e} (oracle32 {own:.2e})")
        assert err <= 8 * own, (name, err, own)
    for name, a, b32, b64 in zip(("v_xys", "v_depths", "v_conics"), gg, g32, g64):
        sel = keep
        own, err = rel_l2(b32[sel], b64[sel]), rel_l2(a[sel], b64[sel])
        line.append(f"{name} {err:.2e} (oracle32 {own:.2e})")
        assert err <= 8 * own, (name, err, own)
    print(f"[rs pair] n={n} {axis} sign={sign} table={with_table}: " + "  ".join(line) +
          f"  alive {int(alive.sum())} near-integer rows {int(near.sum())}")


def test_an_absent_depth_gradient_is_a_null_pointer():
    """No gradient through depths': the node hands the kernel NULL, and the result is that of a zero gradient."""
    from sgn_rast import shutter
    cam, rs, inputs, ids, obj_vel, v = _pair_case(257, "rows", 1, True)
    res = []
    for with_depth in (False, True):
        x, d, q = (t.detach().to(DEV).requires_grad_(True) for t in (inputs[0], inputs[1], inputs[3]))
        out = shutter.apply(x, d, inputs[2].to(DEV), q, inputs[4].to(DEV), cam, rs, RO.BLOCK, object_ids=ids.to(DEV),
                            object_velocities=obj_vel.to(DEV))
        loss = (out[0] * v[0].to(DEV)).sum() + (out[3] * v[2].to(DEV)).sum()
        if with_depth:
            loss = loss + (out[1] * 0.0).sum()
        loss.backward()
        res.append((x.grad, d.grad, q.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 2. zero motion

def _gpu_projection(cam, raw, rs=None):
    from sgn_rast import fused, shutter
    P = _to_dev(raw)
    return fused.project_gaussians_fused(P["means"], P["log_scales"], P["quats"], cam.viewmat[:3, :], cam.fx, cam.fy,
                                         *shutter.projection_frame(cam, rs), RO.BLOCK)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("axis,duration", [("rows", 0.03), ("cols", -0.03)])
def test_zero_motion_margin_0_is_the_identity_bit_for_bit(axis, duration):
    from sgn_rast import shutter, step
    cam, raw = RO.scene()
    cam = _dev_cam(cam)
    rs = shutter.RollingShutter((0, 0, 0), (0, 0, 0), duration, axis, margin=0)
    xys, depths, radii, conics, _, nth, _ = _gpu_projection(cam, raw)
    out = shutter.apply(xys, depths, radii, conics, nth, cam, rs, RO.BLOCK)
    assert int((radii > 0).sum()) > 100 and int((radii == 0).sum()) > 0
    for got, want in zip(out, (xys, depths, radii, conics, nth)):
        assert got.data_ptr() != want.data_ptr() and torch.equal(_bits(got), _bits(want))
    # ... with an object table of zeros as well
    ids = (torch.arange(xys.shape[0], device=DEV) % 3).to(torch.int32)
    out = shutter.apply(xys, depths, radii, conics, nth, cam, rs, RO.BLOCK, object_ids=ids,
                        object_velocities=torch.zeros(3, 3, device=DEV))
    for got, want in zip(out, (xys, depths, radii, conics, nth)):
        assert torch.equal(_bits(got), _bits(want))
    with torch.no_grad():
        plain = step.render_fused(_to_dev(raw), cam, 0, with_depth=True)
        still = step.render_fused(_to_dev(raw), cam, 0, with_depth=True, rolling_shutter=rs)
    for k in ("rgb", "alpha", "depth"):
        assert torch.equal(getattr(plain, k), getattr(still, k)), k
    assert float(plain.alpha.mean()) > 0.3


def test_zero_motion_margin_16_differs_by_the_margins_rounding_only():
    from sgn_rast import shutter
    cam, raw = RO.scene()
    cam = _dev_cam(cam)
    rs = shutter.RollingShutter((0, 0, 0), (0, 0, 0), 0.03, "rows", margin=16)
    xys, depths, radii, conics, _, nth, _ = _gpu_projection(cam, raw)
    out = shutter.apply(*[t for i, t in enumerate(_gpu_projection(cam, raw, rs)) if i in (0, 1, 2, 3, 5)], cam, rs, RO.BLOCK)
    vis = radii > 0
    assert int(vis.sum()) > 100 and int((out[2] > 0).sum()) >= int(vis.sum())
    assert torch.equal(out[2][vis], radii[vis]) and torch.equal(out[4][vis], nth[vis])
    assert torch.equal(_bits(out[3][vis]), _bits(conics[vis])) and torch.equal(_bits(out[1][vis]), _bits(depths[vis]))
    ulp = 2.0 ** -17                           # of W + 2 m = 96: two half-ulp roundings, adding and subtracting m
    assert float((out[0][vis] - xys[vis]).abs().max()) <= ulp


# ---------------------------------------------------------------- 3. the time-sliced truth

@pytest.fixture(scope="module")
def hip_ops():
    from sgn_rast import ops
    return ops


def _oracle_compensated(raw, cam, rs):
    from oracle import torch_oracle as O
    return RO.compensated_image(O, raw, cam, rs)


@pytest.mark.parametrize("name", list(RO.MOTIONS))
def test_compensated_render_against_oracle_and_time_sliced_truth(name, hip_ops):
    """`render_fused(rolling_shutter=)` within 1e-4 max-abs of the oracle's compensated image (projection, oracle shear
    and rasterizer on the CPU), and better than the global-shutter render against the truth — rendered line by line
    through the product's own operators — by the threshold the CPU test derives."""
    from sgn_rast import shutter, step
    lin, ang, T, axis = RO.MOTIONS[name]
    cam, raw = RO.scene()
    rs = shutter.RollingShutter(lin, ang, T, axis)
    want = _oracle_compensated(raw, cam, rs)
    cam_d, raw_d = _dev_cam(cam), _to_dev(raw)
    with torch.no_grad():
        got = step.render_fused(raw_d, cam_d, 0, rolling_shutter=rs).rgb
        plain = step.render_fused(raw_d, cam_d, 0).rgb
        truth = RO.truth_image(hip_ops, raw_d, cam_d, rs)
    err = float((got.cpu() - want).abs().max())
    p_plain, p_comp = RO.psnr(plain, truth), RO.psnr(got, truth)
    print(f"[rs truth] {name}: max|err| vs oracle {err:.2e}; uncompensated {p_plain:.2f} dB, compensated {p_comp:.2f} dB")
    assert err <= 1e-4
    assert p_comp - p_plain >= MOTION_GAIN_DB


def test_margin_against_oracle_and_time_sliced_truth(hip_ops):
    from sgn_rast import shutter, step
    lin, ang, T, axis = RO.EDGE_MOTION
    cam, raw = RO.edge_scene()
    cam_d, raw_d = _dev_cam(cam), _to_dev(raw)
    psnr = {}
    with torch.no_grad():
        truth = RO.truth_image(hip_ops, raw_d, cam_d, shutter.RollingShutter(lin, ang, T, axis))[:8]
        for m in (0, 16):
            rs = shutter.RollingShutter(lin, ang, T, axis, margin=m)
            got = step.render_fused(raw_d, cam_d, 0, rolling_shutter=rs).rgb
            err = float((got.cpu() - _oracle_compensated(raw, cam, rs)).abs().max())
            psnr[m] = RO.psnr(got[:8], truth)
            print(f"[rs margin] margin {m}: max|err| vs oracle {err:.2e}; top 8 rows {psnr[m]:.2f} dB")
            assert err <= 1e-4
    assert psnr[16] - psnr[0] >= MARGIN_GAIN_DB


# ---------------------------------------------------------------- 4. through the layers

class _ShearedOps:
    """An operator namespace whose projection is followed by the ORACLE's shear under autograd: the expected side of the
    layer tests runs `step.render` / `train_step` on it without `rolling_shutter=`."""

    def __init__(self, ops, cam, rs, lin_table=None, counts=None):
        self.spherical_harmonics, self.rasterize_gaussians, self._project = (
            ops.spherical_harmonics, ops.rasterize_gaussians, ops.project_gaussians)
        self.cam, self.rs, self.lin_table = cam, rs, lin_table
        self.ids = None if counts is None else torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))

    def project_gaussians(self, means, scales, glob, quats, viewmat, fx, fy, cx, cy, H, W, block, *a):
        from sgn_rast import shutter
        pcx, pcy, pH, pW = shutter.projection_frame(self.cam, self.rs)
        xys, depths, radii, conics, comp, nth, cov = self._project(means, scales, glob, quats, viewmat, fx, fy, pcx, pcy,
                                                                   pH, pW, block, *a)
        xys, depths, radii, conics, nth, _ = RO.apply(xys, depths, radii, conics, self.cam, self.rs, block,
                                                      object_ids=self.ids, lin_table=self.lin_table)
        return xys, depths, radii, conics, comp, nth, cov


def _oracle_photometric(rgb, gt, lam):
    from oracle import torch_oracle as O
    l1, s = O.l1_ssim_losses(rgb, gt)
    return (1 - lam) * l1 + lam * (1 - s)


RS_STEP = dict(lin_vel=(1.0, 0.2, 6.0), ang_vel=(0.05, 0.5, 0.1), duration=0.03)


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "drop-in"])
def test_train_step_matches_the_oracle_composition(fused, mode):
    """project -> the oracle's shear under autograd -> rasterize -> loss on the C oracle, against `train_step(gt=,
    rolling_shutter=)`: every leaf gradient rel-L2 <= 1e-4, the classic mode's tolerance (smoke())."""
    import oracle_ops
    from sgn_rast import scenes, shutter, step
    cam, raw = scenes.make_scene("c1", n_override=2000)
    rs = shutter.RollingShutter(**RS_STEP)
    gt = torch.rand(cam.height, cam.width, 3, generator=torch.Generator().manual_seed(4))
    w_img, w_a = step.loss_weights(cam, seed=7)
    Pc = step.leaf_params(raw)
    exp = step.train_step(Pc, cam, w_img, w_a, ops=_ShearedOps(oracle_ops, cam, rs), gt=gt, loss_fn=_oracle_photometric,
                          rasterize_mode=mode)
    Pn = step.leaf_params(raw)
    none = step.train_step(Pn, cam, w_img, w_a, ops=oracle_ops, gt=gt, loss_fn=_oracle_photometric, rasterize_mode=mode)
    assert float((exp.rgb - none.rgb).detach().abs().mean()) > 1e-3 and rel_l2(Pn["means"].grad, Pc["means"].grad) > 0.05
    cam_d = _dev_cam(cam)
    Pd = step.leaf_params(_to_dev(raw))
    got = step.train_step(Pd, cam_d, w_img.to(DEV), w_a.to(DEV), gt=gt.to(DEV), fused=fused, rasterize_mode=mode,
                          rolling_shutter=rs)
    torch.cuda.synchronize()
    mism = float((got.radii.cpu() != exp.radii).float().mean())
    e_img = float((got.rgb.detach().cpu() - exp.rgb.detach()).abs().max())
    rels = {k: rel_l2(Pd[k].grad.cpu(), Pc[k].grad) for k in Pd}
    print(f"[rs step] fused={fused} {mode}: radii mismatch {mism:.2e}  rgb max|err| {e_img:.2e}  loss err "
          f"{abs(float(got.loss) - float(exp.loss)):.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    assert mism < 1e-3 and abs(float(got.loss) - float(exp.loss)) < 1e-5
    for k, v in rels.items():
        assert v <= 1e-4, (k, v)
    # out.xys is the sheared one, and its gradient is retained
    assert float((got.xys.detach().cpu() - exp.xys.detach())[exp.radii > 0].abs().max()) < 2e-3
    assert got.xys.grad is not None and got.xys.grad.shape == got.xys.shape


def _graph_scene():
    from sgn_rast import scenes
    cam = scenes.make_camera(160, 96, 140.0)
    models, poses, idft = scenes.make_scene_graph(800, cam, n_objects=3, object_frac=0.3, z_range=(2.0, 8.0))
    poses[1:, 11] = torch.tensor([4.0, 5.0, 6.0])
    poses[1:, 9] = torch.tensor([-1.0, 0.2, 1.0]); poses[1:, 10] = 0.0
    return cam, models, poses, idft


def test_scene_graph_both_paths_with_object_velocities():
    """The fused path (group accumulations, and the two id-range passes) against the drop-in path under a rolling
    shutter with a per-object velocity table: the scene-graph replay's tolerances (tests/test_gpu_fused.py); an object's
    own velocity moves its rows and no others."""
    from sgn_rast import scenes, shutter, step
    cam, models, poses, idft = _graph_scene()
    counts = [m["means"].shape[0] for m in models]
    assert len(models) == 4 and 200 < sum(counts) < 1000
    rs = shutter.RollingShutter((2.0, 0.0, 8.0), (0.0, 0.4, 0.0), 0.03)
    vel = torch.tensor([[0.0, 0.0, 0.0], [6.0, 0.0, 2.0], [0.0, 0.0, 0.0], [-4.0, 1.0, -3.0]])
    w_img, w_a = (t.to(DEV) for t in step.loss_weights(cam, seed=7))

    def run(object_velocities=vel, **kw):
        leaves = [step.leaf_params(_to_dev(m)) for m in models]
        out = step.render_scene_graph(leaves, poses.to(DEV), idft.to(DEV), _dev_cam(cam), rolling_shutter=rs,
                                      object_velocities=None if object_velocities is None else object_velocities.to(DEV),
                                      **kw)
        loss = ((out.rgb * w_img).sum() + (out.alpha * w_a).sum() + (out.object_acc * w_a).sum()) / (cam.height * cam.width)
        loss.backward()
        return out, leaves

    ref, Lr = run()
    for name, kw in (("fused groups", dict(fused=True, groups=True)), ("fused id-range", dict(fused=True, groups=False))):
        got, Lg = run(**kw)
        assert float((got.radii != ref.radii).float().mean()) < 2e-3, name
        for k in ("rgb", "alpha", "object_acc", "background_acc"):
            err = (getattr(got, k).detach() - getattr(ref, k).detach()).abs()
            assert float(err.mean()) < 2e-5 and float((err > 1e-3).float().mean()) < 5e-3, (name, k, float(err.mean()))
        rels = [rel_l2(mg[k].grad, mr[k].grad) for mg, mr in zip(Lg, Lr) for k in mg]
        print(f"[rs graph] {name} vs drop-in: worst grad rel-L2 {max(rels):.2e}")
        assert max(rels) < 2e-3, name
    assert float(ref.object_acc.max()) > 0.5 and float(ref.background_acc.max()) > 0.5
    # a moving object shears differently from the background: its rows move, the others keep their bits
    for kw in (dict(fused=True), dict()):
        still, _ = run(object_velocities=torch.zeros(4, 3), **kw)
        moved, _ = run(**kw)
        parts_s, parts_m = torch.split(still.xys.detach(), counts), torch.split(moved.xys.detach(), counts)
        vis = torch.split((still.radii > 0) & (moved.radii > 0), counts)
        assert torch.equal(parts_s[0], parts_m[0]) and torch.equal(parts_s[2], parts_m[2])
        for o in (1, 3):
            assert float((parts_s[o] - parts_m[o])[vis[o]].abs().max()) > 0.25, o
        assert not torch.equal(still.rgb, moved.rgb)
    with pytest.raises(ValueError):
        step.render_scene_graph([_to_dev(m) for m in models], poses.to(DEV), idft.to(DEV), _dev_cam(cam),
                                object_velocities=vel.to(DEV))


def test_render_eval_returns_the_compensated_image():
    from sgn_rast import scenes, shutter, step
    cam, raw = scenes.make_scene("c1", n_override=2000)
    cam, P = _dev_cam(cam), _to_dev(raw)
    rs = shutter.RollingShutter(**RS_STEP)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    with torch.no_grad():
        want = step.render_fused(P, cam, 3, background=bg, with_depth=True, rolling_shutter=rs)
    for fused in (True, False):
        got = step.render_eval(P, cam, bg, fused=fused, rolling_shutter=rs)
        plain = step.render_eval(P, cam, bg, fused=fused)
        if fused:
            assert torch.equal(got["rgb"], want.rgb.clamp(0.0, 1.0)) and torch.equal(got["depth"], want.depth)
        assert float((got["rgb"] - want.rgb.clamp(0.0, 1.0)).abs().mean()) < 1e-6
        assert float((got["rgb"] - plain["rgb"]).abs().mean()) > 1e-3


def test_absgrad_and_the_densifier_read_the_sheared_xys():
    from sgn_rast import densify, scenes, shutter, step
    cam = scenes.make_camera(56, 40, 60.0, device=DEV)
    raw = scenes.make_gaussians(400, scenes.make_camera(56, 40, 60.0), seed=5, z_range=(1.0, 5.0), device=DEV)
    rs = shutter.RollingShutter((3.0, 0.0, 4.0), (0.0, 0.8, 0.0), 0.03)
    w_img, w_a = step.loss_weights(cam, seed=2, device=DEV)
    P = step.leaf_params(raw)
    d = densify.Densifier(P, {k: None for k in densify.PARAM_NAMES}, densify.DensifyConfig(absgrad=True))
    out = step.train_step(P, cam, w_img, w_a, fused=True, absgrad=True, densifier=d, step=0, rolling_shutter=rs)
    torch.cuda.synchronize()
    assert type(out.xys.grad_fn).__name__ == "_ShearBackward"                      # out.xys is the pass's result
    assert out.xys.absgrad.shape == (400, 2) and float(out.xys.absgrad.abs().max()) > 0
    by_hand = densify.Stats()
    by_hand.update(out.xys.absgrad, out.radii, (cam.height, cam.width), step=0)
    assert torch.equal(d.stats.xys_grad_norm, by_hand.xys_grad_norm) and torch.equal(d.stats.vis_counts, by_hand.vis_counts)
    Q = step.leaf_params(raw)
    plain = step.train_step(Q, cam, w_img, w_a, fused=True, absgrad=True)
    assert not torch.equal(plain.xys.absgrad, out.xys.absgrad) and not torch.equal(plain.radii, out.radii)


@pytest.mark.parametrize("fused", [False, True])
def test_empty_view_falls_through(fused):
    from sgn_rast import scenes, shutter, step
    cam = scenes.make_camera(64, 48, 64.0, device=DEV)
    raw = scenes.make_gaussians(300, cam, seed=0, z_range=(1.0, 4.0))
    raw["means"][:, 2] = -5.0                                    # everything behind the camera
    raw = _to_dev(raw)
    w_img, w_a = (t.to(DEV) for t in step.loss_weights(cam))
    rs = shutter.RollingShutter(**RS_STEP)
    outs = {}
    for key, kw in (("plain", {}), ("rs", dict(rolling_shutter=rs))):
        P = step.leaf_params(raw)
        outs[key] = o = step.train_step(P, cam, w_img, w_a, with_depth=True, fused=fused, caller_syncs=True, **kw)
        torch.cuda.synchronize()
        assert int(o.radii.sum()) == 0 and float(o.loss) == 0.0
        assert o.rgb.shape == (48, 64, 3) and float(o.rgb.abs().max()) == 0.0 and float(o.alpha.abs().max()) == 0.0
        for k, p in P.items():
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert torch.equal(outs["plain"].rgb, outs["rs"].rgb)

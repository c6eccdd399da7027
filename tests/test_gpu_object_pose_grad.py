"""GPU: the pose-table gradient of the fused projection (csrc/project.hip POSE, sgn_project_bwd_fused_pose) against
an fp64 torch-oracle, against an fp64 reduction of the kernel's own per-Gaussian outputs at 1 M Gaussians, its
run-to-run determinism, and pose recovery with :class:`sgn_rast.poses.ObjectPoses`."""
import math
import time

import pytest
import torch

import pose_oracle as PO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _rot(yaw, pitch):
    Ry = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]])
    return (Ry @ Rx).float()


def _models(counts, behind=(), seed=4, F=5):
    """Background + objects sized ``counts[1:]`` in their local frames (test_gpu_fused._scene_graph_scene's shape);
    objects listed in ``behind`` sit behind the camera."""
    from sgn_rast import fused, scenes
    cam = scenes.make_camera(160, 96, 140.0)
    g = torch.Generator().manual_seed(seed)
    models, Rs, ts = [], [torch.eye(3)], [torch.zeros(3)]
    for k, cnt in enumerate(counts):
        raw = scenes.make_gaussians(cnt, cam, seed=seed + k, z_range=(2.0, 8.0))
        dc = torch.randn(cnt, F if k else 1, 3, generator=g) * 0.3
        dc[:, 0] += raw["features_dc"][:, 0]
        raw["features_dc"] = dc
        if k:
            raw["means"] = torch.randn(cnt, 3, generator=g) * 0.4
            Rs.append(_rot(0.7 * k, -0.3 * k))
            ts.append(torch.tensor([0.5 * ((k % 4) - 1.5), 0.1 * (k % 3), (-5.0 if k in behind else 4.0 + 0.3 * k)]))
        models.append(raw)
    poses = fused.make_pose_table(torch.stack(Rs), torch.stack(ts))
    from oracle import torch_oracle as TO
    idft = torch.stack([torch.cat([torch.ones(1), torch.zeros(F - 1)])] +
                       [TO.idft(0.1 + 0.8 * k / len(counts), F) for k in range(1, len(counts))])
    return cam, models, poses, idft


def _render_loss(models_d, poses_d, idft_d, cam, seed=7):
    from sgn_rast import step
    out = step.render_scene_graph(models_d, poses_d, idft_d, cam, fused=True, sh_parts=False)
    for t in (out.depths, out.conics):
        t.retain_grad()
    g = torch.Generator().manual_seed(seed)
    H, W = cam.height, cam.width
    w = [torch.rand(*s, generator=g).to(DEV) for s in ((H, W, 3), (H, W), (H, W, 1), (H, W), (H, W))]
    loss = ((out.rgb * w[0]).sum() + (out.alpha * w[1]).sum() + (out.depth * w[2]).sum() * 0.01 +
            (out.object_acc * w[3]).sum() + (out.background_acc * w[4]).sum()) / (H * W)
    return out, loss


CASES = {
    "one_object": [2500, 600],
    "two_objects": [2500, 600, 400],
    # rows start mid-wave and cross workgroups; a 1-Gaussian object, an empty one, one behind the camera (id 7)
    "eight_objects": [2000, 37, 1, 0, 300, 129, 64, 250, 513],
}


@pytest.mark.parametrize("case", list(CASES))
def test_pose_grad_matches_fp64_oracle(case):
    from sgn_rast import fused
    counts = CASES[case]
    behind = (7,) if case == "eight_objects" else ()
    cam, models, poses, idft = _models(counts, behind=behind)
    cam.viewmat, cam.cam_pos = cam.viewmat.to(DEV), cam.cam_pos.to(DEV)
    md = [{k: v.to(DEV).requires_grad_(True) for k, v in m.items()} for m in models]
    pd = poses.to(DEV).requires_grad_(True)
    out, loss = _render_loss(md, pd, idft.to(DEV), cam)
    loss.backward()
    assert pd.grad is not None, "no gradient reached the pose table"
    got = pd.grad.cpu().double()
    ids = fused.object_ids_for(counts, "cpu")
    cat = lambda key: torch.cat([m[key] for m in models])
    vis = out.radii.cpu() > 0
    n = ids.shape[0]
    grad_or_zero = lambda t, shape: t.grad.cpu() if t.grad is not None else torch.zeros(shape)
    ref = PO.table_vjp(cat("means"), cat("log_scales"), cat("quats"), ids, poses, cam, grad_or_zero(out.xys, (n, 2)),
                       grad_or_zero(out.depths, (n,)), grad_or_zero(out.conics, (n, 3)), vis)
    offs = [0] + list(torch.cumsum(torch.tensor(counts), 0).tolist())
    for o in range(len(counts)):
        live = bool(vis[offs[o]:offs[o + 1]].any())
        if not live:                     # zero-count object, or entirely culled: exact zeros
            assert torch.equal(got[o], torch.zeros(16, dtype=torch.float64)), (case, o, got[o])
            continue
        for name, sl in (("R", slice(0, 9)), ("t", slice(9, 12)), ("q", slice(12, 16))):
            err = rel_l2(got[o, sl], ref[o, sl])
            assert err <= 1e-4, (case, o, name, err, got[o, sl], ref[o, sl])
    if case == "eight_objects":
        assert not bool(vis[offs[7]:offs[8]].any()) and counts[3] == 0 and counts[2] == 1


def _at_size_inputs(seed=3):
    from sgn_rast import fused, scenes
    cam = scenes.make_camera(1920, 1280, 2000.0)
    models, poses, _idft = scenes.make_scene_graph(1_000_000, cam, n_objects=8, object_frac=0.3)
    counts = [m["means"].shape[0] for m in models]
    cat = lambda key: torch.cat([m[key] for m in models]).to(DEV)
    cam.viewmat, cam.cam_pos = cam.viewmat.to(DEV), cam.cam_pos.to(DEV)
    ids = fused.object_ids_for(counts, DEV)
    g = torch.Generator().manual_seed(seed)
    n = sum(counts)
    ups = [torch.randn(n, 2, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV),
           torch.randn(n, 3, generator=g).to(DEV)]
    return cam, counts, cat("means"), cat("log_scales"), cat("quats"), ids, poses.to(DEV), ups


def _project_bwd(cam, m, ls, q, ids, poses, ups, pose_grad=True):
    from sgn_rast import fused
    leaves = [t.detach().clone().requires_grad_(True) for t in (m, ls, q)]
    p = poses.detach().clone().requires_grad_(pose_grad)
    xys, depths, radii, conics, _c, _n, _cov = fused.project_gaussians_fused(
        *leaves, cam.viewmat[:3, :], cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, 16, object_ids=ids,
        poses=p)
    loss = (xys * ups[0]).sum() + (depths * ups[1]).sum() + (conics * ups[2]).sum()
    grads = torch.autograd.grad(loss, leaves + ([p] if pose_grad else []))
    return grads, radii


def test_pose_grad_at_size_against_kernel_outputs():
    cam, counts, m, ls, q, ids, poses, ups = _at_size_inputs()
    (vm, vs, vq, vp), radii = _project_bwd(cam, m, ls, q, ids, poses, ups)
    (vm0, vs0, vq0), _ = _project_bwd(cam, m, ls, q, ids, poses, ups, pose_grad=False)
    for a, b in ((vm, vm0), (vs, vs0), (vq, vq0)):
        assert torch.equal(a, b), "per-Gaussian gradients must not change with the pose gradient on"
    idc = ids.cpu()
    v_w, gq, v_w_mag, g_mag = PO.from_kernel_outputs(poses.cpu(), idc, vm.cpu(), vq.cpu())
    vis = (radii.cpu() > 0).double()[:, None]
    s, a = PO.closed_form(m.cpu(), q.cpu(), idc, v_w * vis, gq * vis, len(counts), v_w_mag * vis, g_mag * vis)
    got = vp.cpu().double()
    worst = []
    for o, n_o in enumerate(counts):
        bound = (math.ceil(math.log2(max(n_o, 2))) + 8) * 2.0 ** -24 * a[o]
        err = (got[o] - s[o]).abs()
        assert bool((err <= bound).all()), (o, n_o, err, bound)
        worst.append(float((err / bound.clamp_min(1e-300)).max()))
    print(f"at size: largest |err|/bound per object {[f'{w:.3g}' for w in worst]}")


def test_pose_grad_is_deterministic_also_on_a_side_stream():
    cam, counts, m, ls, q, ids, poses, ups = _at_size_inputs(seed=5)
    (_, _, _, a), _ = _project_bwd(cam, m, ls, q, ids, poses, ups)
    (_, _, _, b), _ = _project_bwd(cam, m, ls, q, ids, poses, ups)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (_, _, _, c), _ = _project_bwd(cam, m, ls, q, ids, poses, ups)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert bool(a.abs().sum() > 0)


def _recovery_scene(n_total=200_000, n_obj=4, seed=11):
    """Background + 4 textured boxes of Gaussians, 4 cameras at 960x640 looking at them from different positions."""
    from sgn_rast import scenes
    g = torch.Generator().manual_seed(seed)
    cam0 = scenes.make_camera(960, 640, 900.0)
    n_o = n_total // 10
    n_bg = n_total - n_o * n_obj
    bg = scenes.make_gaussians(n_bg, cam0, seed=seed, z_range=(30.0, 60.0), sh_degree=1)
    models = [bg]
    rots, centers = [], []
    for k in range(n_obj):
        m = scenes.make_gaussians(n_o, cam0, seed=seed + 1 + k, sh_degree=1, scale_range=(0.02, 0.06))
        m["means"] = (torch.rand(n_o, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.7, 1.6])
        m["opacity_logits"] = torch.full((n_o, 1), 3.0)
        # a smooth texture (wavelengths of 1-3 m): the loss keeps a wide basin around the true pose
        u = m["means"]
        col = torch.stack([torch.sin(2.1 * u[:, 0] + 1.3 * u[:, 1] + k), torch.sin(1.7 * u[:, 1] - 2.3 * u[:, 2]),
                           torch.sin(2.9 * u[:, 2] + 1.1 * u[:, 0] - k)], -1)
        m["features_dc"] = (0.4 * col / 0.2820947917738781)[:, None, :]
        m["features_rest"] = m["features_rest"] * 0.0
        models.append(m)
        rots.append(_rot(0.8 * k - 1.2, 0.0))
        centers.append(torch.tensor([3.0 * k - 4.5, 0.5, 14.0 + 2.0 * (k % 2)]))
    cams = []
    for c in range(4):
        x = 2.0 * c - 3.0
        cam = scenes.make_camera(960, 640, 900.0, yaw=0.06 * (1.5 - c))
        cam.viewmat[:3, 3] = -(cam.viewmat[:3, :3] @ torch.tensor([x, 0.0, 0.0]))
        cam.cam_pos = torch.tensor([x, 0.0, 0.0])
        cam.viewmat, cam.cam_pos = cam.viewmat.to(DEV), cam.cam_pos.to(DEV)
        cams.append(cam)
    return models, torch.stack(rots), torch.stack(centers), cams


def _axis_angle(R):
    return math.degrees(math.acos(max(-1.0, min(1.0, (float(torch.trace(R)) - 1) / 2))))


def test_pose_recovery_with_object_poses():
    from sgn_rast import poses as PS
    from sgn_rast import step
    t0 = time.time()
    torch.manual_seed(0)
    models, rots, centers, cams = _recovery_scene()
    md = [{k: v.to(DEV) for k, v in m.items()} for m in models]
    F = 1
    idft = torch.ones(len(models), F, device=DEV)
    rots_d, centers_d = rots.to(DEV, torch.float64), centers.to(DEV, torch.float64)
    frame, tracks = torch.zeros(4, dtype=torch.long, device=DEV), torch.arange(4, device=DEV)
    with torch.no_grad():
        true_table = PS.ObjectPoses(1, 4, "off", DEV).table(frame, tracks, centers_d, rots_d)
        targets = [step.render_scene_graph(md, true_table, idft, c, sh_degree_to_use=1, fused=True).rgb for c in cams]
    # perturb every object by 0.3 m and 5 degrees about a per-object axis
    g = torch.Generator().manual_seed(1)
    axes = torch.nn.functional.normalize(torch.randn(4, 3, generator=g, dtype=torch.float64), dim=-1)
    dirs = torch.nn.functional.normalize(torch.randn(4, 3, generator=g, dtype=torch.float64), dim=-1)
    dR = PS.exp_map_SO3xR3(torch.cat([torch.zeros(4, 3, dtype=torch.float64), axes * math.radians(5.0)], 1))[:, :, :3]
    noisy_rots = (dR @ rots.double()).to(DEV)
    noisy_centers = (centers.double() + 0.3 * dirs).to(DEV)
    op = PS.ObjectPoses(1, 4, "SO3xR3", DEV)
    opt = torch.optim.Adam(op.param_groups()["bbox_opt"], lr=1e-2)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.99)
    torch.cuda.synchronize()
    for it in range(300):
        opt.zero_grad(set_to_none=True)
        torch.cuda.set_sync_debug_mode("error")
        table = op.table(frame, tracks, noisy_centers, noisy_rots)
        torch.cuda.set_sync_debug_mode(0)
        c = it % len(cams)
        out = step.render_scene_graph(md, table, idft, cams[c], sh_degree_to_use=1, fused=True)
        loss = (out.rgb - targets[c]).abs().mean()
        gt = torch.autograd.grad(loss, table)[0]
        torch.cuda.set_sync_debug_mode("error")
        table.backward(gt)
        torch.cuda.set_sync_debug_mode(0)
        opt.step()
        sched.step()
    c_fit, R_fit = op.corrected(frame, tracks, noisy_centers, noisy_rots)
    t_err = [float(torch.from_numpy(c_fit[k]).sub(centers[k].double()).norm()) for k in range(4)]
    a_err = [_axis_angle(torch.from_numpy(R_fit[k]) @ rots[k].double().T) for k in range(4)]
    took = time.time() - t0
    print(f"recovery: translation errors {[f'{e:.4f}' for e in t_err]} m, angles {[f'{e:.3f}' for e in a_err]} deg, "
          f"{took:.1f} s")
    assert max(t_err) < 0.05 and max(a_err) < 1.0, (t_err, a_err)
    assert took < 60.0

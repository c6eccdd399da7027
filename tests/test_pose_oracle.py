"""CPU: the fp64 pose-vjp oracle of tests/pose_oracle.py checks itself — the closed-form per-object sums of
v_w m^T, v_w and M_R(q_raw)^T g, chained through the quaternion of the rotation, against autograd through
torch_oracle.object2world_gs + project_gaussians."""
import math

import torch

import pose_oracle as PO
from oracle import torch_oracle as TO


def test_closed_form_sums_match_autograd_through_the_oracle():
    from sgn_rast import fused, poses, scenes
    d = torch.float64
    cam = scenes.make_camera(96, 64, 80.0)
    g = torch.Generator().manual_seed(3)
    counts = [200, 150, 1, 90]
    raw = scenes.make_gaussians(sum(counts), cam, seed=2, z_range=(2.0, 6.0))
    ids = fused.object_ids_for(counts, "cpu")
    means = raw["means"].to(d)
    means[counts[0]:] = torch.randn(sum(counts[1:]), 3, generator=g, dtype=d) * 0.4
    quats, ls = raw["quats"].to(d), raw["log_scales"].to(d)
    Rs = [torch.eye(3, dtype=d)] + [poses.exp_map_SO3xR3(torch.tensor([0, 0, 0, 0.3 * k, 1.1 * k, -0.4], dtype=d))[:3, :3]
                                    for k in range(1, 4)]
    Rs[3] = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=d)) @ Rs[3]            # a trace <= 0 rotation
    ts = [torch.zeros(3, dtype=d)] + [torch.tensor([0.4 * k - 0.6, 0.1, 3.0 + 0.2 * k], dtype=d) for k in range(1, 4)]
    vis = None
    w = [torch.randn(sum(counts), 2, generator=g, dtype=d), torch.randn(sum(counts), generator=g, dtype=d),
         torch.randn(sum(counts), 3, generator=g, dtype=d)]

    def loss_of(mw, qw):
        nonlocal vis
        xys, depths, radii, conics, _c, _n, _cov = TO.project_gaussians(
            mw, ls.exp(), 1.0, qw / qw.norm(dim=-1, keepdim=True), cam.viewmat.to(d)[:3, :], cam.fx, cam.fy, cam.cx,
            cam.cy, cam.height, cam.width, 16)
        vis = (radii > 0).to(d)
        return (((w[0] * xys).sum(-1) + w[1] * depths + (w[2] * conics).sum(-1)) * vis).sum()

    # autograd through object2world_gs (the quaternion derived from R inside) + project_gaussians
    Rl = [R.clone().requires_grad_(True) for R in Rs]
    tl = [t.clone().requires_grad_(True) for t in ts]
    parts = [TO.object2world_gs(means[ids == o], quats[ids == o], Rl[o], tl[o]) for o in range(4)]
    loss_of(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])).backward()

    # closed form: per-Gaussian world gradients, per-object sums, then the quaternion chained back to R
    table = poses.pose_rows(torch.stack(Rs), torch.stack(ts))
    mw, qw = PO.world_from_table(means, quats, ids, table)
    mw, qw = mw.detach().requires_grad_(True), qw.detach().requires_grad_(True)
    loss_of(mw, qw).backward()
    s, _ = PO.closed_form(means, quats, ids, mw.grad, qw.grad, 4)
    assert float(vis[ids == 2].sum()) == 1.0
    for o in range(4):
        R = Rs[o].clone().requires_grad_(True)
        q = poses.pose_rows(R[None], ts[o][None])[0, 12:16]
        (dq,) = torch.autograd.grad(q, R, s[o, 12:16])
        dR = s[o, :9].reshape(3, 3) + dq
        assert torch.allclose(dR, Rl[o].grad, rtol=1e-9, atol=1e-9), (o, dR, Rl[o].grad)
        assert torch.allclose(s[o, 9:12], tl[o].grad, rtol=1e-9, atol=1e-9), o

    # and the table vjp (independent R, t, q columns) equals the same per-object sums
    vjp = PO.table_vjp(means, ls, quats, ids, table, cam, w[0], w[1], w[2], vis > 0)
    assert torch.allclose(vjp, s, rtol=1e-9, atol=1e-9)
    assert math.isfinite(float(s.abs().sum()))

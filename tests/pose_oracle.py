"""fp64 oracles of the pose-table gradient of the fused projection (sgn_project_bwd_fused_pose).

``table_vjp``: torch-oracle autograd — world means / quaternions from the table's columns (R, t, q_o2w taken as
independent inputs, as the kernel reads them), ``torch_oracle.project_gaussians`` in fp64, and the upstream gradients
of the projection outputs on the visible rows; returns dL/dtable [M,16].

``closed_form``: the per-Gaussian sums the kernel reduces — v_R = v_w m^T, v_t = v_w, v_q = M_R(q_raw)^T g — from the
world-mean gradient v_w and the un-normalised world-quaternion gradient g, per object; also the per-element sums of
|term| for the rounding bound."""
import torch

from oracle import torch_oracle as TO


def world_from_table(means, quats, ids, table):
    """means_w = R m + t, q_w = q_o2w (x) q_raw per row, with R, t, q read from the table rows ``ids``."""
    P = table[ids.long()]
    R = P[:, :9].reshape(-1, 3, 3)
    means_w = (R @ means[:, :, None])[:, :, 0] + P[:, 9:12]
    a, b = P[:, 12:16], quats
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    quats_w = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                           aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)
    return means_w, quats_w


def table_vjp(means, log_scales, quats, ids, table, cam, v_xys, v_depths, v_conics, vis, block=16):
    """fp64 dL/dtable for L = sum(v_xys xys + v_depths depths + v_conics conics) over the rows ``vis``."""
    d = torch.float64
    tab = table.detach().to(d).clone().requires_grad_(True)
    mw, qw = world_from_table(means.detach().to(d), quats.detach().to(d), ids, tab)
    qn = qw / qw.norm(dim=-1, keepdim=True)
    xys, depths, _r, conics, _c, _n, _cov = TO.project_gaussians(
        mw, log_scales.detach().to(d).exp(), 1.0, qn, cam.viewmat.detach().cpu().to(d)[:3, :], cam.fx, cam.fy, cam.cx,
        cam.cy, cam.height, cam.width, block)
    m = vis.to(d)
    loss = ((v_xys.to(d) * xys).sum(-1) * m).sum() + (v_depths.to(d) * depths * m).sum() + \
        ((v_conics.to(d) * conics).sum(-1) * m).sum()
    loss.backward()
    return tab.grad


def _terms(m, b, v_w, g):
    vR = (v_w[:, :, None] * m[:, None, :]).reshape(-1, 9)
    bw, bx, by, bz = b.unbind(-1)
    vq = torch.stack([bw * g[:, 0] + bx * g[:, 1] + by * g[:, 2] + bz * g[:, 3],
                      -bx * g[:, 0] + bw * g[:, 1] - bz * g[:, 2] + by * g[:, 3],
                      -by * g[:, 0] + bz * g[:, 1] + bw * g[:, 2] - bx * g[:, 3],
                      -bz * g[:, 0] - by * g[:, 1] + bx * g[:, 2] + bw * g[:, 3]], -1)
    return torch.cat([vR, v_w, vq], 1)


def closed_form(means, quats, ids, v_w, g, m_rows, v_w_mag=None, g_mag=None):
    """fp64 [m_rows,16] per-object sums of the 16 per-Gaussian pose terms, and the sums of the terms' magnitudes: the
    terms evaluated on |inputs| (each product of a dot product counted by its absolute value), with ``v_w_mag`` /
    ``g_mag`` the magnitudes v_w and g were computed from (default |v_w|, |g|)."""
    d = torch.float64
    m, b, v_w, g = means.to(d), quats.to(d), v_w.to(d), g.to(d)
    terms = _terms(m, b, v_w, g)
    vwm = v_w.abs() if v_w_mag is None else v_w_mag.to(d)
    gm = g.abs() if g_mag is None else g_mag.to(d)
    # the products of each M_R(q_raw)^T g dot product counted by magnitude: at most sum_j |b_j| max_j |g_j|
    mags = torch.cat([(vwm[:, :, None] * m.abs()[:, None, :]).reshape(-1, 9), vwm,
                      (b.abs().sum(-1) * gm.max(dim=-1).values)[:, None].expand(-1, 4)], 1)
    idx = ids.long()[:, None].expand(-1, 16)
    s = torch.zeros(m_rows, 16, dtype=d).scatter_add_(0, idx, terms)
    a = torch.zeros(m_rows, 16, dtype=d).scatter_add_(0, idx, mags)
    return s, a


def from_kernel_outputs(table, ids, v_means_local, v_quats_raw):
    """The kernel's v_w and g recovered from its per-Gaussian outputs with exact identities (fp64):
    v_w = R v_local (R orthonormal to fp32 rounding) and g = M_L(q_o2w) v_qraw / |q_o2w|^2.  Also their magnitudes
    |R| |v_local| and |M_L(q_o2w)| |v_qraw| / |q_o2w|^2, the scale of the rounding both directions carry."""
    d = torch.float64
    P = table.to(d)[ids.long()]
    R = P[:, :9].reshape(-1, 3, 3)
    v_w = (R @ v_means_local.to(d)[:, :, None])[:, :, 0]
    a, u = P[:, 12:16], v_quats_raw.to(d)
    aw, ax, ay, az = a.unbind(-1)
    # v_qraw = M_L(a)^T g and M_L(a) M_L(a)^T = |a|^2 I
    Lg = torch.stack([aw * u[:, 0] - ax * u[:, 1] - ay * u[:, 2] - az * u[:, 3],
                      ax * u[:, 0] + aw * u[:, 1] - az * u[:, 2] + ay * u[:, 3],
                      ay * u[:, 0] + az * u[:, 1] + aw * u[:, 2] - ax * u[:, 3],
                      az * u[:, 0] - ay * u[:, 1] + ax * u[:, 2] + aw * u[:, 3]], -1)
    n2 = (a * a).sum(-1, keepdim=True)
    g = Lg / n2
    g_mag = (a.norm(dim=-1) * u.norm(dim=-1))[:, None].expand(-1, 4) / n2[:, 0, None]      # = |g|
    v_w_mag = (R.abs() @ v_means_local.to(d).abs()[:, :, None])[:, :, 0]
    return v_w, g, v_w_mag, g_mag

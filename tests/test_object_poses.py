"""CPU: sgn_rast.poses — the exp maps against fp64 matrix_exp, pose_rows against fused.make_pose_table and gradcheck,
ObjectPoses' tables against fused.scene_graph_tables, the "simple" mode against apply_to_bbox's formulas, non-trainable
tracks and the regulariser."""
import math
import sys
import os

import numpy as np
import pytest
import torch

from sgn_rast import fused
from sgn_rast import poses as PS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "stubs"))
from nerfstudio.cameras.lie_groups import exp_map_SO3xR3 as stub_SO3xR3  # noqa: E402

D = torch.float64


def _tangents(seed=0, scales=(1e-3, 0.05, 0.7, 2.5)):
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in scales:
        v = torch.randn(4, 6, generator=g, dtype=D)
        v[:, 3:] = torch.nn.functional.normalize(v[:, 3:], dim=-1) * s
        out.append(v)
    return torch.cat(out)


def _hat(w):
    return PS._skew(w)


def test_so3xr3_matches_matrix_exp_and_the_clamped_stub():
    v = _tangents()
    got = PS.exp_map_SO3xR3(v)
    big = (v[:, 3:].norm(dim=-1) > 1e-2)
    ref = torch.linalg.matrix_exp(_hat(v[:, 3:]))
    assert torch.allclose(got[big, :, :3], ref[big], atol=1e-12)
    assert torch.allclose(got[:, :, 3], v[:, :3], atol=0)
    # around 1e-3 rad the squared angle is clamped at 1e-4 as nerfstudio does: equal to its restatement, and within the
    # clamp's error of the exact exponential
    assert torch.allclose(got, stub_SO3xR3(v), atol=1e-15)
    assert torch.allclose(got[~big, :, :3], ref[~big], atol=1e-5)
    assert not torch.allclose(got[~big, :, :3], ref[~big], atol=1e-9)


def test_se3_matches_matrix_exp_of_the_twist():
    v = _tangents(seed=1, scales=(0.0, 1e-4, 3e-3, 0.05, 0.9, 2.8))
    got = PS.exp_map_SE3(v)
    X = torch.zeros(v.shape[0], 4, 4, dtype=D)
    X[:, :3, :3] = _hat(v[:, 3:])
    X[:, :3, 3] = v[:, :3]
    ref = torch.linalg.matrix_exp(X)[:, :3, :]
    assert torch.allclose(got, ref, atol=1e-12), float((got - ref).abs().max())


def _rotations(seed=2):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(12, 3, generator=g, dtype=D)
    w = torch.nn.functional.normalize(w, dim=-1) * torch.linspace(0.1, 3.1, 12, dtype=D)[:, None]
    Rs = PS.exp_map_SO3xR3(torch.cat([torch.zeros(12, 3, dtype=D), w], 1))[:, :, :3]
    flips = torch.stack([torch.diag(torch.tensor(d, dtype=D)) for d in
                         ([-1.0, -1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0])])
    extra = torch.cat([flips, flips @ Rs[:3], torch.eye(3, dtype=D)[None]])         # trace <= 0, ties, identity
    return torch.cat([Rs, extra])


def test_pose_rows_matches_make_pose_table_within_2_ulp():
    R = _rotations().to(torch.float32)
    t = torch.randn(R.shape[0], 3, generator=torch.Generator().manual_seed(3))
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    assert bool((tr <= 0).sum() >= 4)
    got, ref = PS.pose_rows(R, t), fused.make_pose_table(R, t)
    assert got.dtype == torch.float32
    ulp = torch.finfo(torch.float32).eps * ref.abs().clamp_min(torch.finfo(torch.float32).tiny)
    assert bool(((got - ref).abs() <= 2 * ulp).all()), (got - ref).abs().max()


def test_pose_rows_gradcheck():
    R = _rotations()
    # keep every row away from the branch switches (trace 0, diagonal ties): the function is smooth there
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    d = torch.diagonal(R, dim1=1, dim2=2).sort(dim=-1).values
    ok = (tr.abs() > 1e-3) & ((d[:, 2] - d[:, 1]) > 1e-3)
    R = R[ok].clone().requires_grad_(True)
    t = torch.randn(R.shape[0], 3, dtype=D, requires_grad=True)
    assert bool((R.detach()[:, 0, 0] + R.detach()[:, 1, 1] + R.detach()[:, 2, 2] <= 0).any())
    assert torch.autograd.gradcheck(PS.pose_rows, (R, t))


def _boxes(k=3, seed=4):
    g = torch.Generator().manual_seed(seed)
    R = _rotations(seed)[[1, 5, 13][:k]]
    c = torch.randn(k, 3, generator=g, dtype=D) * 5
    return c, R


def test_zero_initialised_object_poses_reproduce_scene_graph_tables():
    c, R = _boxes()
    frame, tracks = torch.tensor([2, 2, 2]), torch.tensor([0, 2, 1])
    for mode in ("off", "SO3xR3", "SE3"):
        op = PS.ObjectPoses(4, 3, mode)
        got = op.table(frame, tracks, c, R)
        q = fused.make_pose_table(R, c)[:, 12:16]
        ref = fused.scene_graph_tables([10, 5, 5, 5], [(R[k].numpy(), c[k].numpy(), q[k].numpy()) for k in range(3)],
                                       [None] * 3, "cpu")["poses"]
        ulp = torch.finfo(torch.float32).eps * ref.abs()
        assert bool(((got - ref).abs() <= 2 * ulp).all()), (mode, (got - ref).abs().max())


def _quat_from_matrix_np(R):
    return fused.make_pose_table(torch.from_numpy(R)[None], torch.zeros(1, 3))[0, 12:16].double().numpy()


def _quat_mul_np(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _quat_matrix_np(q):
    """nerfstudio camera_utils.quaternion_matrix, restated."""
    q = np.array(q, dtype=np.float64)
    q *= math.sqrt(2.0 / np.dot(q, q))
    q = np.outer(q, q)
    return np.array([[1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0]],
                     [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0]],
                     [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2]]])


def test_simple_mode_matches_apply_to_bbox():
    c, R = _boxes()
    op = PS.ObjectPoses(3, 3, "simple")
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        op.delta_center.copy_(torch.randn(3, 3, 3, generator=g) * 0.2)
        op.delta_yaw.copy_(torch.randn(3, 3, generator=g) * 0.3)
    frame, tracks = torch.tensor([1, 1, 1]), torch.tensor([2, 0, 1])
    cc, RR = op.corrected(frame, tracks, c, R)
    for k in range(3):
        f, b = 1, int(tracks[k])
        # apply_to_bbox, "simple": center + delta_center; quaternion_multiply(q_box, (cos psi, 0, 0, sin psi))
        psi = float(op.delta_yaw[f, b].detach())
        q = _quat_mul_np(_quat_from_matrix_np(R[k].numpy()), np.array([math.cos(psi), 0, 0, math.sin(psi)]))
        np.testing.assert_allclose(cc[k], c[k].numpy() + op.delta_center[f, b].detach().double().numpy(), atol=1e-7)
        np.testing.assert_allclose(RR[k], _quat_matrix_np(q), atol=1e-7)
    assert float(op.regularizer()) == 0.0


def test_corrections_do_not_accumulate():
    c, R = _boxes()
    op = PS.ObjectPoses(1, 3, "SO3xR3")
    with torch.no_grad():
        op.pose_adjustment.copy_(torch.randn(1, 3, 6, generator=torch.Generator().manual_seed(6)) * 0.1)
    f, t = torch.zeros(3, dtype=torch.long), torch.arange(3)
    a, b = op.table(f, t, c, R), op.table(f, t, c, R)
    assert torch.equal(a, b)
    C = PS.exp_map_SO3xR3(op.pose_adjustment[0].detach().double())
    cc, RR = op.corrected(f, t, c, R)
    np.testing.assert_allclose(RR, (C[:, :, :3] @ R).numpy(), atol=1e-12)
    np.testing.assert_allclose(cc, (c + C[:, :, 3]).numpy(), atol=1e-12)


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3", "simple"])
def test_non_trainable_tracks_get_identity_and_no_gradient(mode):
    c, R = _boxes()
    op = PS.ObjectPoses(2, 3, mode, non_trainable=[1])
    with torch.no_grad():
        for p in op.parameters():
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(7)) * 0.1)
    f, t = torch.ones(3, dtype=torch.long), torch.arange(3)
    table = op.table(f, t, c, R)
    ref = fused.make_pose_table(R, c)
    assert torch.equal(table[2], ref[1])                                  # track 1: the annotation as it is
    assert not torch.allclose(table[1], ref[0])
    table.sum().backward()
    for p in op.parameters():
        assert torch.equal(p.grad[:, 1], torch.zeros_like(p.grad[:, 1]))
        assert bool(p.grad[1, 0].abs().sum() > 0)
    assert torch.equal(table[0], fused.make_pose_table(torch.eye(3)[None], torch.zeros(1, 3))[0])


def test_regularizer_values_and_param_groups():
    op = PS.ObjectPoses(2, 3, "SO3xR3")
    with torch.no_grad():
        op.pose_adjustment.copy_(torch.arange(36, dtype=torch.float32).reshape(2, 3, 6) / 10)
    a = op.pose_adjustment.detach().double()
    ref = a[..., :3].norm(dim=-1).mean() * 1e-2 + a[..., 3:].norm(dim=-1).mean() * 1e-3
    assert abs(float(op.regularizer()) - float(ref)) < 1e-6
    assert list(op.param_groups()) == ["bbox_opt"] and op.param_groups()["bbox_opt"][0] is op.pose_adjustment
    assert PS.ObjectPoses(2, 3, "off").param_groups() == {"bbox_opt": []}
    assert float(PS.ObjectPoses(2, 3, "off").regularizer()) == 0.0
    with pytest.raises(ValueError):
        PS.ObjectPoses(1, 1, "bogus")


def test_object_offsets_validate_foreign_ids():
    ids = torch.tensor([0, 0, 1, 1, 1, 3], dtype=torch.int32)
    assert fused.object_offsets(ids, 4).tolist() == [0, 2, 5, 5, 6]
    with pytest.raises(ValueError):
        fused.object_offsets(torch.tensor([0, 1, 0], dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        fused.object_offsets(torch.tensor([0, 1, 2], dtype=torch.int32), 2)
    cached = fused.object_ids_for([3, 0, 2], "cpu")
    assert fused.object_offsets(cached, 3).tolist() == [0, 3, 3, 5]

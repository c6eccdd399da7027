"""CPU: the fp64 two-cloud brute force of tests/cloud_nn_oracle.py (the checker of the GPU search and of the chamfer
metric) on answers known by construction, and its restatements of the LiDAR filters and transform."""
import numpy as np

import cloud_nn_oracle as CO


def test_shifted_lattice_is_half_a_cell_away_both_ways():
    q, t = CO.lattice_pair()
    for a, b in ((q, t), (t, q)):
        d, i = CO.nearest_brute(a, b)
        assert d.shape == (1000,) and i.shape == (1000,) and i.dtype == np.int64
        assert (d == 0.5).all()
        assert ((i >= 0) & (i < 1000)).all()
        np.testing.assert_array_equal(np.linalg.norm(a.astype(np.float64) - b[i], axis=1), d)
    d1, d2 = CO.chamfer(q, t)
    assert d1 == 0.5 / CO.CD_UNIT and d2 == 0.5 / CO.CD_UNIT


def test_asymmetric_pair_by_hand():
    pred, gt, d1, d2 = CO.asymmetric_pair()
    d, i = CO.nearest_brute(pred, gt)
    np.testing.assert_array_equal(d, [0.0, 3.0])
    np.testing.assert_array_equal(i, [0, 2])
    d, i = CO.nearest_brute(gt, pred)
    np.testing.assert_array_equal(d, [0.0, 3.0, 1.0, 12.0])
    np.testing.assert_array_equal(i, [0, 0, 0, 0])
    got = CO.chamfer(pred, gt)
    assert d1 != d2
    np.testing.assert_allclose(got, (d1, d2), rtol=1e-15)
    np.testing.assert_allclose(CO.chamfer(gt, pred), (d2, d1), rtol=1e-15)      # the order of the pair follows the arguments


def test_chunking_does_not_change_the_answer():
    q, t = CO.cloud("uniform_n1000"), CO.cloud("uniform_n777")
    d0, i0 = CO.nearest_brute(q, t, chunk=1000)
    d1, i1 = CO.nearest_brute(q, t, chunk=37)
    np.testing.assert_array_equal(d0, d1)
    np.testing.assert_array_equal(i0, i1)
    full = np.linalg.norm(q.astype(np.float64)[:, None] - t.astype(np.float64)[None], axis=-1)
    np.testing.assert_allclose(d0, full.min(1), rtol=1e-15)


def test_ego_box_faces_are_kept_and_nan_rows_dropped():
    faces = np.array([[3, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 2], [0, 0, -1]], dtype=np.float64)
    inside = np.array([[2.999, 0, 0], [-0.999, 0.999, 1.999], [0, -0.999, -0.999], [0, 0, 0]])
    outside = np.array([[3.001, 0, 0], [0, 5, 0], [0, 0, -7], [-50, 0.5, 0.5]])
    nan = np.array([[np.nan, 10, 10], [10, np.nan, 10], [0, 0, np.nan]])
    p = np.concatenate([faces, inside, nan, outside])
    np.testing.assert_array_equal(CO.filter_lidar(p), np.concatenate([faces, outside]))          # order preserved
    np.testing.assert_array_equal(CO.filter_lidar(p, filter_ego=False), np.concatenate([faces, inside, outside]))
    kept = CO.filter_lidar(p, ignore_nan=False)
    assert kept.shape[0] == 6 + 3 + 4 and np.isnan(kept).any(axis=1).sum() == 3   # a NaN compares false: never "inside"
    assert CO.filter_lidar(p, ignore_nan=False, filter_ego=False).shape == p.shape


def test_lidar_transform_by_hand():
    # translation (1, 2, 3) is added as (2, 1, -3); then a quarter turn about z, a shift, a scale
    rot = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    transform = np.concatenate([rot, [[10.0], [20.0], [30.0]]], 1)
    got = CO.lidar_to_scene([[1.0, 1.0, 1.0]], [1.0, 2.0, 3.0], transform, 0.5)
    # p + shift = (3, 2, -2); R p = (-2, 3, -2); + T = (8, 23, 28); * 0.5
    np.testing.assert_allclose(got, [[4.0, 11.5, 14.0]], rtol=1e-15)
    four = np.concatenate([transform, [[0, 0, 0, 1.0]]])
    np.testing.assert_array_equal(CO.lidar_to_scene([[1.0, 1.0, 1.0]], [1.0, 2.0, 3.0], four, 0.5), got)


def test_lidar_scene_fixture_has_every_kind_of_row():
    means, world, translation, transform, scale = CO.lidar_scene()
    kept = CO.filter_lidar(world)
    assert np.isnan(world).any(axis=1).sum() > 10
    assert kept.shape[0] < world.shape[0] - 100 and not np.isnan(kept).any()
    np.testing.assert_array_equal(kept[:6], world[:6])                  # the six face points survive, in order
    np.testing.assert_allclose(transform[:, :3] @ transform[:, :3].T, np.eye(3), atol=1e-15)
    res = CO.evaluate_lidar_geometric(means, world, translation, transform, scale)
    assert 0 < res["lidar_chamfer_distance_1"] < res["lidar_chamfer_distance_2"]       # means cover half the cloud
    assert res["lidar_chamfer_distance_avg"] == (res["lidar_chamfer_distance_1"] + res["lidar_chamfer_distance_2"]) / 2

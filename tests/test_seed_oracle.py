"""CPU: the numpy restatement of the LiDAR seeding contract (tests/seed_oracle.py) on hand-built known answers, the
float32 restatement against the float64 one on every generated scene the GPU test uses, and `sweep_to_world` against the
reference's literal sequence of row and column operations.

Float32 against float64: a point is *threshold-adjacent* when, in float64, some ||loc[k]| - half[k]| < 5e-5, or
|pc.z| < 5e-5, or u or v lies within 5e-4 of an integer.  The two restatements may differ on adjacent points only, and
adjacent points are at most 1 % of the live points of every scene (a condition on the scenes, which the seeds of
seed_oracle.SCENES / ACC_SCENES meet).  Over 80 further seeds at (4 099 points, 7 boxes) and (20 000 points, 64 boxes)
this generator gave: worst adjacent share 0.72 %, 7 differing points among 899 k live ones, none outside the adjacent
set."""
import numpy as np
import pytest

import seed_oracle as SO
from sgn_rast import seed

EYE34 = np.eye(4, dtype=np.float32)[:3]


def _unit_scene(points, boxes, **kw):
    """Identity LiDAR pose; a camera at the origin looking along +z with fx = fy = 10, cx = cy = 8 into 16 x 16."""
    sc = dict(points=np.asarray(points, np.float32).reshape(-1, 3), l2w=EYE34, boxes=boxes, w2c=EYE34, fx=10.0, fy=10.0,
              cx=8.0, cy=8.0, width=16, height=16, min_z=-2.0)
    sc.update(kw)
    return sc


def _img16():
    return SO.image(5, 16, 16)


AXIS_BOX = SO.make_boxes([[0.0, 0.0, 4.0]], [np.eye(3)], [[2.0, 1.0, 2.0]], scale=1.0)      # half = (1, 0.5, 1)


def test_axis_aligned_box_identity_transforms():
    pts = [[0.25, -0.25, 4.5],      # inside: loc = (0.25, -0.25, 0.5); u = trunc(2.5 / 4.5 + 8) = 8, v = trunc(8 - 0.55) = 7
           [0.25, 0.75, 4.5],       # outside along y -> background; v = trunc(7.5 / 4.5 + 8) = 9
           [3.0, 0.0, 1.0]]         # u = 38: off the image
    img = _img16()
    out = SO.seed_sweep(_unit_scene(pts, AXIS_BOX), img)
    assert out["offsets"] == [0, 1] and out["totals"] == [1, 1, 3]
    assert np.array_equal(out["local"], np.array([[0.25, -0.25, 0.5]], np.float32)) and out["local"].dtype == np.float32
    assert out["obj_src"].tolist() == [0] and np.array_equal(out["obj_rgb"][0], img[7, 8])
    assert np.array_equal(out["world"], np.array([[0.25, 0.75, 4.5]], np.float32))
    assert out["bg_src"].tolist() == [1] and np.array_equal(out["bg_rgb"][0], img[9, 8])


def test_a_point_on_a_face_is_inside():
    out = SO.seed_sweep(_unit_scene([[1.0, 0.0, 4.0], [0.0, 0.5, 5.0], [np.nextafter(np.float32(1.0), np.float32(2.0)), 0.0, 4.0]],
                                    AXIS_BOX), _img16())
    assert out["obj_src"].tolist() == [0, 1] and out["bg_src"].tolist() == [2]


def test_u_of_minus_a_half_is_column_zero():
    # fu = (10 * -0.85 + 8 * 1) / 1 = -0.5 -> trunc = -0 -> column 0, visible; fu = -1 exactly is not
    img = _img16()
    out = SO.seed_sweep(_unit_scene([[-0.85, 0.0, 1.0], [-0.9, 0.0, 1.0]], np.zeros((0, 15), np.float32)), img)
    c = SO.classify(**_unit_scene([[-0.85, 0.0, 1.0], [-0.9, 0.0, 1.0]], np.zeros((0, 15), np.float32)))
    assert -0.51 < float(c["fu"][0]) < -0.49 and c["ok"].tolist() == [True, False]
    assert out["bg_src"].tolist() == [0] and np.array_equal(out["bg_rgb"][0], img[8, 0])


def test_camera_plane_and_behind_are_invisible():
    out = SO.seed_sweep(_unit_scene([[0.0, 0.0, 0.0], [0.1, 0.1, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]],
                                    np.zeros((0, 15), np.float32)), _img16())
    assert out["bg_src"].tolist() == [3] and out["totals"] == [1, 4]


def test_min_z_is_strict_and_far_x_is_dropped():
    l2w = EYE34.copy(); l2w[2, 3] = 10.0            # z_lidar = -2 is world z = 8: in front of the camera
    pts = [[0.0, 0.0, -2.0], [0.0, 0.0, np.nextafter(np.float32(-2.0), np.float32(0.0))], [0.0, 0.0, -2.5],
           [100000.0, 0.0, 1.0], [100000.01, 0.0, 1.0], [-100000.01, 0.0, 1.0], [np.nan, 0.0, 1.0], [0.0, 0.0, np.nan]]
    c = SO.classify(**_unit_scene(pts, np.zeros((0, 15), np.float32), l2w=l2w))
    assert c["live"].tolist() == [False, True, False, True, False, False, False, False]
    out = SO.partition(c, _img16())
    assert out["bg_src"].tolist() == [1] and out["totals"] == [1, 2]


def test_a_point_inside_two_boxes_is_in_both_and_order_is_stable():
    boxes = SO.make_boxes([[0.0, 0.0, 4.0], [0.5, 0.0, 4.0]], [np.eye(3), np.eye(3)], [[2.0, 2.0, 2.0]] * 2, scale=1.0)
    pts = [[0.9, 0.0, 4.0],         # both boxes
           [-0.9, 0.0, 4.0],        # box 0 only
           [5.0, 5.0, 100.0],       # visible background
           [1.4, 0.0, 4.0],         # box 1 only
           [0.0, 0.1, 4.2]]         # both
    out = SO.seed_sweep(_unit_scene(pts, boxes), _img16())
    assert out["offsets"] == [0, 3, 6]
    assert out["obj_src"].tolist() == [0, 1, 4, 0, 3, 4] and out["bg_src"].tolist() == [2]
    assert np.array_equal(out["local"][0], np.array([0.9, 0.0, 0.0], np.float32))
    assert np.array_equal(out["local"][3], np.array([np.float32(0.9) - np.float32(0.5), 0.0, 0.0], np.float32))
    assert out["totals"] == [3, 3, 1, 5]


def test_rotated_box_uses_the_transpose():
    R = SO._rot([0, 0, 1], np.pi / 2)               # box x axis = world y
    boxes = SO.make_boxes([[0.0, 0.0, 4.0]], [R], [[4.0, 1.0, 1.0]], scale=1.0)
    out = SO.seed_sweep(_unit_scene([[0.0, 1.5, 4.0], [1.5, 0.0, 4.0]], boxes), _img16())
    assert out["obj_src"].tolist() == [0] and abs(float(out["local"][0, 0]) - 1.5) < 1e-6


def test_sweep_to_world_is_the_literal_shuffle():
    rng = np.random.default_rng(3)
    m = np.eye(4); m[:3] = rng.normal(size=(3, 4)) * 10
    t0 = rng.normal(size=3) * 100
    l2w = m.copy()                                  # the reference's sequence, operation for operation
    l2w[0:3, 1:3] *= -1
    l2w = l2w[np.array([1, 0, 2, 3]), :]
    l2w[2, :] *= -1
    l2w[:3, 3] -= t0
    l2w[2, :] *= -1
    l2w = l2w[np.array([1, 0, 2, 3]), :]
    l2w[0:3, 1:3] *= -1
    got = seed.sweep_to_world(m, t0)
    assert got.dtype == np.float64 and np.array_equal(got, l2w)
    assert np.array_equal(got[:3, :3], m[:3, :3]) and np.array_equal(seed.sweep_to_world(m[:3], t0), l2w)
    assert np.array_equal(m[:3, 3] - got[:3, 3], np.array([t0[1], t0[0], -t0[2]]))


def test_make_boxes_matches_the_oracle_and_scales_by_1_1():
    sc = SO.scene(4099, 7, 14)
    got = seed.make_boxes([[1.0, 2.0, 3.0]], [np.eye(3)], [[4.0, 2.0, 1.0]])
    assert got.dtype == np.float32 and got.shape == (1, 15)
    assert np.array_equal(got[0, 12:], (np.array([4.0, 2.0, 1.0]) * 0.55).astype(np.float32))
    assert np.array_equal(seed.make_boxes(sc["boxes"][:, :3], sc["boxes"][:, 3:12], sc["boxes"][:, 12:] * 2.0, scale=1.0),
                          sc["boxes"])


@pytest.mark.parametrize("n,nb,s", SO.SCENES + SO.ACC_SCENES)
def test_float32_differs_from_float64_on_adjacent_points_only(n, nb, s):
    sc = SO.scene(n, nb, s)
    c32, c64 = SO.classify(dtype=np.float32, **sc), SO.classify(dtype=np.float64, **sc)
    adj, diff = SO.adjacent(c64), SO.differs(c32, c64)
    live = int(c64["live"].sum())
    share = float((adj & c64["live"]).sum()) / max(live, 1)
    print(f"n={n} boxes={nb} seed={s}: live {live}, adjacent {int((adj & c64['live']).sum())} ({100 * share:.2f} %), "
          f"differing {int(diff.sum())}")
    assert not (diff & ~adj).any()
    assert share <= 0.01
    if n >= 1000:                                   # the scenes exercise every destination
        assert c32["ok"].sum() > 0.1 * n and (c32["member"].sum(axis=0) > 0).all()
        if nb >= 2:
            assert (c32["member"][:, 0] & c32["member"][:, 1]).any()

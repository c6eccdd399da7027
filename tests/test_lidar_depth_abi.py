"""CPU: the LiDAR depth entry points (include/sgn_rast.h "LiDAR DEPTH", csrc/lidar_depth.hip) are exported with the stream
last and reject bad arguments with rc < 0 and a message that names the argument before touching the device."""
import ctypes
import math
import os

import pytest

from sgn_rast import _lib
from sgn_rast import lidar

ENTRIES = (("sgn_lidar_depth_begin", 4), ("sgn_lidar_depth_splat", 8), ("sgn_lidar_depth_finish", 7),
           ("sgn_depth_loss_fwd", 12), ("sgn_depth_loss_bwd", 12), ("sgn_depth_metrics", 10))
MAX_N = 1 << 27


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


def test_the_six_entries_are_exported_stream_last(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES:
        assert hasattr(raw, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert _lib.SIGNATURES[name][1][-1] is ctypes.c_void_p      # stream last
    assert lidar.MAX_RADIUS == 8 and lidar.WS_BYTES == 64 and lidar.KINDS == {"l1": 0, "inverse": 1}
    import sgn_rast
    assert sgn_rast.splat_depth is lidar.splat_depth and sgn_rast.depth_loss is lidar.depth_loss
    assert sgn_rast.depth_metrics is lidar.depth_metrics


FAKE = ctypes.c_void_p(0x1000)            # never dereferenced: every device pointer below fails an argument check first
FAKE2 = ctypes.c_void_p(0x2000)


def _cam(width=160, height=96):
    c = _lib.SeedCam()
    c.w2c[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    c.fx = c.fy = 100.0
    c.cx, c.cy, c.width, c.height = width / 2, height / 2, width, height
    return c


def _begin(lib, depth=1, height=96, width=160):
    return lib.sgn_lidar_depth_begin(FAKE if depth else None, height, width, None)


def _splat(lib, n=100, cam=None, points=1, l2w=1, with_cam=1, depth=1, max_depth=math.inf):
    cam = cam or _cam()
    l2w12 = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    return lib.sgn_lidar_depth_splat(n, FAKE if points else None, ctypes.addressof(l2w12) if l2w else None, -2.0,
                                     max_depth, ctypes.addressof(cam) if with_cam else None, FAKE if depth else None, None)


def _finish(lib, depth=FAKE, out=FAKE2, height=96, width=160, radius=2, rel_tol=0.05):
    return lib.sgn_lidar_depth_finish(depth, height, width, radius, rel_tol, out, None)


def _fwd(lib, h=96, w=160, dsum=1, alpha=1, target=1, kind=0, loss=1, count=1, ws=1, ws_bytes=64):
    p = lambda on: FAKE if on else None
    return lib.sgn_depth_loss_fwd(h, w, p(dsum), p(alpha), p(target), None, kind, p(loss), p(count), p(ws), ws_bytes, None)


def _bwd(lib, h=96, w=160, dsum=1, alpha=1, target=1, kind=0, v_loss=1, count=1, v_dsum=1, v_alpha=1):
    p = lambda on: FAKE if on else None
    return lib.sgn_depth_loss_bwd(h, w, p(dsum), p(alpha), p(target), None, kind, p(v_loss), p(count), p(v_dsum),
                                  p(v_alpha), None)


def _metrics(lib, h=96, w=160, dsum=1, alpha=1, target=1, out5=1, ws=1, ws_bytes=64):
    p = lambda on: FAKE if on else None
    return lib.sgn_depth_metrics(h, w, p(dsum), p(alpha), p(target), None, p(out5), p(ws), ws_bytes, None)


def _refused(lib, rc, fn, what):
    assert rc < 0, rc
    msg = lib.sgn_last_error()
    assert fn in msg and what in msg, msg


@pytest.mark.parametrize("kw,what", [(dict(width=0), b"width >= 1"), (dict(width=16385), b"width <= "),
                                     (dict(height=0), b"height >= 1"), (dict(height=16385), b"height <= "),
                                     (dict(depth=0), b"depth")])
def test_begin_refuses(lib, kw, what):
    _refused(lib, _begin(lib, **kw), b"sgn_lidar_depth_begin", what)


@pytest.mark.parametrize("kw,what", [(dict(n=0), b"n >= 1"), (dict(n=-3), b"n >= 1"), (dict(n=MAX_N + 1), b"n <= "),
                                     (dict(cam=_cam(width=0)), b"width >= 1"), (dict(cam=_cam(width=16385)), b"width <= "),
                                     (dict(cam=_cam(height=0)), b"height >= 1"),
                                     (dict(cam=_cam(height=16385)), b"height <= "), (dict(max_depth=0.0), b"max_depth"),
                                     (dict(max_depth=math.nan), b"max_depth"), (dict(points=0), b"points"),
                                     (dict(l2w=0), b"l2w12"), (dict(with_cam=0), b"cam"), (dict(depth=0), b"depth")])
def test_splat_refuses(lib, kw, what):
    _refused(lib, _splat(lib, **kw), b"sgn_lidar_depth_splat", what)


@pytest.mark.parametrize("kw,what", [(dict(width=0), b"width >= 1"), (dict(height=16385), b"height <= "),
                                     (dict(radius=-1), b"radius >= 0"), (dict(radius=9), b"radius <= "),
                                     (dict(rel_tol=1.0), b"rel_tol"), (dict(rel_tol=-0.1), b"rel_tol"),
                                     (dict(depth=None), b"depth"), (dict(out=None), b"out"),
                                     (dict(out=FAKE), b"out != depth")])
def test_finish_refuses(lib, kw, what):
    _refused(lib, _finish(lib, **kw), b"sgn_lidar_depth_finish", what)


@pytest.mark.parametrize("kw,what", [(dict(w=0), b"img_w >= 1"), (dict(w=16385), b"img_w <= "), (dict(h=0), b"img_h >= 1"),
                                     (dict(h=16385), b"img_h <= "), (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"),
                                     (dict(dsum=0), b"dsum"), (dict(alpha=0), b"alpha"), (dict(target=0), b"target"),
                                     (dict(loss=0), b"loss_out"), (dict(count=0), b"count_out"), (dict(ws=0), b"ws"),
                                     (dict(ws_bytes=63), b"ws_bytes")])
def test_loss_fwd_refuses(lib, kw, what):
    _refused(lib, _fwd(lib, **kw), b"sgn_depth_loss_fwd", what)


@pytest.mark.parametrize("kw,what", [(dict(w=0), b"img_w >= 1"), (dict(h=16385), b"img_h <= "), (dict(kind=2), b"kind"),
                                     (dict(kind=-1), b"kind"), (dict(dsum=0), b"dsum"), (dict(alpha=0), b"alpha"),
                                     (dict(target=0), b"target"), (dict(v_loss=0), b"v_loss"), (dict(count=0), b"count"),
                                     (dict(v_dsum=0), b"v_dsum"), (dict(v_alpha=0), b"v_alpha")])
def test_loss_bwd_refuses(lib, kw, what):
    _refused(lib, _bwd(lib, **kw), b"sgn_depth_loss_bwd", what)


@pytest.mark.parametrize("kw,what", [(dict(w=0), b"img_w >= 1"), (dict(h=16385), b"img_h <= "), (dict(dsum=0), b"dsum"),
                                     (dict(alpha=0), b"alpha"), (dict(target=0), b"target"), (dict(out5=0), b"out5"),
                                     (dict(ws=0), b"ws"), (dict(ws_bytes=0), b"ws_bytes")])
def test_metrics_refuses(lib, kw, what):
    _refused(lib, _metrics(lib, **kw), b"sgn_depth_metrics", what)


def test_python_validation_comes_before_any_launch():
    """Host-side errors of the module: raised on CPU tensors' shapes and values, before a device is asked for."""
    import torch
    from sgn_rast import seed, step, scenes
    cam = seed.SeedCamera(torch.eye(4), 100.0, 100.0, 80.0, 48.0, 160, 96)
    pts = torch.zeros(10, 3)
    for bad, what in (((pts[:, :2], torch.eye(4)), "shape"), ((pts.double(), torch.eye(4)), "float32"),
                      ((pts, torch.eye(3)), "l2w"), ((pts, torch.eye(4)), "device tensor")):
        with pytest.raises(ValueError, match=what):
            lidar.splat_depth(bad, cam)
    for kw, what in ((dict(radius=9), "radius"), (dict(radius=-1), "radius"), (dict(rel_tol=1.0), "rel_tol"),
                     (dict(max_depth=0.0), "max_depth")):
        with pytest.raises(ValueError, match=what):
            lidar.splat_depth((pts, torch.eye(4)), cam, **kw)
    with pytest.raises(ValueError, match="SeedCamera"):
        lidar.splat_depth((pts, torch.eye(4)), None)
    with pytest.raises(ValueError, match="at least one"):
        lidar.splat_depth([], cam)
    img = torch.ones(8, 6)
    with pytest.raises(ValueError, match="kind"):
        lidar.depth_loss(img, img, img, kind="l2")
    with pytest.raises(ValueError, match="target"):
        lidar.depth_loss(img, img, torch.ones(6, 8))
    with pytest.raises(ValueError, match="alpha"):
        lidar.depth_metrics(img, torch.ones(8, 6, 2), img)
    with pytest.raises(ValueError, match="float32"):
        lidar.depth_loss(img, img, img.double())
    with pytest.raises(ValueError, match="mask"):
        lidar.depth_loss(img, img, img, mask=torch.ones(6, 8, dtype=torch.bool))
    with pytest.raises(_lib.SgnRastError):              # no CPU fallback
        lidar.depth_loss(img, img, img)
    # train_step: a wrong target shape or kind is a ValueError before the render launches anything (CPU tensors here:
    # a launch would raise SgnRastError instead)
    c, raw = scenes.make_scene("c1", n_override=50)
    P = step.leaf_params(raw)
    w_img, w_a = step.loss_weights(c)
    with pytest.raises(ValueError, match="lidar_depth"):
        step.train_step(P, c, w_img, w_a, lidar_depth=torch.zeros(c.height, c.width + 1))
    with pytest.raises(ValueError, match="depth_loss_kind"):
        step.train_step(P, c, w_img, w_a, lidar_depth=torch.zeros(c.height, c.width), depth_loss_kind="l2")

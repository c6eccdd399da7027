"""CPU: the batched-views entry points (include/sgn_rast.h "Batched views") are exported, reject each bad argument with
its documented rc before touching the device, and sgn_rast.views validates a batch on the host before anything
launches."""
import ctypes
import os

import pytest
import torch

from sgn_rast import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


F = ctypes.c_void_p(0x1000)      # never dereferenced: every case below fails its argument check first


def _cams(b=2):
    return (_lib.ViewCam * max(b, 1))()


def test_entries_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sgn_project_views_fwd", "sgn_project_views_bwd", "sgn_sh_views_fwd", "sgn_sh_views_bwd",
                 "sgn_rasterize_views_arena_bytes", "sgn_rasterize_views_fwd_all", "sgn_rasterize_views_bwd_all"):
        assert hasattr(raw, name), name
        assert _lib.SIGNATURES[name][1][-1] is ctypes.c_void_p or name.endswith("_bytes")
    assert ctypes.sizeof(_lib.ViewCam) == 19 * 4 and _lib.VIEWS_MAX == 16


def _proj_fwd(lib, b=2, n=1000, cams=True, means=F, h=64, w=64):
    return lib.sgn_project_views_fwd(b, n, _cams(b) if cams else None, means, F, 1.0, F, h, w, 16, 0.01, F, F, F, F, F,
                                     F, F, 0, None)


def _proj_bwd(lib, b=2, n=1000, cams=True, v_means=F):
    return lib.sgn_project_views_bwd(b, n, _cams(b) if cams else None, F, F, 1.0, F, F, F, F, F, F, None, F, None,
                                     v_means, F, F, 0, 64, 64, None)


def _sh(lib, fwd, b=2, n=1000, k=16, deg=3, cams=True, ptr=F):
    if fwd:
        return lib.sgn_sh_views_fwd(b, n, k, deg, _cams(b) if cams else None, F, ptr, F, 1, F, None)
    return lib.sgn_sh_views_bwd(b, n, k, deg, _cams(b) if cams else None, F, 1, F, F, ptr, F, None)


def _fwd_all(lib, b=2, n=1000, bw=16, xys=F, cap=1 << 20, arena_bytes=None):
    ab = lib.sgn_rasterize_views_arena_bytes(b, n, cap) if arena_bytes is None else arena_bytes
    nh = ctypes.c_int64(0)
    return lib.sgn_rasterize_views_fwd_all(b, n, xys, F, F, F, F, F, 1, 64, 64, bw, F, 0, F, F, F, None, F, cap, F, F, F,
                                           F, 1 << 30, F, 4096, F, ab, None, ctypes.byref(nh), 0, 0, None, None)


def _bwd_all(lib, b=2, n=1000, v_xy=F, grad_bytes=1 << 30):
    return lib.sgn_rasterize_views_bwd_all(b, n, 10, 64, 64, F, F, F, F, F, F, F, F, F, F, 0.99, v_xy, F, F, F, F,
                                           1 << 30, F, grad_bytes, F, F, 4096, 0, None, None, None)


@pytest.mark.parametrize("call", [
    lambda lib, **kw: _proj_fwd(lib, **kw), lambda lib, **kw: _proj_bwd(lib, **kw),
    lambda lib, **kw: _sh(lib, True, **kw), lambda lib, **kw: _sh(lib, False, **kw),
    lambda lib, **kw: _fwd_all(lib, **kw), lambda lib, **kw: _bwd_all(lib, **kw)])
def test_view_count_and_row_limits(lib, call):
    assert call(lib, b=0) == -1 and b"n_views" in lib.sgn_last_error()
    assert call(lib, b=17) == -1
    assert call(lib, b=16, n=1 << 24) == -2 and b"2^28" in lib.sgn_last_error()      # 16 * 2^24 = 2^28
    assert call(lib, b=2, n=-1) == -2


def test_null_pointers_and_sizes(lib):
    assert _proj_fwd(lib, cams=False) == -4
    assert _proj_fwd(lib, means=None) == -4
    assert _proj_fwd(lib, h=0) == -3
    assert _proj_bwd(lib, cams=False) == -4
    assert _proj_bwd(lib, v_means=None) == -4
    assert _sh(lib, True, cams=False) == -4 and _sh(lib, True, ptr=None) == -4
    assert _sh(lib, False, ptr=None) == -4
    assert _sh(lib, True, k=7) == -3 and _sh(lib, True, k=4, deg=3) == -3
    assert _fwd_all(lib, bw=8) == -3
    assert _fwd_all(lib, xys=None) == -4
    assert _fwd_all(lib, cap=0) == -6
    assert _fwd_all(lib, arena_bytes=256) == -5
    assert _bwd_all(lib, v_xy=None) == -4
    assert _bwd_all(lib, grad_bytes=16) == -5
    # nothing to do: n = 0 succeeds without touching the device
    assert _proj_fwd(lib, n=0, means=None) == 0 and _sh(lib, True, n=0, ptr=None) == 0


def test_arena_size(lib):
    assert lib.sgn_rasterize_views_arena_bytes(0, 100, 1000) == 0
    assert lib.sgn_rasterize_views_arena_bytes(17, 100, 1000) == 0
    one = lib.sgn_rasterize_arena_bytes(300, 1000)
    assert lib.sgn_rasterize_views_arena_bytes(3, 100, 1000) == one + ((300 * 4 + 255) // 256) * 256


def _P(n=10):
    from sgn_rast import scenes
    cam, raw = scenes.make_scene("c1", n_override=n)
    return cam, raw


def test_host_validation_before_any_launch():
    """CPU tensors would make any launch fail: every case below must raise its host-side error first."""
    from sgn_rast import scenes, views
    cam, P = _P()
    other = scenes.make_camera(cam.width, cam.height + 16, 100.0)
    with pytest.raises(ValueError, match="image size"):
        views.render_views(P, [cam, other])
    with pytest.raises(ValueError, match="block_width"):
        views.render_views(P, [cam], block_width=8)
    with pytest.raises(ValueError, match="1 to 16"):
        views.render_views(P, [])
    with pytest.raises(ValueError, match="1 to 16"):
        views.render_views(P, [cam] * 17)
    big = dict(P, means=torch.empty((1 << 24), 3, device="meta"))
    with pytest.raises(ValueError, match="2\\^28"):
        views.render_views(big, [cam] * 16)
    with pytest.raises(ValueError, match="features_dc"):
        views.render_views(dict(P, features_dc=torch.zeros(10, 5, 3)), [cam])
    for kw in (dict(object_ids=torch.zeros(10, dtype=torch.int32)), dict(poses=torch.zeros(1, 16)),
               dict(idft=torch.ones(1, 1)), dict(group_split=3), dict(id_range=(0, 5))):
        with pytest.raises(NotImplementedError, match="scene-graph"):
            views.render_views(P, [cam], **kw)
    with pytest.raises(ValueError, match="ground-truth"):
        views.train_step_views(P, [cam, cam], [torch.zeros(cam.height, cam.width, 3)])


def test_camera_table_holds_the_single_view_values():
    from sgn_rast import views
    cam, _ = _P()
    cam.viewmat = torch.arange(16, dtype=torch.float32).reshape(4, 4) * 0.1
    cam.cam_pos = torch.tensor([0.5, -1.25, 3.0])
    t = views.cam_table([cam, cam])
    assert list(t[1].viewmat) == cam.viewmat[:3, :].reshape(-1).tolist()
    assert list(t[0].cam_pos) == [0.5, -1.25, 3.0]
    assert (t[0].fx, t[0].fy, t[0].cx, t[0].cy) == (cam.fx, cam.fy, cam.cx, cam.cy)

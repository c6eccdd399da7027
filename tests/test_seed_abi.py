"""CPU: the LiDAR seeding entry points (include/sgn_rast.h, csrc/seed.hip) are exported with the stream last, reject bad
arguments with rc < 0 and a message that names the argument before touching the device, and size their workspace from the
two counts alone."""
import ctypes
import os

import pytest

from sgn_rast import _lib
from sgn_rast import seed  # noqa: F401  (the module the entry points serve)

MAX_N = 1 << 27


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


def test_entries_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("sgn_seed_workspace_bytes", 2), ("sgn_seed_classify", 11), ("sgn_seed_emit", 17)):
        assert hasattr(raw, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    for name in ("sgn_seed_classify", "sgn_seed_emit"):
        assert _lib.SIGNATURES[name][1][-1] is ctypes.c_void_p      # stream last
    assert ctypes.sizeof(_lib.SeedBox) == 15 * 4 and ctypes.sizeof(_lib.SeedCam) == 18 * 4
    assert seed.MAX_BOXES == _lib.SEED_MAX_BOXES == 64 and seed.MAX_POINTS == MAX_N


FAKE = ctypes.c_void_p(0x1000)            # never dereferenced: every device pointer below fails an argument check first


def _cam(width=160, height=96):
    c = _lib.SeedCam()
    c.w2c[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    c.fx = c.fy = 100.0
    c.cx, c.cy, c.width, c.height = width / 2, height / 2, width, height
    return c


def _classify(lib, n=100, n_boxes=2, cam=None, points=1, l2w=1, boxes=1, with_cam=1, ws=1, totals=1, ws_bytes=1 << 40):
    cam = cam or _cam()
    l2w12 = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    table = (_lib.SeedBox * 64)()
    return lib.sgn_seed_classify(n, FAKE if points else None, ctypes.addressof(l2w12) if l2w else None, -2.0, n_boxes,
                                 ctypes.addressof(table) if boxes else None, ctypes.addressof(cam) if with_cam else None,
                                 FAKE if ws else None, ws_bytes, FAKE if totals else None, None)


def _emit(lib, n=100, n_boxes=2, width=160, height=96, points=1, image=1, ws=1, obj=1, bg=1, obj_rows=10, bg_rows=10,
          ws_bytes=1 << 40):
    o, b = (FAKE if obj else None), (FAKE if bg else None)
    return lib.sgn_seed_emit(n, FAKE if points else None, n_boxes, FAKE if image else None, width, height,
                             FAKE if ws else None, ws_bytes, o, o, o, obj_rows, b, b, b, bg_rows, None)


@pytest.mark.parametrize("kw,what", [(dict(n=0), b"n >= 1"), (dict(n=-3), b"n >= 1"), (dict(n=MAX_N + 1), b"n <= "),
                                     (dict(n_boxes=65), b"n_boxes <= "), (dict(n_boxes=-1), b"n_boxes >= 0"),
                                     (dict(cam=_cam(width=0)), b"width >= 1"), (dict(cam=_cam(width=16385)), b"width <= "),
                                     (dict(cam=_cam(height=0)), b"height >= 1"),
                                     (dict(cam=_cam(height=16385)), b"height <= ")])
def test_classify_bad_sizes_give_negative_rc_and_name_the_argument(lib, kw, what):
    assert _classify(lib, **kw) < 0
    assert b"sgn_seed_classify" in lib.sgn_last_error() and what in lib.sgn_last_error()


@pytest.mark.parametrize("kw,what", [(dict(n=0), b"n >= 1"), (dict(n=MAX_N + 1), b"n <= "), (dict(n_boxes=65), b"n_boxes <= "),
                                     (dict(width=0), b"width >= 1"), (dict(height=16385), b"height <= "),
                                     (dict(obj_rows=-1), b"obj_rows >= 0"), (dict(bg_rows=101), b"bg_rows <= "),
                                     (dict(obj_rows=100 * 64 + 1), b"obj_rows <= ")])
def test_emit_bad_sizes_give_negative_rc_and_name_the_argument(lib, kw, what):
    assert _emit(lib, **kw) < 0
    assert b"sgn_seed_emit" in lib.sgn_last_error() and what in lib.sgn_last_error()


@pytest.mark.parametrize("missing,what", [("points", b"points"), ("l2w", b"l2w12"), ("boxes", b"boxes"), ("with_cam", b"cam"),
                                          ("ws", b"ws"), ("totals", b"totals")])
def test_classify_null_pointers_are_refused(lib, missing, what):
    assert _classify(lib, **{missing: 0}) < 0 and what in lib.sgn_last_error()


@pytest.mark.parametrize("missing,what", [("points", b"points"), ("image", b"image"), ("ws", b"ws"), ("obj", b"obj_local"),
                                          ("bg", b"bg_world")])
def test_emit_null_pointers_are_refused(lib, missing, what):
    assert _emit(lib, **{missing: 0}) < 0 and what in lib.sgn_last_error()


def test_no_boxes_need_no_table_and_empty_outputs_need_no_arrays(lib):
    # n_boxes == 0 with boxes == NULL passes the pointer checks: the call is refused by the NEXT check, the workspace's
    assert _classify(lib, n_boxes=0, boxes=0, ws_bytes=0) < 0 and b"ws_bytes" in lib.sgn_last_error()
    need = lib.sgn_seed_workspace_bytes(100, 2)
    assert _emit(lib, obj=0, bg=0, obj_rows=0, bg_rows=0, ws_bytes=need) == 0       # nothing to write: no launch


def test_short_workspace_is_refused(lib):
    need = lib.sgn_seed_workspace_bytes(1000, 7)
    assert _classify(lib, n=1000, n_boxes=7, ws_bytes=need - 1) < 0 and b"ws_bytes" in lib.sgn_last_error()
    assert _emit(lib, n=1000, n_boxes=7, ws_bytes=need - 1) < 0 and b"ws_bytes" in lib.sgn_last_error()


def test_workspace_size_is_monotone_in_both_counts(lib):
    ns = (1, 63, 64, 65, 255, 256, 257, 1000, 4096, 100_000, 1 << 20, 1 << 24, MAX_N)
    for nb in (0, 1, 7, 64):
        by_n = [lib.sgn_seed_workspace_bytes(n, nb) for n in ns]
        assert all(a <= b for a, b in zip(by_n, by_n[1:])), by_n
        assert by_n[0] > 0
    for n in (1, 1000, 1 << 20):
        by_b = [lib.sgn_seed_workspace_bytes(n, nb) for nb in range(65)]
        assert all(a <= b for a, b in zip(by_b, by_b[1:])), by_b
    # a membership word and a pixel word per point, a count per destination and 256-point block, the box table
    n, nb = 1 << 20, 32
    assert lib.sgn_seed_workspace_bytes(n, nb) >= n * 12 + (n // 256) * (nb + 2) * 4 + 64 * 15 * 4
    for bad in ((0, 1), (-1, 1), (MAX_N + 1, 1), (10, -1), (10, 65)):
        assert lib.sgn_seed_workspace_bytes(*bad) == 0

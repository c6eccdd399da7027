"""CPU: the pose-gradient entry points (include/sgn_rast.h, csrc/project.hip) are exported, reject each bad argument
with its documented rc before touching the device, and size their workspace from n and m alone."""
import ctypes
import os

import pytest

from sgn_rast import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


def test_entries_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "sgn_project_bwd_fused_pose") and hasattr(raw, "sgn_project_pose_workspace_bytes")
    assert _lib.SIGNATURES["sgn_project_bwd_fused_pose"][1][-1] is ctypes.c_void_p      # stream last
    assert lib.sgn_version() >= 100


FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: every case below fails its argument check first


def _call(lib, n=1000, m=3, offsets=FAKE, v_poses=FAKE, ws=FAKE, ws_bytes=None, ids=FAKE, poses=FAKE, v_mean=FAKE):
    ws_bytes = lib.sgn_project_pose_workspace_bytes(max(n, 1), max(m, 1)) if ws_bytes is None else ws_bytes
    f = FAKE
    return lib.sgn_project_bwd_fused_pose(n, f, f, 1.0, f, ids, poses, f, 100.0, 100.0, f, f, f, f, f, None, f, None,
                                          v_mean, f, f, 0, 64, 64, m, offsets, v_poses, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,rc,what", [
    (dict(n=-1), -1, b"n >= 0"),
    (dict(m=0), -8, b"m >= 1"),
    (dict(offsets=None), -9, b"object_offsets"),
    (dict(v_poses=None), -9, b"v_poses"),
    (dict(ws=None), -10, b"ws_bytes"),
    (dict(ws_bytes=16), -10, b"ws_bytes"),
    (dict(ws=ctypes.c_void_p(0x1004)), -10, b"ws_bytes"),
    (dict(ids=None, poses=None), -11, b"object_ids"),
    (dict(poses=None), -6, b"object_ids"),
    (dict(ids=None), -6, b"object_ids"),
    (dict(v_mean=None), -4, b"v_means_local"),
])
def test_bad_arguments_give_their_documented_rc(lib, kw, rc, what):
    assert _call(lib, **kw) == rc
    assert what in lib.sgn_last_error()


def test_workspace_size(lib):
    assert lib.sgn_project_pose_workspace_bytes(0, 3) == 0
    assert lib.sgn_project_pose_workspace_bytes(-5, 3) == 0
    assert lib.sgn_project_pose_workspace_bytes(100, 0) == 0
    # one 64-byte partial per wave and object, plus 64 second-level partials per object
    assert lib.sgn_project_pose_workspace_bytes(64, 1) == (1 + 1 + 64) * 64
    assert lib.sgn_project_pose_workspace_bytes(65, 9) == (2 + 9 + 9 * 64) * 64
    assert lib.sgn_project_pose_workspace_bytes(1 << 20, 9) == ((1 << 14) + 9 + 9 * 64) * 64

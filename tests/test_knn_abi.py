"""CPU: the k-nearest-neighbour entry points (include/sgn_rast.h, csrc/knn.hip) are exported, reject bad arguments
with rc < 0 and a message before touching the device, and size their workspace from n and k alone."""
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
    assert hasattr(raw, "sgn_knn") and hasattr(raw, "sgn_knn_workspace_bytes")
    assert _lib.SIGNATURES["sgn_knn"][1][-1] is ctypes.c_void_p      # stream last


def _call(lib, n, k, points=1, ws_bytes=None):
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: every case below fails its argument check first
    ws = lib.sgn_knn_workspace_bytes(max(n, 1), max(k, 1)) if ws_bytes is None else ws_bytes
    return lib.sgn_knn(n, k, fake if points else None, fake, fake, None, fake, ws, None)


@pytest.mark.parametrize("n,k,points,what", [(100, 0, 1, b"k >= 1"), (100, 17, 1, b"k <= 16"),
                                             (3, 3, 1, b"n > k"), (1, 1, 1, b"n > k"), (0, 1, 1, b"n > k"),
                                             (100, 3, 0, b"points")])
def test_bad_arguments_give_negative_rc_and_a_message(lib, n, k, points, what):
    rc = _call(lib, n, k, points)
    assert rc < 0
    assert what in lib.sgn_last_error()


def test_short_workspace_is_refused(lib):
    need = lib.sgn_knn_workspace_bytes(1000, 3)
    rc = _call(lib, 1000, 3, ws_bytes=need - 1)
    assert rc < 0 and b"ws_bytes" in lib.sgn_last_error()


def test_workspace_size_is_monotone_in_n(lib):
    sizes = [lib.sgn_knn_workspace_bytes(n, 3) for n in (2, 63, 64, 65, 1000, 4096, 100_000, 1 << 20, 1 << 22)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] >= (1 << 22) * 40                               # keys, ids, sorted points
    assert lib.sgn_knn_workspace_bytes(1000, 1) == lib.sgn_knn_workspace_bytes(1000, 16)
    assert lib.sgn_knn_workspace_bytes(0, 3) == 0

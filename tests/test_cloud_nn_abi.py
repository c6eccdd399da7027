"""CPU: the two-cloud nearest-neighbour entry points (include/sgn_rast.h, csrc/cloud_nn.hip) are exported, reject bad
arguments with rc < 0 and a message before touching the device, and size their workspace from the two counts alone."""
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
    assert hasattr(raw, "sgn_cloud_nn") and hasattr(raw, "sgn_cloud_nn_workspace_bytes")
    assert _lib.SIGNATURES["sgn_cloud_nn"][1][-1] is ctypes.c_void_p      # stream last
    assert len(_lib.SIGNATURES["sgn_cloud_nn"][1]) == 10 and len(_lib.SIGNATURES["sgn_cloud_nn_workspace_bytes"][1]) == 2


def _call(lib, nt, nq, target=1, query=1, dist=1, ws=1, ws_bytes=None):
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: every case below fails its argument check first
    need = lib.sgn_cloud_nn_workspace_bytes(max(nt, 1), max(nq, 1)) if ws_bytes is None else ws_bytes
    return lib.sgn_cloud_nn(nt, fake if target else None, nq, fake if query else None, fake if dist else None, None,
                            None, fake if ws else None, need, None)


@pytest.mark.parametrize("nt,nq,what", [(0, 100, b"n_target >= 1"), (-5, 100, b"n_target >= 1"),
                                        ((1 << 30) + 1, 100, b"n_target"), (100, 0, b"n_query >= 1"),
                                        (100, -1, b"n_query >= 1"), (100, (1 << 30) + 1, b"n_query")])
def test_bad_sizes_give_negative_rc_and_a_message(lib, nt, nq, what):
    fake = ctypes.c_void_p(0x1000)
    rc = lib.sgn_cloud_nn(nt, fake, nq, fake, fake, None, None, fake, 1 << 40, None)
    assert rc < 0
    assert what in lib.sgn_last_error()


@pytest.mark.parametrize("missing", ["target", "query", "dist", "ws"])
def test_null_pointers_are_refused(lib, missing):
    rc = _call(lib, 100, 200, **{missing: 0})
    assert rc < 0 and missing.encode() in lib.sgn_last_error()


def test_short_workspace_is_refused(lib):
    need = lib.sgn_cloud_nn_workspace_bytes(1000, 3000)
    rc = _call(lib, 1000, 3000, ws_bytes=need - 1)
    assert rc < 0 and b"ws_bytes" in lib.sgn_last_error()


def test_workspace_size_is_monotone_in_both_counts(lib):
    ns = (1, 63, 64, 65, 1000, 4096, 100_000, 1 << 20, 1 << 22)
    for fixed in (1, 1000, 1 << 20):
        by_target = [lib.sgn_cloud_nn_workspace_bytes(n, fixed) for n in ns]
        by_query = [lib.sgn_cloud_nn_workspace_bytes(fixed, n) for n in ns]
        assert all(a <= b for a, b in zip(by_target, by_target[1:])), by_target
        assert all(a <= b for a, b in zip(by_query, by_query[1:])), by_query
        assert by_target[0] > 0 and by_query[0] > 0
    # the target's tree (what sgn_knn needs for it) plus keys and ids of the queries, in and out
    assert lib.sgn_cloud_nn_workspace_bytes(1 << 20, 1 << 22) >= lib.sgn_knn_workspace_bytes(1 << 20, 1) + (1 << 22) * 24
    for bad in ((0, 10), (10, 0), (-1, 10), ((1 << 30) + 1, 10), (10, (1 << 30) + 1)):
        assert lib.sgn_cloud_nn_workspace_bytes(*bad) == 0
    assert lib.sgn_cloud_nn_workspace_bytes(1 << 30, 1 << 30) > (1 << 30) * 64

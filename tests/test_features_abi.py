"""CPU: the feature rasterizer's and the semantic cross-entropy's C entry points exist, bind through ctypes with the
header's argument counts, and report argument errors before any launch (no GPU needed; the non-NULL "pointers" below are
never dereferenced: every call returns at its argument checks)."""
import ctypes

import test_abi as TA
from sgn_rast import features as F  # noqa: F401  (the module under test: without it nothing here runs)

NAMES = ("sgn_raster_features_workspace_bytes", "sgn_raster_features_fwd", "sgn_raster_features_bwd",
         "sgn_semantic_ce_workspace_bytes", "sgn_semantic_ce_fwd", "sgn_semantic_ce_bwd")
P = 1          # a non-NULL pointer


def _lib():
    from sgn_rast import _lib
    return _lib.load()


def _fwd(lib, bw=16, n=4, K=5, n_isect=1, ids=P, bins=P, xys=P, conics=P, feats=P, opac=P, out=P, Ts=P, idx=P, ws=P,
         ws_bytes=None, opts=None):
    ws_bytes = lib.sgn_raster_features_workspace_bytes(n) if ws_bytes is None else ws_bytes
    return lib.sgn_raster_features_fwd(32, 32, bw, n, K, n_isect, ids, bins, xys, conics, feats, opac, 0, None, out, Ts,
                                       idx, ws, ws_bytes, opts, None)


def _bwd(lib, bw=16, n=4, K=5, n_isect=1, ids=P, bins=P, xys=P, conics=P, feats=P, opac=P, Ts=P, idx=P, v_xy=P,
         v_conic=P, v_feats=P, v_opac=P, ws=P, ws_bytes=None, clamp=0.99):
    ws_bytes = lib.sgn_raster_features_workspace_bytes(n) if ws_bytes is None else ws_bytes
    return lib.sgn_raster_features_bwd(32, 32, bw, n, K, n_isect, ids, bins, xys, conics, feats, opac, 0, None, Ts, idx,
                                       None, None, clamp, v_xy, v_conic, v_feats, v_opac, ws, ws_bytes, None, None)


def test_feature_entries_are_declared_exported_and_bound():
    from sgn_rast import _lib
    fns = TA._header_functions()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in fns and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == fns[name], name
        assert hasattr(raw, name), name
        want = ctypes.c_size_t if name.endswith("workspace_bytes") else ctypes.c_int
        assert getattr(lib, name).restype is want, name
    assert lib.sgn_raster_features_workspace_bytes(1000) >= 1000 * 32
    assert lib.sgn_semantic_ce_workspace_bytes() >= 12


def test_channel_count_and_tile_width_are_checked_first():
    lib = _lib()
    for call in (_fwd, _bwd):
        assert call(lib, K=0) == -13 and call(lib, K=65) == -13 and call(lib, K=-3) == -13
        assert b"n_channels" in lib.sgn_last_error()
        assert call(lib, bw=8) == -12 and b"block_width" in lib.sgn_last_error()     # 16x16 tiles only, the usual code
        assert call(lib, bw=8, K=0) == -12
        assert call(lib, n_isect=-1) == -3 and call(lib, n_isect=1 << 31) == -3


def test_null_pointers_are_refused():
    lib = _lib()
    for arg in ("out", "Ts", "idx"):
        assert _fwd(lib, **{arg: None}) == -4, arg
    for arg in ("ids", "bins", "xys", "conics", "feats", "opac", "ws"):
        assert _fwd(lib, **{arg: None}) == -5, arg
    for arg in ("v_xy", "v_conic", "v_feats", "v_opac", "conics", "opac", "ws"):
        assert _bwd(lib, **{arg: None}) == -4, arg
    for arg in ("ids", "bins", "xys", "feats", "Ts", "idx"):
        assert _bwd(lib, **{arg: None}) == -5, arg


def test_short_workspace_and_bad_clamp_are_refused():
    lib = _lib()
    need = lib.sgn_raster_features_workspace_bytes(4)
    assert _fwd(lib, ws_bytes=need - 1) == -6 and _bwd(lib, ws_bytes=need - 1) == -6
    assert _fwd(lib, ws_bytes=0) == -6 and _bwd(lib, ws_bytes=0) == -6
    assert _bwd(lib, clamp=0.0) == -7 and _bwd(lib, clamp=1.0) == -7
    assert _bwd(lib, n=0, ws=None, ws_bytes=0) == 0                      # nothing to do: returns before any launch


def test_semantic_entries_check_their_arguments():
    lib = _lib()
    fwd = lambda h=8, w=8, K=4, logits=P, labels=P, ignore=-1, loss=P, ws=P, ws_bytes=16: lib.sgn_semantic_ce_fwd(
        h, w, K, logits, labels, ignore, None, loss, ws, ws_bytes, None)
    bwd = lambda h=8, w=8, K=4, logits=P, labels=P, ignore=-1, v_loss=P, ws=P, ws_bytes=16, v_logits=P: \
        lib.sgn_semantic_ce_bwd(h, w, K, logits, labels, ignore, None, v_loss, ws, ws_bytes, v_logits, None)
    for call in (fwd, bwd):
        assert call(h=0) == -1
        assert call(K=0) == -2 and call(K=65) == -2
        assert call(ignore=-2) == -3 and call(ignore=256) == -3
        assert call(logits=None) == -4 and call(labels=None) == -4 and call(ws=None) == -4
        assert call(ws_bytes=8) == -5
    assert fwd(loss=None) == -4 and bwd(v_loss=None) == -4 and bwd(v_logits=None) == -4

"""CPU: the layered evaluation forward's C entry points exist, bind through ctypes with the header's argument counts,
and report argument errors before any launch (no GPU needed)."""
import ctypes

import test_abi as TA


def test_layer_entries_are_declared_exported_and_bound():
    from sgn_rast import _lib
    fns = TA._header_functions()
    lib = _lib.load()
    for name in ("sgn_raster_layers_fwd", "sgn_layers_finish"):
        assert name in fns and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == fns[name], name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert getattr(lib, name).restype is ctypes.c_int


def test_layer_entries_check_their_arguments_without_a_gpu():
    from sgn_rast import _lib
    lib = _lib.load()
    call = lambda bw, n, split, own_ids=None: lib.sgn_raster_layers_fwd(
        32, 32, bw, n, 0, None, 1, None, None, None, None, 1, 1, None, split, own_ids, None, 1, 1, 1, 1, n * 48, 0, None,
        None, None)
    assert call(8, 4, 2) == -12 and b"block_width" in lib.sgn_last_error()       # 16x16 tiles only, the usual code
    assert call(16, 4, 5) == -14 and call(16, 4, -1) == -14                       # split outside [0, n]
    assert call(16, 4, 2, own_ids=1) == -15                                       # own list: ids and bins, or neither
    assert lib.sgn_layers_finish(0, 8, 1, 1, 1, None, 1, 1, 1, None) == -1
    assert lib.sgn_layers_finish(8, 8, 1, 1, None, None, 1, 1, 1, None) == -2

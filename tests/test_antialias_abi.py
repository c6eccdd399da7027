"""CPU: the antialiased mode's kernel pair (`csrc/antialias.hip`) is declared in the header, exported, bound through
ctypes with the header's argument counts, and reports argument errors before any launch (no GPU needed; the non-NULL
"pointers" below are never dereferenced: every call returns at its argument checks)."""
import ctypes

import test_abi as TA

NAMES = ("sgn_aa_opacity_fwd", "sgn_aa_opacity_bwd")
P = 1          # a non-NULL pointer


def _lib():
    from sgn_rast import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_bound():
    from sgn_rast import _lib
    fns = TA._header_functions()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (5, 7)):
        assert name in fns and name in _lib.SIGNATURES, name
        assert fns[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).restype is ctypes.c_int, name


def test_nothing_to_do_returns_before_any_launch():
    lib = _lib()
    assert lib.sgn_aa_opacity_fwd(0, None, None, None, None) == 0
    assert lib.sgn_aa_opacity_bwd(0, None, None, None, None, None, None) == 0
    assert lib.sgn_aa_opacity_bwd(5, P, P, P, None, None, None) == 0           # neither gradient is wanted


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    assert lib.sgn_aa_opacity_fwd(-1, P, P, P, None) < 0 and b"sgn_aa_opacity_fwd" in lib.sgn_last_error()
    assert lib.sgn_aa_opacity_bwd(-1, P, P, P, P, P, None) < 0 and b"sgn_aa_opacity_bwd" in lib.sgn_last_error()
    for k in range(3):
        args = [P, P, P]
        args[k] = None
        assert lib.sgn_aa_opacity_fwd(4, *args, None) < 0, k
        assert b"sgn_aa_opacity_fwd" in lib.sgn_last_error()
        for outs in ((P, P), (P, None), (None, P), (None, None)):
            assert lib.sgn_aa_opacity_bwd(4, *args, *outs, None) < 0, (k, outs)
            assert b"sgn_aa_opacity_bwd" in lib.sgn_last_error()

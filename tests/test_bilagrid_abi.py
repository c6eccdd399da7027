"""CPU: the bilateral-grid pair (`csrc/bilagrid.hip`) is declared in the header, exported, bound through ctypes with the
header's argument counts, and reports argument errors before any launch (no GPU needed; the non-NULL "pointers" below
are never dereferenced: every call returns at its argument checks).  The Python surface raises its ``ValueError``s
before it looks at the device, and ``train_step(appearance=...)`` insists on ``gt`` before it renders."""
import ctypes

import pytest
import torch

import test_abi as TA

NAMES = ("sgn_bilagrid_slice_fwd", "sgn_bilagrid_slice_bwd")
P = 64         # a non-NULL, 16-byte aligned pointer


def _lib():
    from sgn_rast import _lib
    return _lib.load()


def _fwd(lib, L=8, Hg=16, Wg=16, grid=P, H=4, W=4, n_pix=16, rgb=P, out=P):
    return lib.sgn_bilagrid_slice_fwd(L, Hg, Wg, grid, H, W, n_pix, rgb, out, None)


def _bwd(lib, L=8, Hg=16, Wg=16, grid=P, H=4, W=4, n_pix=16, rgb=P, v_out=P, v_rgb=P, v_grid=P):
    return lib.sgn_bilagrid_slice_bwd(L, Hg, Wg, grid, H, W, n_pix, rgb, v_out, v_rgb, v_grid, None)


def test_entries_are_declared_exported_and_bound():
    from sgn_rast import _lib
    fns = TA._header_functions()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (10, 12)):
        assert name in fns and name in _lib.SIGNATURES, name
        assert fns[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).restype is ctypes.c_int, name


def test_nothing_to_do_returns_before_any_launch():
    lib = _lib()
    assert _fwd(lib, n_pix=0, grid=None, rgb=None, out=None) == 0                 # n_pix == 0 is not an error
    assert _bwd(lib, n_pix=0, grid=None, rgb=None, v_out=None, v_rgb=None, v_grid=None) == 0
    assert _bwd(lib, v_rgb=None, v_grid=None) == 0                                # neither gradient is wanted


@pytest.mark.parametrize("call, name", [(_fwd, b"sgn_bilagrid_slice_fwd"), (_bwd, b"sgn_bilagrid_slice_bwd")])
def test_bad_arguments_are_refused_with_a_message(call, name):
    lib = _lib()

    def refused(rc, code):
        assert rc == code, (rc, code)
        assert name in lib.sgn_last_error()

    for dim in ("L", "Hg", "Wg", "H", "W"):
        for bad in (0, -3):
            refused(call(lib, **{dim: bad}), -1)
    refused(call(lib, H=16385, n_pix=1), -1)
    refused(call(lib, n_pix=-1), -1)
    refused(call(lib, n_pix=17), -1)                                              # more than H * W
    refused(call(lib, L=1 << 10, Hg=1 << 10, Wg=1 << 10), -1)                     # 32-bit cell offsets
    refused(call(lib, L=0, grid=None), -1)                                        # sizes are judged before pointers
    for ptr in ("grid", "rgb", "out" if call is _fwd else "v_out"):
        refused(call(lib, **{ptr: None}), -2)
    refused(call(lib, grid=P + 4), -3)                                            # cells are read 16 bytes at a time
    if call is _bwd:                                                              # one gradient alone is a valid request:
        refused(call(lib, v_grid=None, rgb=None), -2)                             # ... the other checks still hold


def test_python_surface_raises_before_any_launch():
    from sgn_rast import _lib, appearance
    g = torch.zeros(2, 2, 3, 4, 12)            # CPU tensors: a launch would raise SgnRastError, not ValueError
    rgb = torch.zeros(5, 6, 3)
    with pytest.raises(ValueError, match=r"grids must be \[num"):
        appearance.slice_image(torch.zeros(2, 3, 4, 12), 0, rgb)
    with pytest.raises(ValueError, match=r"grids must be \[num"):
        appearance.slice_image(torch.zeros(2, 2, 3, 4, 9), 0, rgb)
    with pytest.raises(ValueError, match="grids must be float32"):
        appearance.slice_image(g.double(), 0, rgb)
    with pytest.raises(ValueError, match=r"rgb must be \[H, W, 3\]"):
        appearance.slice_image(g, 0, torch.zeros(5, 6, 4))
    with pytest.raises(ValueError, match=r"rgb must be \[H, W, 3\]"):
        appearance.slice_image(g, 0, torch.zeros(1, 5, 6, 3))
    with pytest.raises(ValueError, match="rgb must be float32"):
        appearance.slice_image(g, 0, rgb.half())
    for bad in (2, -1):
        with pytest.raises(ValueError, match="out of range"):
            appearance.slice_image(g, bad, rgb)
    with pytest.raises(ValueError, match="Python int"):
        appearance.slice_image(g, 0.0, rgb)
    with pytest.raises(ValueError, match="grids must be"):
        appearance.total_variation(torch.zeros(2, 3, 4, 12))
    with pytest.raises(ValueError):
        appearance.BilateralGrids(0)
    with pytest.raises(ValueError):
        appearance.BilateralGrids(2, (4, 0, 2))
    with pytest.raises(ValueError):
        appearance.BilateralGrids.from_channel_major(torch.zeros(2, 2, 3, 4, 12))
    # well-formed CPU tensors fail loudly, as everywhere in the package: there is no fallback
    with pytest.raises(_lib.SgnRastError):
        appearance.slice_image(g, 0, rgb)
    with pytest.raises(_lib.SgnRastError):
        appearance.BilateralGrids(2, (4, 3, 2))(1, rgb)


def test_package_exports_the_surface():
    import sgn_rast
    from sgn_rast import appearance
    assert sgn_rast.BilateralGrids is appearance.BilateralGrids
    assert sgn_rast.slice_image is appearance.slice_image and sgn_rast.total_variation is appearance.total_variation


def test_train_step_appearance_needs_gt_and_a_wellformed_pair():
    from sgn_rast import appearance, step
    grids = appearance.BilateralGrids(2, (2, 2, 2))
    with pytest.raises(ValueError, match="pass gt as well"):       # before the render: nothing else is even looked at
        step.train_step({}, None, None, None, fused=True, appearance=(grids, 0))
    gt = torch.zeros(8, 8, 3)
    with pytest.raises(ValueError, match="appearance must be"):
        step.train_step({}, None, None, None, fused=True, gt=gt, appearance=(grids, 2))
    with pytest.raises(ValueError, match="appearance must be"):
        step.train_step({}, None, None, None, fused=True, gt=gt, appearance=(torch.zeros(2, 2, 2, 12), 0))

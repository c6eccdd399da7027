"""CPU: the byte-ground-truth L1 + SSIM entry points (include/sgn_rast.h, "The same loss with the ground truth as the
data set caches it") are exported and in the ctypes table, reject each bad argument with the masked entries' return codes
before touching the device, and share the masked entries' workspace.  Also the arithmetic fact the byte contract rests
on: u / 255 and u * (1 / 255) are different fp32 numbers for 126 of the 256 byte values."""
import ctypes
import os

import numpy as np
import pytest
import torch

from sgn_rast import _lib

NAMES = ("sgn_l1_ssim_gt8_fwd", "sgn_l1_ssim_gt8_bwd")
F = ctypes.c_void_p(0x1000)      # never dereferenced: every case below fails its argument check first


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


def test_entries_are_exported_and_declared(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    # the masked entries' arguments, gt as bytes
    assert _lib.SIGNATURES["sgn_l1_ssim_gt8_fwd"] == _lib.SIGNATURES["sgn_l1_ssim_masked_fwd"]
    assert _lib.SIGNATURES["sgn_l1_ssim_gt8_bwd"] == _lib.SIGNATURES["sgn_l1_ssim_masked_bwd"]
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sgn_rast.h")).read()
    for name in NAMES:
        assert f"int {name}(int h, int w, const float *pred, const unsigned char *gt, const unsigned char *mask," in header


def _fwd(lib, h=64, w=64, pred=F, gt=F, mask=F, out4=F, with_grad=1, ws=F, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sgn_l1_ssim_masked_workspace_bytes(h, w, with_grad)
    return lib.sgn_l1_ssim_gt8_fwd(h, w, pred, gt, mask, 1.0, float("inf"), 0.2, out4, with_grad, ws, ws_bytes, None)


def _bwd(lib, h=64, w=64, pred=F, gt=F, mask=F, ws=F, gscale=F, v_pred=F):
    return lib.sgn_l1_ssim_gt8_bwd(h, w, pred, gt, mask, 1.0, ws, gscale, v_pred, None)


def test_forward_argument_errors(lib):
    for h, w in ((10, 64), (64, 10), (0, 0), (-5, 64)):
        assert _fwd(lib, h=h, w=w) == -1
        assert b"sgn_l1_ssim_gt8_fwd" in lib.sgn_last_error()
    for kw in (dict(pred=None), dict(gt=None), dict(out4=None), dict(ws=None)):
        assert _fwd(lib, **kw) == -2, kw
    assert _fwd(lib, mask=None, pred=None) == -2              # a NULL mask is legal, it is not what is reported
    need = lib.sgn_l1_ssim_masked_workspace_bytes(64, 64, 1)
    assert _fwd(lib, ws_bytes=need - 1) == -3 and b"ws_bytes" in lib.sgn_last_error()
    # the workspace is the masked one (three floats per workgroup), not the unmasked one (two): at 1280 x 1920 the
    # unmasked size is short by one 256-byte unit of partials ...
    assert _fwd(lib, h=1280, w=1920, ws_bytes=lib.sgn_l1_ssim_workspace_bytes(1280, 1920, 1)) == -3
    assert _fwd(lib, with_grad=1, ws_bytes=lib.sgn_l1_ssim_masked_workspace_bytes(64, 64, 0)) == -3


def test_backward_argument_errors(lib):
    for h, w in ((10, 64), (64, 10)):
        assert _bwd(lib, h=h, w=w) == -1
        assert b"sgn_l1_ssim_gt8_bwd" in lib.sgn_last_error()
    for kw in (dict(pred=None), dict(gt=None), dict(ws=None), dict(gscale=None), dict(v_pred=None)):
        assert _bwd(lib, **kw) == -2, kw
    assert _bwd(lib, mask=None, gt=None) == -2


def test_workspace_is_the_masked_one(lib):
    """No size function of its own: the smallest workspace the forward accepts is exactly the masked entries'."""
    for h, w in ((11, 11), (64, 64), (37, 53), (1280, 1920)):
        for with_grad in (0, 1):
            need = lib.sgn_l1_ssim_masked_workspace_bytes(h, w, with_grad)
            assert _fwd(lib, h=h, w=w, with_grad=with_grad, ws_bytes=need - 1) == -3
            assert _fwd(lib, h=h, w=w, with_grad=with_grad, ws_bytes=need, pred=None) == -2    # past the size check
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "sgn_l1_ssim_gt8_workspace_bytes")


def test_quotient_is_not_the_reciprocal_product():
    """Why the kernels divide: the cached value is astype(float32) / 255.0, and multiplying by the fp32 reciprocal
    gives another number for 126 of the 256 bytes (one unit in the last place each)."""
    u = np.arange(256, dtype=np.float32)
    q, p = u / np.float32(255.0), u * (np.float32(1.0) / np.float32(255.0))
    assert int((q != p).sum()) == 126
    assert np.array_equal(q, (torch.arange(256, dtype=torch.uint8).float() / 255.0).numpy())
    exact = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)          # fp64 quotient rounded once more ...
    assert np.array_equal(q, exact)                                                # ... agrees: q is the correctly rounded one


# ------------------------------------------------------------------------------------------------ host-side errors
H, W = 24, 32


def test_integer_pred_is_a_type_error_before_the_device_check():
    from sgn_rast import loss
    g = torch.Generator().manual_seed(0)
    gt8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
    gtf = gt8.float() / 255.0
    m = torch.ones(H, W, dtype=torch.bool)
    assert not issubclass(_lib.SgnRastError, TypeError)
    for pred in (gt8, gt8.to(torch.int32), gt8.bool()):
        for gt in (gt8, gtf):
            for mask in (None, m):
                with pytest.raises(TypeError, match="pred"):
                    loss.l1_ssim(pred, gt, mask=mask)
                with pytest.raises(TypeError, match="pred"):
                    loss.photometric_loss(pred, gt, 0.2, clamp_max=1.0, mask=mask)
                with pytest.raises(TypeError, match="pred"):
                    loss.image_metrics(pred, gt, mask=mask)


def test_a_byte_gt_on_cpu_tensors_reaches_the_device_check():
    """No quiet CPU path for the new dtype either; a bad mask is still reported first."""
    from sgn_rast import loss
    g = torch.Generator().manual_seed(0)
    gt8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
    pred = torch.rand(H, W, 3, generator=g)
    for mask in (None, torch.ones(H, W, dtype=torch.bool)):
        with pytest.raises(_lib.SgnRastError):
            loss.l1_ssim(pred, gt8, mask=mask)
        with pytest.raises(_lib.SgnRastError):
            loss.photometric_loss(pred, gt8, mask=mask)
        with pytest.raises(_lib.SgnRastError):
            loss.image_metrics(pred, gt8, mask=mask)
    with pytest.raises(TypeError):
        loss.l1_ssim(pred, gt8, mask=torch.ones(H, W))

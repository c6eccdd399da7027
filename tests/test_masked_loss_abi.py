"""CPU: the masked L1 + SSIM entry points (include/sgn_rast.h, "The same loss under the batch's pixel mask") are
exported and in the ctypes table, reject each bad argument with its documented rc before touching the device, and
the Python layer raises its host-side TypeError / ValueError for a bad mask before the "no fallback" device check."""
import ctypes
import os

import pytest
import torch

from sgn_rast import _lib

NAMES = ("sgn_l1_ssim_masked_workspace_bytes", "sgn_l1_ssim_masked_fwd", "sgn_l1_ssim_masked_bwd")
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
    # one argument (the mask) more than the unmasked entries, in front of data_range / clamp_max
    assert len(_lib.SIGNATURES["sgn_l1_ssim_masked_fwd"][1]) == len(_lib.SIGNATURES["sgn_l1_ssim_fwd"][1]) + 1
    assert len(_lib.SIGNATURES["sgn_l1_ssim_masked_bwd"][1]) == len(_lib.SIGNATURES["sgn_l1_ssim_bwd"][1]) + 1
    assert _lib.SIGNATURES["sgn_l1_ssim_masked_workspace_bytes"][0] is ctypes.c_size_t


def _fwd(lib, h=64, w=64, pred=F, gt=F, mask=F, out4=F, with_grad=1, ws=F, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sgn_l1_ssim_masked_workspace_bytes(h, w, with_grad)
    return lib.sgn_l1_ssim_masked_fwd(h, w, pred, gt, mask, 1.0, float("inf"), 0.2, out4, with_grad, ws, ws_bytes, None)


def _bwd(lib, h=64, w=64, pred=F, gt=F, mask=F, ws=F, gscale=F, v_pred=F):
    return lib.sgn_l1_ssim_masked_bwd(h, w, pred, gt, mask, 1.0, ws, gscale, v_pred, None)


def test_forward_argument_errors(lib):
    for h, w in ((10, 64), (64, 10), (0, 0), (-5, 64)):
        assert _fwd(lib, h=h, w=w) == -1
        assert b"sgn_l1_ssim_masked_fwd" in lib.sgn_last_error()
    for kw in (dict(pred=None), dict(gt=None), dict(out4=None), dict(ws=None)):
        assert _fwd(lib, **kw) == -2, kw
    assert _fwd(lib, mask=None, pred=None) == -2              # a NULL mask is legal, it is not what is reported
    need = lib.sgn_l1_ssim_masked_workspace_bytes(64, 64, 1)
    assert _fwd(lib, ws_bytes=need - 1) == -3 and b"ws_bytes" in lib.sgn_last_error()
    assert _fwd(lib, with_grad=1, ws_bytes=lib.sgn_l1_ssim_masked_workspace_bytes(64, 64, 0)) == -3


def test_backward_argument_errors(lib):
    for h, w in ((10, 64), (64, 10)):
        assert _bwd(lib, h=h, w=w) == -1
        assert b"sgn_l1_ssim_masked_bwd" in lib.sgn_last_error()
    for kw in (dict(pred=None), dict(gt=None), dict(ws=None), dict(gscale=None), dict(v_pred=None)):
        assert _bwd(lib, **kw) == -2, kw


def test_workspace_size(lib):
    wsb = lib.sgn_l1_ssim_masked_workspace_bytes
    assert wsb(10, 64, 1) == 256 and wsb(64, 10, 0) == 256          # too small an image: the floor, as the unmasked one
    blocks = 4 * 4                                                  # 64 x 64 in 16 x 16 tiles
    partials = ((blocks * 3 * 4 + 255) // 256) * 256                # three floats per workgroup: L1, SSIM, squared error
    assert wsb(64, 64, 0) == partials
    assert wsb(64, 64, 1) == partials + 9 * 54 * 54 * 4             # + the same nine maps as the unmasked workspace
    assert wsb(64, 64, 1) - wsb(64, 64, 0) == (lib.sgn_l1_ssim_workspace_bytes(64, 64, 1)
                                               - lib.sgn_l1_ssim_workspace_bytes(64, 64, 0))


# ------------------------------------------------------------------------------------------------ host-side errors
H, W = 24, 32


def _imgs():
    g = torch.Generator().manual_seed(0)
    return torch.rand(H, W, 3, generator=g), torch.rand(H, W, 3, generator=g)


BAD_MASKS = [
    (lambda: torch.ones(H, W), TypeError),                                   # a float image would be a weight map
    (lambda: torch.ones(H, W, 1, dtype=torch.float64), TypeError),
    (lambda: torch.ones(H, W, dtype=torch.int64), TypeError),
    (lambda: torch.ones(H, W - 1, dtype=torch.bool), ValueError),
    (lambda: torch.ones(H + 1, W, 1, dtype=torch.uint8), ValueError),
    (lambda: torch.ones(H * W * 3, dtype=torch.bool), ValueError),
]


@pytest.mark.parametrize("make,exc", BAD_MASKS)
def test_loss_functions_reject_a_bad_mask_before_the_device_check(make, exc):
    """CPU tensors: any launch (and the device check in front of it) would raise SgnRastError; the mask's own error
    must come first."""
    from sgn_rast import loss
    pred, gt = _imgs()
    assert not issubclass(_lib.SgnRastError, (TypeError, ValueError))
    with pytest.raises(exc):
        loss.l1_ssim(pred, gt, mask=make())
    with pytest.raises(exc):
        loss.photometric_loss(pred, gt, 0.2, clamp_max=1.0, mask=make())
    with pytest.raises(exc):
        loss.image_metrics(pred, gt, mask=make())


def test_a_good_mask_on_cpu_tensors_reaches_the_device_check():
    from sgn_rast import loss
    pred, gt = _imgs()
    for m in (torch.ones(H, W, dtype=torch.bool), torch.ones(H, W, 1, dtype=torch.uint8)):
        with pytest.raises(_lib.SgnRastError):
            loss.l1_ssim(pred, gt, mask=m)
        with pytest.raises(_lib.SgnRastError):
            loss.image_metrics(pred, gt, mask=m)
    with pytest.raises(_lib.SgnRastError):
        loss.image_metrics(pred, gt)


def _scene(n=10):
    from sgn_rast import scenes
    return scenes.make_scene("c1", n_override=n)


def test_train_step_rejects_a_bad_mask_before_rendering():
    from sgn_rast import step
    cam, raw = _scene()
    P = step.leaf_params(raw)
    w_img, w_a = step.loss_weights(cam)
    gt = torch.zeros(cam.height, cam.width, 3)
    ok = torch.ones(cam.height, cam.width, dtype=torch.bool)
    for bad, exc in ((ok.float(), TypeError), (ok[:, :-1], ValueError), (ok[None], ValueError)):
        for fused in (False, True):
            with pytest.raises(exc):
                step.train_step(P, cam, w_img, w_a, gt=gt, mask=bad, fused=fused)
    with pytest.raises(ValueError, match="gt"):
        step.train_step(P, cam, w_img, w_a, mask=ok)


def test_train_step_views_checks_masks_on_the_host():
    from sgn_rast import views
    cam, P = _scene()
    gts = [torch.zeros(cam.height, cam.width, 3)] * 2
    ok = torch.ones(cam.height, cam.width, dtype=torch.bool)
    with pytest.raises(ValueError, match="masks"):
        views.train_step_views(P, [cam, cam], gts, masks=[ok])
    with pytest.raises(ValueError, match="masks"):
        views.train_step_views(P, [cam, cam], gts, masks=[ok, None, None])
    with pytest.raises(TypeError):
        views.train_step_views(P, [cam, cam], gts, masks=[None, ok.float()])
    with pytest.raises(ValueError):
        views.train_step_views(P, [cam, cam], gts, masks=[ok[:-1], None])

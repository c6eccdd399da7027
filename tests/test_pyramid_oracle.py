"""CPU: the numpy restatement of the pyramid kernel's contract (tests/pyramid_oracle.py) against the reference's own
operation — ``F.interpolate(x, size, mode="bilinear", align_corners=False, antialias=False)`` on ``x = img.float() / 255``
(what ``TF.resize(..., antialias=None)`` runs) and ``mode="nearest"`` for the byte maps — and the host pieces of
``sgn_rast.pyramid`` (schedule, level size, scaled camera) against the reference's expressions.

Tolerance of the bilinear comparison, derived, not measured: ``1e-6 + 8 * 2**-23 * max(H, W)``.
* ``1e-6``: each implementation makes at most 7 roundings of values <= 1 (the quotient, four products, ... the final
  sum), 2**-24 each; twice.
* second term: the two may round the source coordinate differently — at most 3 roundings at magnitude <= max(H, W) per
  axis (scale, product, subtraction), each 2**-24 relative — which moves the weight by that much, and neighbouring taps
  differ by at most 1.
Where ``d`` divides both sides the scale and every source coordinate are exact in fp32 and ``1e-6`` alone holds."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pyramid_oracle as PO

SIZES = [(64, 96), (37, 53), (5, 7), (2, 2), (1, 9), (886, 1918), (1279, 1917), (1280, 1920)]
DS = [2, 4, 8]


def tolerance(h, w, d):
    exact = h % d == 0 and w % d == 0
    return 1e-6 if exact else 1e-6 + 8 * 2.0 ** -23 * max(h, w)


def torch_reference(img: torch.Tensor, byte_map: torch.Tensor, oh: int, ow: int):
    """(bilinear image [oh,ow,3] float32, nearest map [oh,ow] uint8) of CPU tensors, as the reference resizes them."""
    x = (img.float() / 255.0).permute(2, 0, 1)[None]
    y = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)
    n = F.interpolate(byte_map[None, None], size=(oh, ow), mode="nearest")
    return y[0].permute(1, 2, 0).contiguous(), n[0, 0].contiguous()


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_against_interpolate(h, w, d):
    from sgn_rast import pyramid
    g = torch.Generator().manual_seed(h * 10000 + w * 10 + d)
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g)
    sem = torch.randint(0, 256, (h, w), dtype=torch.uint8, generator=g)
    oh, ow = pyramid.level_size(h, w, d)
    ref_img, ref_sem = torch_reference(img, sem, oh, ow)
    got_img, got_sem = PO.image(img.numpy(), oh, ow), PO.nearest(sem.numpy(), oh, ow)
    assert got_img.shape == (oh, ow, 3) and got_img.dtype == np.float32
    assert np.array_equal(got_sem, ref_sem.numpy())
    diff = float(np.abs(got_img - ref_img.numpy()).max())
    tol = tolerance(h, w, d)
    print(f"[pyramid oracle] {h}x{w} d={d} -> {oh}x{ow}: max |restatement - interpolate| {diff:.2e} (tolerance {tol:.2e})")
    assert diff <= tol


def test_size_override_against_interpolate():
    """The floor size of the scaled camera on a non-divisible image."""
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (37, 53, 3), dtype=torch.uint8, generator=g)
    sem = torch.randint(0, 20, (37, 53), dtype=torch.uint8, generator=g)
    ref_img, ref_sem = torch_reference(img, sem, 18, 26)
    assert np.array_equal(PO.nearest(sem.numpy(), 18, 26), ref_sem.numpy())
    assert float(np.abs(PO.image(img.numpy(), 18, 26) - ref_img.numpy()).max()) <= tolerance(37, 53, 2)


def test_identity_level_is_the_quotient():
    """oh = h, ow = w: scale 1, every weight (1, 0): the level is u / 255 itself."""
    img = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3).astype(np.uint8)
    assert np.array_equal(PO.image(img, 16, 16), img.astype(np.float32) / np.float32(255.0))
    assert np.array_equal(PO.nearest(img[..., 0], 16, 16), img[..., 0])


# --------------------------------------------------------------------------------------------------- the host pieces
def test_downscale_factor_is_the_reference_expression():
    from sgn_rast import pyramid
    got = [pyramid.downscale_factor(s, 2, 250) for s in (0, 249, 250, 499, 500, 30000)]
    assert got == [4, 4, 2, 2, 1, 1]
    for s in (0, 1, 10 ** 6):
        assert pyramid.downscale_factor(s, 0, 250) == 1
    for nd in range(4):
        for sched in (1, 7, 3000):
            for s in (0, 1, 6, 7, 8, 2999, 3000, 9000, 12345):
                assert pyramid.downscale_factor(s, nd, sched) == 2 ** max(nd - s // sched, 0)
    for bad in ((-1, 2, 250), (0, -1, 250), (0, 2, 0), (0, 2, -3), (1.0, 2, 250), (0, 2.0, 250), (0, 2, 250.0),
                (True, 2, 250), (None, 2, 250)):
        with pytest.raises(ValueError):
            pyramid.downscale_factor(*bad)


def test_level_size_is_ceil():
    from sgn_rast import pyramid
    assert pyramid.level_size(1280, 1920, 1) == (1280, 1920)
    assert pyramid.level_size(1280, 1920, 2) == (640, 960)
    assert pyramid.level_size(1279, 1917, 4) == (320, 480)
    assert pyramid.level_size(37, 53, 2) == (19, 27)
    assert pyramid.level_size(2, 2, 4) == (1, 1)
    assert pyramid.level_size(1, 9, 8) == (1, 2)
    for bad in (0, 3, 6, -2):
        with pytest.raises(ValueError):
            pyramid.level_size(8, 8, bad)
    with pytest.raises(TypeError):
        pyramid.level_size(8, 8, 2.0)


def _stub_cameras():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stubs", "nerfstudio", "cameras", "cameras.py")
    spec = importlib.util.spec_from_file_location("_pyramid_stub_cameras", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Cameras


@pytest.mark.parametrize("width,height", [(1920, 1280), (1917, 1279)])
def test_scaled_camera_is_rescale_output_resolution(width, height):
    from sgn_rast import pyramid, scenes
    Cameras = _stub_cameras()
    cam = scenes.make_camera(width, height, 2000.0, yaw=0.1)
    cam.fy, cam.cx, cam.cy = 1990.5, width / 2.0 - 3.25, height / 2.0 + 1.5
    assert pyramid.scaled_camera(cam, 1) is cam
    for d in (2, 4, 8):
        ref = Cameras(torch.eye(4)[:3], cam.fx, cam.fy, cam.cx, cam.cy, width, height)
        ref.rescale_output_resolution(1 / d)
        got = pyramid.scaled_camera(cam, d)
        assert isinstance(got, scenes.Camera) and got is not cam
        assert (got.width, got.height) == (int(ref.width), int(ref.height)) == (width // d, height // d)
        assert isinstance(got.width, int) and isinstance(got.height, int)
        for k in ("fx", "fy", "cx", "cy"):
            assert getattr(got, k) == float(getattr(ref, k)), k          # a power of two: exact in fp32 and fp64 alike
        assert got.viewmat is cam.viewmat and got.cam_pos is cam.cam_pos
    assert (cam.width, cam.height, cam.fx) == (width, height, 2000.0)   # the input is left alone
    for bad in (0, 3, -4):
        with pytest.raises(ValueError):
            pyramid.scaled_camera(cam, bad)

"""CPU: ``sgn_gt_downscale`` (include/sgn_rast.h, "One pyramid level of a batch's byte ground truth") is exported,
declared and in the ctypes table; it rejects each bad argument with its return code before touching the device; and
``sgn_rast.pyramid.downscale`` raises every host-side ``TypeError`` / ``ValueError`` before the library's device check,
which CPU tensors then fail (no quiet CPU path)."""
import ctypes
import os

import pytest
import torch

from sgn_rast import _lib

NAME = "sgn_gt_downscale"
F = ctypes.c_void_p(0x1000)      # never dereferenced: every case below fails its argument check first


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


def test_entry_is_exported_and_declared(lib):
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 11
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sgn_rast.h")).read()
    assert ("int sgn_gt_downscale(int h, int w, int oh, int ow, const unsigned char *image, const unsigned char *mask,"
            in header)
    from sgn_rast import pyramid
    import sgn_rast
    for name in ("Level", "downscale", "downscale_factor", "level_size", "scaled_camera"):
        assert getattr(sgn_rast, name) is getattr(pyramid, name)


def _call(lib, h=64, w=96, oh=32, ow=48, image=F, mask=F, semantic=F, image_out=F, mask_out=F, semantic_out=F):
    return lib.sgn_gt_downscale(h, w, oh, ow, image, mask, semantic, image_out, mask_out, semantic_out, None)


def test_dimension_errors(lib):
    for kw in (dict(h=0), dict(w=0), dict(oh=0), dict(ow=0), dict(h=-4), dict(ow=-1),
               dict(h=16385, oh=16385), dict(w=16385), dict(h=16385), dict(w=16385, ow=16385),
               dict(oh=65), dict(ow=97), dict(h=4, w=4, oh=5, ow=4), dict(h=4, w=4, oh=4, ow=5)):
        assert _call(lib, **kw) == -1, kw
        assert NAME.encode() in lib.sgn_last_error()
    assert _call(lib, h=0, image=None) == -1                 # the dimensions are reported first


def test_pointer_errors(lib):
    for kw in (dict(image=None), dict(image_out=None), dict(mask=None), dict(mask_out=None), dict(semantic=None),
               dict(semantic_out=None), dict(mask=None, mask_out=None, image=None),
               dict(mask=None, mask_out=None, semantic=None, semantic_out=None, image_out=None),
               dict(h=16384, w=16384, oh=1, ow=1, image=None)):
        assert _call(lib, **kw) == -2, kw
        assert NAME.encode() in lib.sgn_last_error()


# ------------------------------------------------------------------------------------------------ host-side errors
H, W = 24, 32


def _triple():
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
    mask = torch.rand(H, W, generator=g) < 0.5
    sem = torch.randint(0, 20, (H, W), dtype=torch.uint8, generator=g)
    return img, mask, sem


def test_host_side_type_errors():
    from sgn_rast import pyramid
    img, mask, sem = _triple()
    assert not issubclass(_lib.SgnRastError, (TypeError, ValueError))
    for bad in ((img.float(), mask, sem), (img.to(torch.int32), None, None), (img.numpy(), None, None),
                (None, mask, sem),
                (img, mask.float(), sem), (img, mask.to(torch.int64), None), (img, [1], None),
                (img, mask, sem.to(torch.int64)), (img, None, sem.float()), (img, None, sem.bool()), (img, None, "sky"),
                img, 7, (img, mask)):
        with pytest.raises(TypeError):
            pyramid.downscale(bad, 2)
    with pytest.raises(TypeError):
        pyramid.downscale([(img, mask, sem), (img.float(), None, None)], 2)      # every item of a list is checked
    for d in (2.0, "2", None, True):
        with pytest.raises(TypeError):
            pyramid.downscale((img, mask, sem), d)
    for size in (12, (12,), (12.5, 16), "ab", (12, 16, 3)):
        with pytest.raises(TypeError):
            pyramid.downscale((img, mask, sem), 2, size=size)


def test_host_side_value_errors():
    from sgn_rast import pyramid
    img, mask, sem = _triple()
    for bad in ((img[..., :2], None, None), (img[..., 0], None, None), (img[None], None, None),
                (img[:0], None, None), (img.permute(2, 0, 1), None, None),
                (img, mask[:-1], None), (img, mask[None], None), (img, mask[..., None, None], None),
                (img, None, sem[:, :-1]), (img, None, sem[None]), (img, mask, sem.reshape(W, H))):
        with pytest.raises(ValueError):
            pyramid.downscale(bad, 2)
    for d in (0, -2, 3, 6, 12):
        with pytest.raises(ValueError):
            pyramid.downscale((img, mask, sem), d)
    for size in ((0, 16), (12, 0), (-1, 16), (H + 1, 16), (12, W + 1)):
        with pytest.raises(ValueError):
            pyramid.downscale((img, mask, sem), 2, size=size)
    with pytest.raises(ValueError):
        pyramid.downscale([], 2)


def test_cpu_tensors_reach_the_device_check():
    """No quiet CPU path; a bad argument is still reported first."""
    from sgn_rast import feed, pyramid
    img, mask, sem = _triple()
    for item in ((img, mask, sem), (img, None, None), feed.Batch(img, mask[..., None].to(torch.uint8), sem[..., None])):
        with pytest.raises(_lib.SgnRastError):
            pyramid.downscale(item, 2)
        with pytest.raises(_lib.SgnRastError):
            pyramid.downscale(item, 1, size=(H, W))
        with pytest.raises(_lib.SgnRastError):
            pyramid.downscale([item, item], 4, size=(5, 7))
    with pytest.raises(TypeError):
        pyramid.downscale((img, mask.float(), sem), 2)


def test_the_full_resolution_level_is_the_batch_itself():
    """d == 1 without a size: nothing is launched (CPU tensors pass), the image stays uint8 for the byte loss."""
    from sgn_rast import feed, pyramid
    img, mask, sem = _triple()
    lv = pyramid.downscale(feed.Batch(img, mask, sem), 1)
    assert isinstance(lv, pyramid.Level)
    assert lv.image is img and lv.mask is mask and lv.semantic is sem
    lvs = pyramid.downscale([(img, None, None), (img, mask, None)], 1)
    assert isinstance(lvs, list) and len(lvs) == 2 and lvs[0].image is img and lvs[0].mask is None and lvs[1].mask is mask

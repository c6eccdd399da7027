"""CPU: every argument error of sgn_rast.feed.ImageFeed is a TypeError / ValueError raised on the host, before any
device work — none of these cases may get as far as pinning memory or touching a GPU (this file runs without one)."""
import pytest
import torch

from sgn_rast import ImageFeed, feed

H, W = 12, 20


def _img(h=H, w=W, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_exported():
    import sgn_rast
    assert sgn_rast.ImageFeed is feed.ImageFeed and sgn_rast.Batch is feed.Batch
    assert feed.Batch._fields == ("image", "mask", "semantic")


BAD_IMAGES = [
    (lambda: [_img().float() / 255.0], TypeError),              # the float cache is what this replaces
    (lambda: [_img().to(torch.int32)], TypeError),
    (lambda: [_img(), _img().numpy()], TypeError),
    (lambda: [_img()[..., 0]], ValueError),                     # wrong rank
    (lambda: [_img()[None]], ValueError),
    (lambda: [_img().permute(2, 0, 1)], ValueError),            # CHW
    (lambda: [torch.zeros(H, W, 4, dtype=torch.uint8)], ValueError),
    (lambda: [torch.zeros(0, W, 3, dtype=torch.uint8)], ValueError),
    (lambda: [], ValueError),
]


@pytest.mark.parametrize("make,exc", BAD_IMAGES)
@pytest.mark.parametrize("cache", ["pinned", "device"])
def test_bad_images(make, exc, cache):
    with pytest.raises(exc):
        ImageFeed(make(), cache=cache)


BAD_MASKS = [
    (lambda: [torch.ones(H, W)], TypeError),                                  # a weight map
    (lambda: [torch.ones(H, W, dtype=torch.int64)], TypeError),
    (lambda: [torch.ones(H, W - 1, dtype=torch.bool)], ValueError),           # not the image's size
    (lambda: [torch.ones(W, H, dtype=torch.bool)], ValueError),
    (lambda: [torch.ones(H, W, 3, dtype=torch.uint8)], ValueError),
    (lambda: [None, None], ValueError),                                       # one entry per image
]


@pytest.mark.parametrize("make,exc", BAD_MASKS)
def test_bad_masks(make, exc):
    with pytest.raises(exc):
        ImageFeed([_img()], masks=make())


def test_a_mask_is_checked_against_its_own_image():
    imgs = [_img(12, 20), _img(16, 24, seed=1)]
    ok = [torch.ones(12, 20, dtype=torch.bool), torch.ones(16, 24, 1, dtype=torch.uint8)]
    ImageFeed(imgs, masks=ok)                                                 # validation only: nothing is allocated
    ImageFeed(imgs, masks=[None, ok[1]])
    with pytest.raises(ValueError):
        ImageFeed(imgs, masks=ok[::-1])


BAD_SEMANTICS = [
    (lambda: [torch.full((H, W), 256, dtype=torch.int64)], ValueError),       # does not fit a byte
    (lambda: [torch.full((H, W, 1), 70000, dtype=torch.int32)], ValueError),
    (lambda: [torch.full((H, W), -1, dtype=torch.int64)], ValueError),
    (lambda: [torch.zeros(H, W)], TypeError),
    (lambda: [torch.zeros(H, W, dtype=torch.bool)], TypeError),               # an "is sky" mask is not a class id
    (lambda: [torch.zeros(H, W + 1, dtype=torch.int64)], ValueError),
    (lambda: [], ValueError),
]


@pytest.mark.parametrize("make,exc", BAD_SEMANTICS)
def test_bad_semantics(make, exc):
    with pytest.raises(exc):
        ImageFeed([_img()], semantics=make())


def test_semantics_up_to_255_pass():
    sem = torch.zeros(H, W, dtype=torch.int64)
    sem[0, 0] = 255
    ImageFeed([_img()], semantics=[sem])
    ImageFeed([_img()], semantics=[sem.to(torch.uint8)[..., None]])


@pytest.mark.parametrize("kw,exc", [
    (dict(cache="host"), ValueError), (dict(cache=None), ValueError), (dict(cache="gpu"), ValueError),
    (dict(slots=1), ValueError), (dict(slots=0), ValueError), (dict(slots=2.0), ValueError),
    (dict(batch=0), ValueError), (dict(device="cpu"), ValueError),
])
def test_bad_settings(kw, exc):
    with pytest.raises(exc):
        ImageFeed([_img()], **kw)


@pytest.mark.parametrize("cache", ["pinned", "device"])
def test_batch_exceeded_and_bad_indices(cache):
    f = ImageFeed([_img(seed=s) for s in range(4)], cache=cache, batch=2)
    assert len(f) == 4
    for call in (f.prefetch, f.get):
        with pytest.raises(ValueError, match="batch"):
            call([0, 1, 2])
        with pytest.raises(ValueError, match="batch"):
            call([])
        with pytest.raises(IndexError):
            call(4)
        with pytest.raises(IndexError):
            call([0, -1])
    one = ImageFeed([_img(), _img(seed=1)])
    with pytest.raises(ValueError, match="batch"):
        one.get([0, 1])

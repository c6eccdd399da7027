"""sgn_rast.pyramid.downscale on the device (csrc/gt_pyramid.hip through sgn_gt_downscale).

* The image is ``torch.equal`` to the numpy restatement of the contract (tests/pyramid_oracle.py): the kernel is the
  contract's operations in the contract's order, built with -ffp-contract=off, so the bits must match.
* The image is within the derived tolerance (tests/test_pyramid_oracle.py: ``1e-6 + 8 * 2**-23 * max(H, W)``, ``1e-6``
  alone where ``d`` divides both sides) of the reference's own operation, ``F.interpolate(..., mode="bilinear",
  align_corners=False, antialias=False)`` on ``img.float() / 255`` computed on the CPU and uploaded.
* Mask and semantic map are ``torch.equal`` to both the restatement and ``F.interpolate(mode="nearest")``.

The images hold every byte value (the first 256 elements are arange(256) wherever there are that many).  Each
reference is computed once per (size, d) and never written to."""
import pytest
import torch
import torch.nn.functional as F

from tests import pyramid_oracle as PO
from tests.test_pyramid_oracle import tolerance, torch_reference

pytestmark = pytest.mark.gpu

# clamped to 1x1, every tap clamped; odd; 11x11, the loss's smallest image; non-divisible, 159-byte rows; divisible;
# three waves a row, the last one partial; one production shape (at d = 2 four workgroups per row)
CASES = [(2, 2, 2), (2, 2, 4), (5, 7, 2), (22, 22, 2), (37, 53, 2), (37, 53, 4), (64, 96, 2), (64, 96, 4), (64, 96, 8),
         (200, 333, 2), (1280, 1920, 2), (1280, 1920, 4), (1280, 1920, 8)]
MASKS = [None, "bool", "uint8x1"]


def _inputs(h, w, seed=None):
    """CPU (image uint8 [h,w,3], mask bool [h,w], semantic uint8 [h,w] of classes 0..19)."""
    g = torch.Generator().manual_seed(h * 1000 + w if seed is None else seed)
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g)
    if img.numel() >= 256:
        img.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
        assert len(torch.unique(img)) == 256
    mask = torch.rand(h, w, generator=g) < 0.6
    sem = torch.randint(0, 20, (h, w), dtype=torch.uint8, generator=g)
    return img, mask, sem


_REFS: dict = {}


def _ref(h, w, oh, ow):
    """Inputs on the device and, per output size, the restatement and the CPU interpolate results uploaded."""
    key = (h, w, oh, ow)
    if key not in _REFS:
        img, mask, sem = _inputs(h, w)
        m8 = mask.to(torch.uint8)
        t_img, t_sem = torch_reference(img, sem, oh, ow)
        t_mask = F.interpolate(m8[None, None], size=(oh, ow), mode="nearest")[0, 0].contiguous()
        _REFS[key] = dict(
            img=img.cuda(), mask=mask.cuda(), sem=sem.cuda(),
            o_img=torch.from_numpy(PO.image(img.numpy(), oh, ow)).cuda(),
            o_mask=torch.from_numpy(PO.nearest(m8.numpy(), oh, ow)).cuda(),
            o_sem=torch.from_numpy(PO.nearest(sem.numpy(), oh, ow)).cuda(),
            t_img=t_img.cuda(), t_mask=t_mask.cuda(), t_sem=t_sem.cuda())
    return _REFS[key]


def _check(lv, r, h, w, d, oh, ow, mask_kind, with_sem):
    assert lv.image.is_cuda and lv.image.dtype == torch.float32 and lv.image.shape == (oh, ow, 3)
    assert lv.image.is_contiguous()
    diff = float((lv.image - r["t_img"]).abs().max())
    tol = tolerance(h, w, d)
    n_off = int((lv.image != r["o_img"]).sum())
    print(f"[pyramid] {h}x{w} d={d} -> {oh}x{ow} mask={mask_kind} sem={with_sem}: {n_off} elements differ from the "
          f"restatement; max |kernel - interpolate| {diff:.2e} (tolerance {tol:.2e})")
    assert torch.equal(lv.image, r["o_img"])
    assert diff <= tol
    if mask_kind is None:
        assert lv.mask is None
    else:
        bool_ = mask_kind == "bool"
        assert lv.mask.dtype == (torch.bool if bool_ else torch.uint8)
        assert lv.mask.shape == ((oh, ow) if bool_ else (oh, ow, 1))
        got = lv.mask.to(torch.uint8).reshape(oh, ow)
        scale = 1 if bool_ else 255
        assert torch.equal(got, r["o_mask"] * scale) and torch.equal(got, r["t_mask"] * scale)
    if not with_sem:
        assert lv.semantic is None
    else:
        assert lv.semantic.dtype == torch.uint8 and lv.semantic.shape == (oh, ow)
        assert torch.equal(lv.semantic, r["o_sem"]) and torch.equal(lv.semantic, r["t_sem"])


def _mask_as(kind, mask):
    if kind is None:
        return None
    return mask if kind == "bool" else (mask.to(torch.uint8) * 255)[..., None]


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("h,w,d", CASES)
def test_level_equals_the_restatement_and_the_reference(h, w, d, mask_kind):
    from sgn_rast import pyramid
    oh, ow = pyramid.level_size(h, w, d)
    r = _ref(h, w, oh, ow)
    before = r["img"].clone()
    for with_sem in (False, True):
        lv = pyramid.downscale((r["img"], _mask_as(mask_kind, r["mask"]), r["sem"] if with_sem else None), d)
        assert isinstance(lv, pyramid.Level)
        _check(lv, r, h, w, d, oh, ow, mask_kind, with_sem)
    assert torch.equal(r["img"], before)                       # the inputs are only read


def test_semantic_keeps_its_trailing_one():
    from sgn_rast import feed, pyramid
    r = _ref(37, 53, 19, 27)
    lv = pyramid.downscale(feed.Batch(r["img"], r["mask"][..., None], r["sem"][..., None]), 2)
    assert lv.mask.dtype == torch.bool and lv.mask.shape == (19, 27, 1)
    assert lv.semantic.dtype == torch.uint8 and lv.semantic.shape == (19, 27, 1)
    assert torch.equal(lv.semantic[..., 0], r["o_sem"]) and torch.equal(lv.mask[..., 0], r["o_mask"].bool())
    assert torch.equal(lv.image, r["o_img"])


def test_size_override_is_the_scaled_cameras_floor():
    """37x53 at d = 2: level_size says 19x27, the scaled camera 18x26; the caller passes the camera's."""
    from sgn_rast import pyramid, scenes
    cam = pyramid.scaled_camera(scenes.make_camera(53, 37, 50.0), 2)
    assert (cam.height, cam.width) == (18, 26)
    r = _ref(37, 53, 18, 26)
    lv = pyramid.downscale((r["img"], r["mask"], r["sem"]), 2, size=(cam.height, cam.width))
    _check(lv, r, 37, 53, 2, 18, 26, "bool", True)
    assert not torch.equal(lv.image, _ref(37, 53, 19, 27)["o_img"][:18, :26])


def test_full_size_through_the_kernel_is_the_quotient():
    """d = 1 with a size: the kernel runs at scale 1 and returns u / 255 (the CPU's quotient), bytes copied."""
    from sgn_rast import pyramid
    r = _ref(37, 53, 19, 27)
    lv = pyramid.downscale((r["img"], r["mask"], r["sem"]), 1, size=(37, 53))
    assert torch.equal(lv.image, (r["img"].cpu().float() / 255.0).cuda())
    assert torch.equal(lv.mask, r["mask"]) and torch.equal(lv.semantic, r["sem"])
    same = pyramid.downscale((r["img"], r["mask"], r["sem"]), 1)
    assert same.image is r["img"] and same.image.dtype == torch.uint8


def test_a_list_gives_a_list():
    from sgn_rast import pyramid
    a, b = _ref(37, 53, 19, 27), _ref(64, 96, 32, 48)
    lvs = pyramid.downscale([(a["img"], a["mask"], None), (b["img"], None, b["sem"])], 2)
    assert isinstance(lvs, list) and len(lvs) == 2
    _check(lvs[0], a, 37, 53, 2, 19, 27, "bool", False)
    _check(lvs[1], b, 64, 96, 2, 32, 48, None, True)


def test_a_side_stream():
    """The launch goes to the current stream."""
    from sgn_rast import pyramid
    r = _ref(200, 333, 100, 167)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        img = r["img"].clone()
        lv = pyramid.downscale((img, None, None), 2)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(lv.image, r["o_img"])


# ------------------------------------------------------------------------------------------------ through the loop
def test_levels_outlive_the_feed_slot():
    """get -> downscale -> prefetch(next) over a pinned feed of two slots.  Slot k is rewritten by the prefetch after
    the next get, so a level that aliased its slot would hold another item's pixels by the time it is compared: level s
    is looked at only after iteration s + 2's prefetch has been enqueued."""
    from sgn_rast import ImageFeed, pyramid
    n, h, w = 4, 64, 96
    items = [_inputs(h, w, seed=70 + i) for i in range(n)]
    masks = [(m if i % 2 == 0 else (m.to(torch.uint8) * 255)[..., None]) for i, (_, m, _) in enumerate(items)]
    feed = ImageFeed([it[0] for it in items], masks, [it[2] for it in items], cache="pinned", slots=2)
    expect = [(torch.from_numpy(PO.image(img.numpy(), 32, 48)), torch.from_numpy(PO.nearest(masks[i].numpy(), 32, 48)),
               torch.from_numpy(PO.nearest(sem.numpy(), 32, 48))) for i, (img, _, sem) in enumerate(items)]

    def same(s, lv):
        e_img, e_mask, e_sem = expect[s]
        assert torch.equal(lv.image.cpu(), e_img), s
        assert lv.mask.dtype == e_mask.dtype and lv.mask.shape == e_mask.shape and torch.equal(lv.mask.cpu(), e_mask), s
        assert lv.semantic.dtype == torch.uint8 and torch.equal(lv.semantic.cpu(), e_sem), s

    levels = []
    feed.prefetch(0)
    for s in range(n):
        b = feed.get(s)
        levels.append(pyramid.downscale(b, 2))
        assert levels[s].image.data_ptr() != b.image.data_ptr()
        feed.prefetch((s + 1) % n)
        if s >= 2:
            same(s - 2, levels[s - 2])
    feed.get(0)                                  # two more turns of the slots behind the last two levels
    feed.prefetch(1)
    feed.get(1)
    feed.prefetch(2)
    same(n - 2, levels[n - 2])
    same(n - 1, levels[n - 1])


# ---------------------------------------------------------------------------------------------------- in the step
def _scene(yaw=0.0):
    from sgn_rast import scenes
    cam = scenes.make_camera(96, 64, 96.0, yaw=yaw, device="cuda")
    raw = scenes.make_gaussians(2000, scenes.make_camera(96, 64, 96.0, device="cuda"), seed=2, z_range=(1.0, 5.0),
                                device="cuda")
    return cam, raw


def test_one_train_step_on_a_level():
    from sgn_rast import loss, pyramid, step
    cam, raw = _scene()
    cam2 = pyramid.scaled_camera(cam, 2)
    assert (cam2.width, cam2.height, cam2.fx, cam2.cx) == (48, 32, 48.0, 24.0)
    r = _ref(64, 96, 32, 48)
    lv = pyramid.downscale((r["img"], r["mask"], r["sem"]), 2, size=(cam2.height, cam2.width))
    P = step.leaf_params(raw)
    w_img = torch.zeros(32, 48, 3, device="cuda")
    w_a = torch.zeros(32, 48, device="cuda")        # the alpha term of the step's loss is then exactly 0
    out = step.train_step(P, cam2, w_img, w_a, gt=lv.image, mask=lv.mask, fused=True)
    assert out.rgb.shape == (32, 48, 3)
    assert bool(torch.isfinite(out.loss))
    assert float(P["means"].grad.abs().max()) > 0.0
    again = loss.photometric_loss(out.rgb.detach(), lv.image, 0.2, clamp_max=1.0, mask=lv.mask)
    print(f"[pyramid step] loss {float(out.loss):.8f}, photometric recomputed {float(again):.8f}")
    assert float(out.loss) == float(again)
    assert 0.0 < float(out.loss) < 1.0


def test_train_step_views_on_levels():
    from sgn_rast import loss, pyramid, step, views
    cam0, raw = _scene()
    cam1, _ = _scene(yaw=0.15)
    cams = [pyramid.scaled_camera(c, 2) for c in (cam0, cam1)]
    a = _ref(64, 96, 32, 48)
    img1, mask1, _ = _inputs(64, 96, seed=91)
    lvs = pyramid.downscale([(a["img"], a["mask"], None), (img1.cuda(), None, None)], 2)
    assert torch.equal(lvs[1].image, torch.from_numpy(PO.image(img1.numpy(), 32, 48)).cuda())
    P = step.leaf_params(raw)
    gts, masks = [lv.image for lv in lvs], [lv.mask for lv in lvs]
    out = views.train_step_views(P, cams, gts=gts, masks=masks)
    assert out.rgb.shape == (2, 32, 48, 3)
    assert bool(torch.isfinite(out.loss))
    assert float(P["means"].grad.abs().max()) > 0.0
    again = sum(loss.photometric_loss(out.rgb[v].detach(), gts[v], 0.2, clamp_max=1.0, mask=masks[v])
                for v in range(2)) / 2
    print(f"[pyramid views] loss {float(out.loss):.8f}, photometric recomputed {float(again):.8f}")
    assert float(out.loss) == float(again)

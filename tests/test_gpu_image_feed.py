"""sgn_rast.feed.ImageFeed on the device: what comes out is what went in (both cache modes, with and without a
matching prefetch), and the slot lifetime contract of the pinned mode — a slot is rewritten only behind the work that
reads it — checked as values: the prefetch loop must reproduce, bit for bit, the same loop on resident tensors.  A wrong
ordering of the copies shows as wrong numbers here, never as a fault: every access stays inside the feed's own slots."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _img(h, w, seed):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _items():
    """Three sizes (none a multiple of the feed's alignment); a bool mask, no mask, a uint8 [H,W,1] mask; semantics on
    all, in three dtypes and both shapes."""
    sizes = [(13, 17), (37, 53), (64, 48)]
    g = torch.Generator().manual_seed(3)
    images = [_img(h, w, 10 + i) for i, (h, w) in enumerate(sizes)]
    masks = [torch.rand(13, 17, generator=g) < 0.6, None,
             (torch.rand(64, 48, 1, generator=g) < 0.6).to(torch.uint8) * 255]
    semantics = [torch.randint(0, 256, (13, 17), generator=g),
                 torch.randint(0, 20, (37, 53, 1), generator=g).to(torch.int32),
                 torch.randint(0, 256, (64, 48), generator=g).to(torch.uint8)]
    return images, masks, semantics


def _same(b, image, mask, semantic):
    assert b.image.is_cuda and b.image.dtype == torch.uint8 and b.image.is_contiguous()
    assert torch.equal(b.image.cpu(), image)
    if mask is None:
        assert b.mask is None
    else:
        assert b.mask.dtype == mask.dtype and b.mask.shape == mask.shape and torch.equal(b.mask.cpu(), mask)
    assert b.semantic.dtype == torch.uint8 and b.semantic.shape == semantic.shape
    assert torch.equal(b.semantic.cpu().to(torch.int64), semantic.to(torch.int64))


@pytest.mark.parametrize("cache", ["pinned", "device"])
def test_round_trip(cache):
    from sgn_rast import Batch, ImageFeed
    images, masks, semantics = _items()
    feed = ImageFeed(images, masks, semantics, cache=cache)
    n = len(images)
    for i in (2, 0, 1, 1):                                  # get without prefetch
        b = feed.get(i)
        assert isinstance(b, Batch)
        _same(b, images[i], masks[i], semantics[i])
    for i in (1, 2, 0):                                     # the intended order
        feed.prefetch(i)
        _same(feed.get(i), images[i], masks[i], semantics[i])
    for i in range(n):                                      # a prefetch of the wrong item, then get
        feed.prefetch((i + 1) % n)
        _same(feed.get(i), images[i], masks[i], semantics[i])
    feed.prefetch(0)                                        # two prefetches in a row: the second one counts
    feed.prefetch(2)
    _same(feed.get(2), images[2], masks[2], semantics[2])
    out = feed.get([1])                                     # a sequence gives a list
    assert isinstance(out, list) and len(out) == 1
    _same(out[0], images[1], masks[1], semantics[1])


def test_a_get_stays_intact_until_the_prefetch_after_the_next_get():
    from sgn_rast import ImageFeed
    images, masks, semantics = _items()
    feed = ImageFeed(images, masks, semantics, cache="pinned", slots=2)
    feed.prefetch(0)
    b0 = feed.get(0)
    feed.prefetch(1)
    b1 = feed.get(1)
    _same(b0, images[0], masks[0], semantics[0])            # slot 0 untouched while slot 1 was filled and handed out
    _same(b1, images[1], masks[1], semantics[1])
    keep = b0.image.clone()
    feed.prefetch(2)                                        # now slot 0 is rewritten, behind the clone above
    b2 = feed.get(2)
    assert torch.equal(keep.cpu(), images[0])
    _same(b1, images[1], masks[1], semantics[1])
    _same(b2, images[2], masks[2], semantics[2])


def test_feed_outputs_go_straight_into_the_losses():
    from sgn_rast import ImageFeed, loss
    h, w = 37, 53
    img = _img(h, w, 1)
    g = torch.Generator().manual_seed(2)
    mask = torch.rand(h, w, generator=g) < 0.7
    sem = torch.randint(0, 5, (h, w, 1), generator=g)
    feed = ImageFeed([img], [mask], [sem])
    b = feed.get(0)
    pred, acc = torch.rand(h, w, 3, generator=g).cuda(), torch.rand(h, w, 1, generator=g).cuda()
    assert torch.equal(loss.photometric_loss(pred, b.image, 0.2, clamp_max=1.0, mask=b.mask),
                       loss.photometric_loss(pred, img.cuda(), 0.2, clamp_max=1.0, mask=mask.cuda()))
    assert torch.equal(loss.sky_accumulation(acc, b.semantic), loss.sky_accumulation(acc, sem.cuda()))


# --------------------------------------------------------------------------------------------------------- lifetime
def _loop(get, prefetch, order, preds, calls):
    """The documented loop; the consumer's work is `calls` photometric forward + backward passes.  Nothing in it
    synchronises the host; the results are looked at after it."""
    from sgn_rast import loss
    losses, grads = [], []
    prefetch(order[0])
    for s, i in enumerate(order):
        b = get(i)
        if s + 1 < len(order):
            prefetch(order[s + 1])
        p = preds[s % len(preds)].clone().requires_grad_(True)
        for _ in range(calls):
            val = loss.photometric_loss(p, b.image, 0.2, clamp_max=1.0, mask=b.mask)
            val.backward()
        losses.append(val.detach())
        grads.append(p.grad)
    return losses, grads


@pytest.mark.parametrize("h,w,n_items,steps,calls", [(200, 333, 5, 24, 1), (1280, 1920, 3, 6, 3)])
def test_prefetch_loop_equals_resident_tensors(h, w, n_items, steps, calls):
    """slots=2.  Small images: the copies are short and many.  Large images, three loss calls per step: the copy is long
    finished while the consumer still reads the other slot, and the next copy must wait for the consumer."""
    from sgn_rast import Batch, ImageFeed
    g = torch.Generator().manual_seed(h + w)
    images = [_img(h, w, 100 + i) for i in range(n_items)]
    masks = [(torch.rand(h, w, generator=g) < 0.8) if i % 2 else None for i in range(n_items)]
    order = torch.randint(0, n_items, (steps,), generator=g).tolist()
    assert len(set(order)) == n_items
    preds = [torch.rand(h, w, 3, generator=g).cuda() * 1.1 for _ in range(2)]
    resident = [Batch(im.cuda(), None if m is None else m.cuda(), None) for im, m in zip(images, masks)]
    exp_l, exp_g = _loop(lambda i: resident[i], lambda i: None, order, preds, calls)
    feed = ImageFeed(images, masks, cache="pinned", slots=2)
    feed.open()
    torch.cuda.synchronize()
    got_l, got_g = _loop(feed.get, feed.prefetch, order, preds, calls)
    torch.cuda.synchronize()
    bad = [s for s in range(steps) if not (torch.equal(got_l[s], exp_l[s]) and torch.equal(got_g[s], exp_g[s]))]
    assert not bad, f"steps {bad} of {order} differ from the resident loop"
    assert len({float(v) for v in exp_l}) >= n_items          # the items do give different losses


# ---------------------------------------------------------------------------------------------------------- batches
def test_batches_feed_train_step_views():
    from sgn_rast import ImageFeed, scenes, step, views
    cam0, raw = scenes.make_scene("c1", seed=2, n_override=1500, device="cuda")
    cam1, _ = scenes.make_scene("c1", seed=2, yaw=0.15, n_override=1500, device="cuda")
    cams = [cam0, cam1]
    h, w = cam0.height, cam0.width
    g = torch.Generator().manual_seed(6)
    images = [_img(h, w, 20 + i) for i in range(4)]
    masks = [torch.rand(h, w, generator=g) < 0.8, None, None, torch.rand(h, w, generator=g) < 0.8]
    feed = ImageFeed(images, masks, batch=2)
    steps = [[0, 1], [2, 3], [1, 0]]
    feed.prefetch(steps[0])
    for s, ids in enumerate(steps):
        bs = feed.get(ids)
        assert isinstance(bs, list) and len(bs) == 2
        if s + 1 < len(steps):
            feed.prefetch(steps[s + 1])
        P = step.leaf_params(raw)
        got = views.train_step_views(P, cams, [b.image for b in bs], masks=[b.mask for b in bs])
        Pr = step.leaf_params(raw)
        ref = views.train_step_views(Pr, cams, [images[i].cuda() for i in ids],
                                     masks=[None if masks[i] is None else masks[i].cuda() for i in ids])
        assert torch.equal(got.loss.detach(), ref.loss.detach()), ids
        for b, i in zip(bs, ids):
            assert torch.equal(b.image.cpu(), images[i])

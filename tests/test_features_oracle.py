"""CPU: the two yardsticks of tests/test_gpu_features.py, pinned on their own.

* The channel-generic torch oracle at K = 5 equals its own 3-channel calls on the column triples — image, alpha and the
  gradients of every input — so "the same channel of a 3-channel pass" and "the channel-generic oracle" are one thing.
* The fp64 definition of the semantic cross-entropy (tests/semantic_fp64.py) equals torch's fp64 `F.cross_entropy`, with
  and without `ignore_index`, with and without a mask."""
import pytest
import torch

import semantic_fp64 as SF
from helpers import activated, small_scene
from sgn_rast import features as F  # noqa: F401  (the module these yardsticks serve: without it nothing here runs)


def test_channel_generic_oracle_equals_its_three_channel_calls(torch_oracle):
    cam, P = small_scene(n=400, w=48, h=40, focal=48.0)
    scales, quats, opac, _ = activated(P)
    with torch.no_grad():
        xys, depths, radii, conics, _comp, nth, _cov = torch_oracle.project_gaussians(
            P["means"], scales, 1.0, quats, cam.viewmat, cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, 16)
    R = dict(xys=xys, depths=depths, radii=radii, conics=conics, nth=nth, opac=opac)
    K, D = 5, torch.float64
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(R["xys"].shape[0], K, generator=g).to(D)
    bg = torch.rand(K, generator=g).to(D)
    w_img = torch.rand(cam.height, cam.width, K, generator=g).to(D)
    w_a = torch.rand(cam.height, cam.width, generator=g).to(D)

    def run(cols, bgc, w, with_alpha):
        t = [R["xys"].to(D).requires_grad_(True), R["conics"].to(D).requires_grad_(True),
             feats.clone().requires_grad_(True), R["opac"].to(D).requires_grad_(True)]
        img, alpha = torch_oracle.rasterize_gaussians(t[0], R["depths"].to(D), R["radii"], t[1], R["nth"], t[2][:, cols],
                                                      t[3], cam.height, cam.width, 16, bgc, True)
        ((img * w).sum() + (alpha * w_a).sum() * float(with_alpha)).backward()
        return img.detach(), alpha.detach(), [x.grad for x in t]

    img5, alpha5, g5 = run(list(range(K)), bg, w_img, True)
    assert float(alpha5.max()) > 0.2
    triples = [[0, 1, 2], [3, 4, 4]]              # the second pass pads with a repeated column of weight zero
    acc = None
    for i, cols in enumerate(triples):
        w = w_img[..., cols].clone()
        if i == 1:
            w[..., 2] = 0.0
        img3, alpha3, g3 = run(cols, bg[cols], w, i == 0)
        assert torch.equal(alpha3, alpha5)
        for j, c in enumerate(cols[:3 if i == 0 else 2]):
            assert torch.allclose(img3[..., j], img5[..., c], rtol=0, atol=1e-14), c
        acc = g3 if acc is None else [a + b for a, b in zip(acc, g3)]
    for a, b in zip(acc, g5):                       # v_alpha is linear in the channels: the passes' gradients add up
        assert float((a - b).norm() / b.norm()) < 1e-12


@pytest.mark.parametrize("n_classes", [3, 19, 64])
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("masked", [False, True])
def test_fp64_cross_entropy_definition_equals_torch(n_classes, ignore, masked):
    logits, labels, mask = SF.case(n_classes, h=20, w=30, ignore_index=255 if ignore is not None else 0)
    if ignore is None:
        labels = labels.clamp(max=n_classes - 1)
    m = mask if masked else None
    loss, grad = SF.cross_entropy_fp64(logits, labels, ignore, m)
    t_loss, t_grad = SF.torch_cross_entropy(logits.double(), labels, ignore, m)
    assert abs(float(loss - t_loss)) < 1e-13 * max(1.0, abs(float(t_loss)))
    assert float((grad - t_grad).abs().max()) < 1e-15
    assert int(SF.counted_pixels(labels, n_classes, ignore, m).sum()) > 100


def test_fp64_cross_entropy_of_an_image_without_counted_pixels():
    logits, labels, mask = SF.case(5, h=8, w=9, all_ignored=True)
    loss, grad = SF.cross_entropy_fp64(logits, labels, 255, mask)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0

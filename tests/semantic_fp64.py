"""The fp64 definition of the semantic cross-entropy that tests/test_gpu_features.py holds `semantic_cross_entropy` to
(tests/test_features_oracle.py pins it against torch's own fp64 `F.cross_entropy` on the CPU), and the seeded inputs both
use.  Written from the formula — loss = mean over counted pixels of logsumexp(x) - x[label], gradient (softmax - onehot) /
count on counted pixels — not through autograd."""
import torch


def counted_pixels(labels, n_classes, ignore_index=None, mask=None):
    lab = labels.reshape(labels.shape[0], labels.shape[1]).long()
    c = lab < n_classes
    if ignore_index is not None:
        c = c & (lab != int(ignore_index))
    if mask is not None:
        c = c & (mask.reshape(c.shape) != 0)
    return c


def cross_entropy_fp64(logits, labels, ignore_index=None, mask=None):
    """-> (loss, gradient [H,W,K]) in fp64."""
    x = logits.detach().double()
    H, W, K = x.shape
    c = counted_pixels(labels, K, ignore_index, mask)
    lab = labels.reshape(H, W).long().clamp(max=K - 1)
    m = x.amax(dim=-1, keepdim=True)
    e = torch.exp(x - m)
    S = e.sum(dim=-1, keepdim=True)
    lse = (m + torch.log(S))[..., 0]
    per_pixel = lse - x.gather(-1, lab[..., None])[..., 0]
    count = int(c.sum())
    if count == 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    loss = (per_pixel * c).sum() / count
    onehot = torch.zeros_like(x).scatter_(-1, lab[..., None], 1.0)
    grad = (e / S - onehot) * c[..., None] / count
    return loss, grad


def torch_cross_entropy(logits, labels, ignore_index=None, mask=None):
    """torch.nn.functional.cross_entropy in the dtype / on the device of `logits` -> (loss, gradient); pixels that do
    not count get torch's ignore label."""
    x = logits.detach().clone().requires_grad_(True)
    H, W, K = x.shape
    c = counted_pixels(labels, K, ignore_index, mask).to(x.device)
    tgt = torch.where(c, labels.reshape(H, W).long().to(x.device), torch.full_like(c, -100, dtype=torch.long))
    if int(c.sum()) == 0:
        return torch.zeros((), dtype=x.dtype, device=x.device), torch.zeros_like(x)
    loss = torch.nn.functional.cross_entropy(x.reshape(-1, K), tgt.reshape(-1), ignore_index=-100)
    loss.backward()
    return loss.detach(), x.grad


def case(n_classes, h=50, w=70, seed=0, ignore_index=255, all_ignored=False):
    """Seeded logits [h,w,K], uint8 labels with about a tenth of the pixels carrying `ignore_index`, a byte mask that
    drops about a fifth."""
    g = torch.Generator().manual_seed(1000 * n_classes + seed)
    logits = torch.randn(h, w, n_classes, generator=g) * 3.0
    labels = torch.randint(0, n_classes, (h, w), generator=g).to(torch.uint8)
    labels[torch.rand(h, w, generator=g) < 0.1] = ignore_index
    if all_ignored:
        labels[:] = ignore_index
    mask = (torch.rand(h, w, generator=g) > 0.2).to(torch.uint8)
    return logits, labels, mask

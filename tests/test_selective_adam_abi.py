"""CPU: ``sgn_adam_step_visible`` reports every argument error with its documented code (include/sgn_rast.h) before
anything touches a device, and ``optim.visibility`` maps a scene graph's parameters to the radii parts without a copy."""
import ctypes as C

import pytest
import torch

N = 2


@pytest.fixture(scope="module")
def built_lib():
    from sgn_rast import _lib
    return _lib


def _call(lib, count=N, null=None, numel=(12, 8), steps=(1, 7), rows=(4, 8), kinds=(1, 2), vis=(0x1000, 0x2000),
          tensors=(0x3000, 0x4000)):
    """One call on made-up addresses: every case below fails its check before a pointer is followed."""
    n = max(count, 0) or 1
    arr = lambda ctype, values: (ctype * n)(*list(values)[:n])
    ptrs = lambda: arr(C.c_void_p, tensors)
    dbl = lambda x: arr(C.c_double, [x] * n)
    args = dict(params=ptrs(), grads=ptrs(), exp_avgs=ptrs(), exp_avg_sqs=ptrs(), numel=arr(C.c_int64, numel),
                lr=dbl(1e-3), beta1=dbl(0.9), beta2=dbl(0.999), eps=dbl(1e-15), steps=arr(C.c_int64, steps),
                rows=arr(C.c_int64, rows), visible=arr(C.c_void_p, vis), vis_kind=arr(C.c_int32, kinds))
    if null is not None:
        args[null] = None
    return lib.sgn_adam_step_visible(count, *args.values(), None)


def test_argument_errors_are_reported_without_a_gpu(built_lib):
    lib = built_lib.load()
    assert _call(lib, count=-1) == -1
    assert _call(lib, count=0) == 0
    assert lib.sgn_adam_step_visible(0, *([None] * 13), None) == 0
    for name in ("params", "grads", "exp_avgs", "exp_avg_sqs", "numel", "lr", "beta1", "beta2", "eps", "steps", "rows",
                 "visible", "vis_kind"):
        assert _call(lib, null=name) == -2, name
    assert b"sgn_adam_step_visible" in lib.sgn_last_error()
    assert _call(lib, numel=(12, -1)) == -3
    assert _call(lib, steps=(1, 0)) == -3
    assert _call(lib, tensors=(0x3000, None)) == -4
    for bad in (-1, 3):
        assert _call(lib, kinds=(1, bad)) == -5, bad
        assert _call(lib, kinds=(bad, 0), numel=(0, 8)) == -5, bad          # also on an empty tensor
    assert b"vis_kind" in lib.sgn_last_error()
    for bad in (0, -4):
        assert _call(lib, rows=(4, bad)) == -6, bad
    assert _call(lib, rows=(5, 8)) == -7                                       # 12 % 5
    assert _call(lib, rows=(4, 3), kinds=(1, 0)) == -7                         # 8 % 3, a dense tensor too
    assert b"numel[i] % rows[i]" in lib.sgn_last_error()
    assert _call(lib, vis=(None, 0x2000)) == -8
    assert _call(lib, vis=(0x1000, None)) == -8
    # the first error in tensor order wins, and nothing was launched for the tensors before it
    assert _call(lib, rows=(5, 0)) == -7 and _call(lib, rows=(0, 3)) == -6


def test_an_empty_tensor_is_skipped_before_its_row_checks(built_lib):
    """numel = 0 with rows = 0 and no pointers at all is not an error (a [0, 3] parameter); the error behind it is
    still found."""
    lib = built_lib.load()
    assert _call(lib, numel=(0, 8), rows=(0, 3), tensors=(None, 0x4000), vis=(None, 0x2000)) == -7


def test_visibility_maps_every_parameter_to_its_part_without_a_copy():
    from sgn_rast import optim
    counts = (5, 0, 3)
    models = [dict(means=torch.zeros(n, 3), opacity_logits=torch.zeros(n, 1), features_rest=torch.zeros(n, 15, 3))
              for n in counts]
    radii = torch.arange(sum(counts), dtype=torch.int32)
    parts = torch.split(radii, counts)
    vis = optim.visibility(models, parts)
    assert len(vis) == 9
    at = 0
    for model, part, n in zip(models, parts, counts):
        for p in model.values():
            assert vis[p] is part
            assert vis[p].shape == (n,)
            assert n == 0 or vis[p].data_ptr() == radii.data_ptr() + 4 * at     # (torch gives an empty view no address)
        at += n
    assert optim.visibility([], []) == {}
    with pytest.raises(ValueError):
        optim.visibility(models, parts[:2])
    with pytest.raises(ValueError):
        optim.visibility(models[:2], parts)
    with pytest.raises(ValueError):                                            # a part of another sub-model's length
        optim.visibility(models, (parts[0], parts[2], parts[1]))


def test_a_bad_visibility_raises_before_a_step_is_counted():
    """On CPU tensors: the visibility is refused before ``state['step']`` moves and before the device is asked for."""
    from sgn_rast.optim import FusedAdam
    p = torch.nn.Parameter(torch.randn(6, 3))
    p.grad = torch.ones_like(p)
    opt = FusedAdam([p], lr=0.01)
    opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    before = p.detach().clone()
    for bad, error in ((torch.ones(6), TypeError), (torch.ones(6, dtype=torch.int64), TypeError),
                       (torch.ones(5, dtype=torch.bool), ValueError), (torch.ones(6, 1, dtype=torch.bool), ValueError),
                       (torch.ones(12, dtype=torch.int32)[::2], ValueError), ([1] * 6, TypeError),
                       ({p: [1] * 6}, TypeError)):
        with pytest.raises(error):
            opt.step(visible=bad)
        assert float(opt.state[p]["step"]) == 3.0 and torch.equal(p.detach(), before)

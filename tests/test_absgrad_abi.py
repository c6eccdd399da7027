"""CPU: `sgn_raster_bwd_abs` (include/sgn_rast.h) reports its argument errors before anything touches a device, in the
style of test_abi.py::test_argument_errors_are_reported_without_a_gpu; the Python surface rejects the call shapes the
absgrad statistic does not exist for before anything is launched."""
import pytest
import torch

from sgn_rast import _lib


ENTRY_TAILS = {"sgn_raster_bwd": 0, "sgn_raster_bwd_part": 2, "sgn_raster_bwd_abs": 3}   # of (first, last, v_xy_abs)


def _call(lib, n=4, window=0, v_xy_abs=1, grad_ws_bytes=4 * 48, block=16, first=1, last=1, entry="sgn_raster_bwd_abs"):
    p = 1                                          # a non-NULL address nothing reads: every case fails its check first
    tail = (first, last, v_xy_abs)[:ENTRY_TAILS[entry]]
    return getattr(lib, entry)(8, 8, block, n, 3, p, p, p, p, p, p, 0, 0, n, window, p, p, p, p, p, 0.99, p, p, p, p,
                               p, n * 48, 1, p, grad_ws_bytes, None, None, None, None, None, *tail)


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    assert "sgn_raster_bwd_abs" in _lib.SIGNATURES
    # one more pointer than sgn_raster_bwd_part, everything else argument for argument
    part, abs_ = _lib.SIGNATURES["sgn_raster_bwd_part"], _lib.SIGNATURES["sgn_raster_bwd_abs"]
    assert abs_[0] is part[0] and abs_[1][:-1] == part[1] and abs_[1][-1] is _lib._vp
    assert _call(lib, v_xy_abs=None) == -14 and b"v_xy_abs" in lib.sgn_last_error()
    assert _call(lib, window=1) == -13 and b"window" in lib.sgn_last_error()
    assert _call(lib, grad_ws_bytes=4 * 48 - 1) == -5 and b"grad_ws_bytes" in lib.sgn_last_error()
    assert _call(lib, block=32) == -2 and b"block_width" in lib.sgn_last_error()
    assert _call(lib, n=0, grad_ws_bytes=0) == 0                   # nothing to do is not an error
    assert lib.sgn_raster_bwd_workspace_bytes(4) == 4 * 48         # slots 9, 10 live in the row the plain walks use


@pytest.mark.parametrize("entry", sorted(ENTRY_TAILS))
def test_shared_checks_report_the_entry_that_was_called(entry):
    """The three single-view backward entries share their checks; a failure carries the name of the entry the caller
    used, and the condition's text its argument names."""
    lib = _lib.load()
    assert _call(lib, block=32, entry=entry) == -2
    err = lib.sgn_last_error()
    assert err.startswith(entry.encode() + b":") and b"block_width" in err, err
    assert _call(lib, grad_ws_bytes=4 * 48 - 1, entry=entry) == -5
    err = lib.sgn_last_error()
    assert err.startswith(entry.encode() + b":") and b"grad_ws_bytes" in err, err


def test_unsupported_call_shapes_raise_before_any_launch():
    from sgn_rast import features, fused, step, views
    t = torch.zeros(4, 2)                          # CPU tensors: a launch would raise SgnRastError, not ValueError
    with pytest.raises(ValueError, match="absgrad is not supported"):
        fused.rasterize_gaussians_fused(t, t, t, t, t, t, t, 8, 8, 16, id_range=(0, 2), absgrad=True)
    with pytest.raises(ValueError, match="absgrad is not supported"):
        features.rasterize_features(t, t, t, t, t, t, t, 8, 8, absgrad=True)
    with pytest.raises(ValueError, match="absgrad is not supported"):
        views.render_views({}, [], absgrad=True)
    with pytest.raises(ValueError, match="absgrad is not supported"):
        step.train_step({}, None, None, None, fused=False, absgrad=True)
    with pytest.raises(ValueError, match="absgrad is not supported"):
        step.render_scene_graph([{"means": t}], None, None, None, fused=False, absgrad=True)


def test_densify_config_reads_absgrad():
    from helpers import TorchStats
    from sgn_rast import densify
    assert densify.DensifyConfig().absgrad is False
    g = torch.Generator().manual_seed(0)
    grad, absg = torch.randn(5, 2, generator=g), torch.rand(5, 2, generator=g) + 1.0
    radii = torch.tensor([3, 0, 2, 5, 1], dtype=torch.int32)
    P = {k: torch.zeros(5, 1) for k in densify.PARAM_NAMES}
    runs = {}
    for flag in (False, True):
        d = densify.Densifier(P, {k: None for k in densify.PARAM_NAMES}, densify.DensifyConfig(absgrad=flag),
                              stats=TorchStats())
        d.after_train(0, grad, radii, (8, 8), absgrad=absg)
        runs[flag] = d.stats.xys_grad_norm.clone()
    by_hand = TorchStats()
    by_hand.update(absg, radii, (8, 8), step=0)
    assert torch.equal(runs[True], by_hand.xys_grad_norm) and not torch.equal(runs[True], runs[False])
    by_hand = TorchStats()
    by_hand.update(grad, radii, (8, 8), step=0)
    assert torch.equal(runs[False], by_hand.xys_grad_norm)
    d = densify.Densifier(P, {k: None for k in densify.PARAM_NAMES}, densify.DensifyConfig(absgrad=True),
                          stats=TorchStats())
    with pytest.raises(ValueError, match="absgrad"):
        d.after_train(0, grad, radii, (8, 8))
    d.after_train(0, None, radii, (8, 8))          # a view that saw nothing: zeros, as without absgrad
    assert float(d.stats.xys_grad_norm.abs().max()) == 0.0

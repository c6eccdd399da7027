"""CPU: the refinement entry points (include/sgn_rast.h, csrc/densify.hip) are exported, reject bad arguments with
rc < 0 and a message before touching the device, return 0 for n == 0, and `Densifier(engine=...)` refuses an unknown
engine and — for "hip" — CPU tensors (no fallback)."""
import ctypes
import os

import pytest
import torch

from sgn_rast import _lib, densify


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: every case below fails its argument check first (or n == 0)
NAMES = ("sgn_densify_workspace_bytes", "sgn_densify_decide", "sgn_densify_scan", "sgn_densify_apply")


def test_entries_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name)
    for name in NAMES[1:]:
        assert _lib.SIGNATURES[name][1][-1] is ctypes.c_void_p      # stream last
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [1, 20, 5, 18]


def _decide(lib, n, grad=FAKE, vis=FAKE, m2d=FAKE, ls=FAKE, op=FAKE, dim=96.0, samps=2, densify=1, screen=1, big=1,
            ws=FAKE, ws_bytes=None):
    need = lib.sgn_densify_workspace_bytes(max(n, 1)) if ws_bytes is None else ws_bytes
    return lib.sgn_densify_decide(n, grad, vis, m2d, ls, op, 2e-4, 0.01, 0.05, 0.1, 0.5, 0.15, dim, samps, densify,
                                  screen, big, ws, need, None)


def _apply(lib, n, n_out, samps=2, count=1, row=3, role=0, inputs=True, src=FAKE, kind=FAKE, ws=FAKE, ws_bytes=None,
           alias=False, quats=FAKE, noise_rows=4):
    need = lib.sgn_densify_workspace_bytes(max(n, 1)) if ws_bytes is None else ws_bytes
    ins = (ctypes.c_void_p * max(count, 1))(*[0x1000] * max(count, 1))
    outs = (ctypes.c_void_p * max(count, 1))(*[0x1000 if alias else 0x2000] * max(count, 1))
    rows = (ctypes.c_int32 * max(count, 1))(*[row] * max(count, 1))
    roles = (ctypes.c_int32 * max(count, 1))(*[role] * max(count, 1))
    return lib.sgn_densify_apply(n, n_out, samps, noise_rows, FAKE, FAKE, quats, FAKE, count, ins if inputs else None,
                                 outs, rows, roles, src, kind, ws, need, None)


def test_workspace_size(lib):
    ns = (1, 63, 64, 65, 255, 256, 257, 1000, 200_003, 1 << 20, 1 << 24)
    sizes = [lib.sgn_densify_workspace_bytes(n) for n in ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    # a flag byte per row, eight int32 per block of 256 rows, the eight totals
    assert all(s >= n + (n + 255) // 256 * 32 + 32 for s, n in zip(sizes, ns))
    assert lib.sgn_densify_workspace_bytes(0) == 0 and lib.sgn_densify_workspace_bytes(-3) == 0


def test_n_zero_returns_zero_without_pointers(lib):
    assert lib.sgn_densify_decide(0, None, None, None, None, None, 2e-4, 0.01, 0.05, 0.1, 0.5, 0.15, 96.0, 2, 1, 1, 1,
                                  None, 0, None) == 0
    assert lib.sgn_densify_scan(0, None, 0, None, None) == 0
    assert lib.sgn_densify_apply(0, 0, 2, 0, None, None, None, None, 0, None, None, None, None, None, None, None, 0,
                                 None) == 0
    # every row culled: nothing to write, no launch with an empty grid
    assert lib.sgn_densify_apply(100, 0, 2, 0, None, None, None, None, 0, None, None, None, None, None, None, None, 0,
                                 None) == 0


@pytest.mark.parametrize("kw,what", [
    (dict(n=-1), b"n >= 0"), (dict(n=100, samps=0), b"n_split_samples"), (dict(n=100, samps=65), b"n_split_samples"),
    (dict(n=1 << 30, samps=2), b"INT32_MAX"), (dict(n=100, ls=None), b"log_scales"),
    (dict(n=100, op=None), b"opacity_logits"), (dict(n=100, ws=None), b"ws"), (dict(n=100, grad=None), b"xys_grad_norm"),
    (dict(n=100, vis=None), b"vis_counts"), (dict(n=100, m2d=None), b"max_2dsize"), (dict(n=100, dim=0.0), b"image_dim"),
    (dict(n=100, ws_bytes=10), b"ws_bytes")])
def test_decide_rejects_bad_arguments(lib, kw, what):
    rc = _decide(lib, **kw)
    assert rc < 0
    assert what in lib.sgn_last_error()


def test_decide_optional_statistics(lib):
    # the cull-only refinement needs no gradient statistics, and no screen size without the screen-size tests: these
    # pass the pointer checks and fail on the workspace size that is checked last
    assert _decide(lib, 100, grad=None, vis=None, densify=0, ws_bytes=10) == -5
    assert _decide(lib, 100, grad=None, vis=None, m2d=None, densify=0, screen=0, ws_bytes=10) == -5
    assert _decide(lib, 100, m2d=None, densify=0, screen=1, ws_bytes=10) == -3


@pytest.mark.parametrize("args,what", [((-1, FAKE, None, FAKE), b"n >= 0"), ((100, None, None, FAKE), b"ws"),
                                       ((100, FAKE, None, None), b"totals8"), ((100, FAKE, 10, FAKE), b"ws_bytes")])
def test_scan_rejects_bad_arguments(lib, args, what):
    n, ws, ws_bytes, totals = args
    need = lib.sgn_densify_workspace_bytes(max(n, 1)) if ws_bytes is None else ws_bytes
    rc = lib.sgn_densify_scan(n, ws, need, totals, None)
    assert rc < 0
    assert what in lib.sgn_last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(n=-1, n_out=5), b"n >= 0"), (dict(n=100, n_out=-5), b"n_out >= 0"), (dict(n=100, n_out=401), b"n_out <="),
    (dict(n=100, n_out=5, samps=0), b"n_split_samples"), (dict(n=100, n_out=5, count=25), b"count"),
    (dict(n=100, n_out=5, noise_rows=-1), b"noise_rows"), (dict(n=100, n_out=5, src=None), b"src"),
    (dict(n=100, n_out=5, kind=None), b"kind"), (dict(n=100, n_out=5, ws=None), b"ws"),
    (dict(n=100, n_out=5, inputs=False), b"inputs"), (dict(n=100, n_out=5, ws_bytes=10), b"ws_bytes"),
    (dict(n=100, n_out=5, alias=True), b"inputs[i] != outputs[i]"), (dict(n=100, n_out=5, row=0), b"row_floats"),
    (dict(n=100, n_out=5, role=4), b"roles"), (dict(n=100, n_out=5, role=1, row=4), b"row_floats[i] == 3"),
    (dict(n=100, n_out=5, role=1, quats=ctypes.c_void_p(0x1004)), b"quats")])
def test_apply_rejects_bad_arguments(lib, kw, what):
    rc = _apply(lib, **kw)
    assert rc < 0
    assert what in lib.sgn_last_error()


def _cpu_world(n=8):
    g = torch.Generator().manual_seed(0)
    shapes = dict(means=(n, 3), log_scales=(n, 3), quats=(n, 4), features_dc=(n, 1, 3), features_rest=(n, 3, 3),
                  opacity_logits=(n, 1))
    P = {k: torch.randn(s, generator=g).requires_grad_(True) for k, s in shapes.items()}
    return P, {k: torch.optim.Adam([P[k]], lr=1e-3) for k in P}


def test_unknown_engine_raises():
    P, opts = _cpu_world()
    with pytest.raises(ValueError, match="engine"):
        densify.Densifier(P, opts, engine="triton")
    with pytest.raises(ValueError, match="engine"):
        densify.SceneGraphDensifier([P], opts, engine="eager")
    assert densify.Densifier(P, opts).engine == "torch"                   # the default stays the torch engine


def test_hip_engine_refuses_cpu_tensors():
    P, opts = _cpu_world()
    with pytest.raises(_lib.SgnRastError, match="no CPU fallback"):
        densify.Densifier(P, opts, engine="hip")
    with pytest.raises(_lib.SgnRastError, match="no CPU fallback"):
        densify.SceneGraphDensifier([P], opts, engine="hip")
    # ... and an engine handed CPU tensors later does not fall back either
    D = densify.Densifier(P, opts, densify.DensifyConfig(warmup_length=0, refine_every=10, reset_alpha_every=3))
    D.engine = "hip"
    D.stats.xys_grad_norm, D.stats.vis_counts, D.stats.max_2Dsize = torch.ones(8), torch.ones(8), torch.zeros(8)
    with pytest.raises(_lib.SgnRastError, match="no CPU fallback"):
        D.refinement_after(15)
    assert D.params["means"].shape[0] == 8

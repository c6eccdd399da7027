"""CPU: the MCMC refinement entry points (include/sgn_rast.h, csrc/mcmc.hip) are exported, reject bad arguments with
every documented return code and a message before touching the device, return 0 for n == 0 / k == 0 without a launch,
and ``MCMCDensifier(engine="hip")`` refuses CPU tensors (no fallback)."""
import ctypes
import os

import pytest
import torch

from sgn_rast import _lib, mcmc

FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: every case below fails its argument check first (or n == 0)
NAMES = ("sgn_mcmc_workspace_bytes", "sgn_mcmc_weights", "sgn_mcmc_scan", "sgn_mcmc_draw", "sgn_mcmc_relocation",
         "sgn_mcmc_apply", "sgn_mcmc_noise")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


def test_entries_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name)
    for name in NAMES[1:]:
        assert _lib.SIGNATURES[name][1][-1] is ctypes.c_void_p      # stream last
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [1, 9, 9, 10, 9, 14, 9]


def test_workspace_size(lib):
    ns = (1, 255, 256, 257, 70_001, 1 << 20, 1 << 24)
    sizes = [lib.sgn_mcmc_workspace_bytes(n) for n in ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    # two int32 per row, an int64 and an int32 per block of 256 rows, two int64 totals
    assert all(s >= 8 * n + (n + 255) // 256 * 12 + 16 for s, n in zip(sizes, ns))
    assert lib.sgn_mcmc_workspace_bytes(0) == 0 and lib.sgn_mcmc_workspace_bytes(-3) == 0


def test_empty_calls_return_zero_without_pointers(lib):
    assert lib.sgn_mcmc_weights(0, None, 0.005, 1, None, None, None, 0, None) == 0
    assert lib.sgn_mcmc_scan(0, None, None, None, None, None, 0, None, None) == 0
    assert lib.sgn_mcmc_draw(0, 5, 1, 51, None, None, None, None, 0, None) == 0
    assert lib.sgn_mcmc_draw(100, 0, 1, 51, None, None, None, None, 0, None) == 0
    assert lib.sgn_mcmc_relocation(0, 5, None, None, 0.005, None, None, None, None) == 0
    assert lib.sgn_mcmc_relocation(100, 0, None, None, 0.005, None, None, None, None) == 0
    assert lib.sgn_mcmc_apply(0, 100, 0, None, None, None, 0, None, None, None, None, None, 0, None) == 0
    assert lib.sgn_mcmc_apply(1, 0, 0, None, None, None, 0, None, None, None, None, None, 0, None) == 0
    assert lib.sgn_mcmc_noise(0, 1, 1.0, None, None, None, None, None, None) == 0


def _need(lib, n, ws_bytes):
    return lib.sgn_mcmc_workspace_bytes(max(n, 1)) if ws_bytes is None else ws_bytes


def _weights(lib, n=100, logits=FAKE, w=FAKE, dead=FAKE, ws=FAKE, ws_bytes=None):
    return lib.sgn_mcmc_weights(n, logits, 0.005, 1, w, dead, ws, _need(lib, n, ws_bytes), None)


def _scan(lib, n=100, w=FAKE, dead=FAKE, prefix=FAKE, rows=FAKE, ws=FAKE, ws_bytes=None, totals=FAKE):
    return lib.sgn_mcmc_scan(n, w, dead, prefix, rows, ws, _need(lib, n, ws_bytes), totals, None)


def _draw(lib, n=100, k=10, n_max=51, prefix=FAKE, src=FAKE, ratio=FAKE, ws=FAKE, ws_bytes=None):
    return lib.sgn_mcmc_draw(n, k, 12345, n_max, prefix, src, ratio, ws, _need(lib, n, ws_bytes), None)


def _relocation(lib, n=100, k=10, logits=FAKE, ls=FAKE, src=FAKE, ratio=FAKE, staging=FAKE):
    return lib.sgn_mcmc_relocation(n, k, logits, ls, 0.005, src, ratio, staging, None)


def _apply(lib, mode=0, n=100, k=10, src=FAKE, targets=FAKE, staging=FAKE, count=1, row=3, role=0, inputs=True,
           alias=None, ws=FAKE, ws_bytes=None, null_entry=False):
    alias = (mode == 0) if alias is None else alias
    m = max(count, 1)
    ins = (ctypes.c_void_p * m)(*[None if null_entry else 0x1000] * m)
    outs = (ctypes.c_void_p * m)(*[0x1000 if alias else 0x2000] * m)
    rows = (ctypes.c_int32 * m)(*[row] * m)
    roles = (ctypes.c_int32 * m)(*[role] * m)
    return lib.sgn_mcmc_apply(mode, n, k, src, targets, staging, count, ins if inputs else None, outs, rows, roles, ws,
                              _need(lib, n, ws_bytes), None)


def _noise(lib, n=100, means=FAKE, ls=FAKE, quats=FAKE, logits=FAKE):
    return lib.sgn_mcmc_noise(n, 1, 1.0, means, ls, quats, logits, None, None)


@pytest.mark.parametrize("fn,kw,rc,what", [
    (_weights, dict(n=-1), -1, b"n >= 0"), (_weights, dict(logits=None), -3, b"opacity_logits"),
    (_weights, dict(w=None), -3, b"w"), (_weights, dict(dead=None), -3, b"dead"), (_weights, dict(ws=None), -3, b"ws"),
    (_weights, dict(ws_bytes=10), -5, b"ws_bytes"),
    (_scan, dict(n=-1), -1, b"n >= 0"), (_scan, dict(prefix=None), -3, b"prefix"),
    (_scan, dict(rows=None), -3, b"dead_rows"), (_scan, dict(totals=None), -3, b"totals2"),
    (_scan, dict(ws_bytes=10), -5, b"ws_bytes"),
    (_draw, dict(n=-1), -1, b"n >= 0"), (_draw, dict(k=-1), -1, b"k >= 0"),
    (_draw, dict(n=1 << 30, k=(1 << 30) + 5), -1, b"INT32_MAX"), (_draw, dict(n_max=0), -2, b"n_max"),
    (_draw, dict(n_max=52), -2, b"n_max"), (_draw, dict(prefix=None), -3, b"prefix"), (_draw, dict(src=None), -3, b"src"),
    (_draw, dict(ratio=None), -3, b"ratio"), (_draw, dict(ws_bytes=10), -5, b"ws_bytes"),
    (_relocation, dict(n=-1), -1, b"n >= 0"), (_relocation, dict(ls=None), -3, b"log_scales"),
    (_relocation, dict(staging=None), -3, b"staging"), (_relocation, dict(src=None), -3, b"src"),
    (_apply, dict(mode=2), -4, b"mode"), (_apply, dict(n=-1), -1, b"n >= 0"), (_apply, dict(k=101), -1, b"k <= n"),
    (_apply, dict(count=25), -6, b"count"), (_apply, dict(src=None), -3, b"src"),
    (_apply, dict(targets=None), -3, b"targets"), (_apply, dict(staging=None), -3, b"staging"),
    (_apply, dict(inputs=False), -3, b"inputs"), (_apply, dict(null_entry=True), -3, b"inputs[i]"),
    (_apply, dict(mode=0, alias=False), -3, b"inputs[i] == outputs[i]"),
    (_apply, dict(mode=1, alias=True), -3, b"inputs[i] != outputs[i]"), (_apply, dict(row=0), -6, b"row_floats"),
    (_apply, dict(role=4), -6, b"roles"), (_apply, dict(role=1, row=3), -6, b"row_floats[i] == 1"),
    (_apply, dict(role=2, row=4), -6, b"row_floats[i] == 3"), (_apply, dict(ws_bytes=10), -5, b"ws_bytes"),
    (_noise, dict(n=-1), -1, b"n >= 0"), (_noise, dict(means=None), -3, b"means"),
    (_noise, dict(quats=ctypes.c_void_p(0x1004)), -7, b"quats")])
def test_bad_arguments_are_rejected_with_the_documented_code(lib, fn, kw, rc, what):
    assert fn(lib, **kw) == rc
    assert what in lib.sgn_last_error()


def test_grow_needs_no_targets(lib):
    # the grow mode ignores `targets`: a NULL passes the pointer checks and fails on the workspace size checked last
    assert _apply(lib, mode=1, targets=None, ws_bytes=10) == -5


def _cpu_world(n=8):
    g = torch.Generator().manual_seed(0)
    shapes = dict(means=(n, 3), log_scales=(n, 3), quats=(n, 4), features_dc=(n, 1, 3), features_rest=(n, 3, 3),
                  opacity_logits=(n, 1))
    P = {k: torch.randn(s, generator=g).requires_grad_(True) for k, s in shapes.items()}
    return P, {k: torch.optim.Adam([P[k]], lr=1e-3) for k in P}


def test_hip_engine_refuses_cpu_tensors():
    P, opts = _cpu_world()
    with pytest.raises(_lib.SgnRastError, match="no CPU fallback"):
        mcmc.MCMCDensifier(P, opts, engine="hip")
    D = mcmc.MCMCDensifier(P, opts, mcmc.MCMCConfig(warmup_length=0, refine_every=10))
    D.engine = "hip"                        # an engine handed CPU tensors later does not fall back either
    with pytest.raises(_lib.SgnRastError, match="no CPU fallback"):
        D.refinement_after(10)
    with pytest.raises(_lib.SgnRastError, match="no CPU fallback"):
        D.inject_noise(3)
    assert D.params["means"].shape[0] == 8

"""GPU: the one-call entries (sgn_rasterize_fwd_all, sgn_rasterize_window_all, sgn_rasterize_views_fwd_all) called through
ctypes the way a non-Python host would, on EVERY transport of their one-word read-back — a pinned (mapped, polled) word,
no pinned word at all (pageable copy + event), a pinned word with the `extra` word riding along — and on a capacity
miss: same list, bins, image and per-pixel state whichever way the word travelled, equal to the call-by-call operator
path, exactly one host wait per call; plus the arena sizes as constants."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H, W, BLOCK = 40, 64, 16                 # 4 x 3 tiles, the last tile row ragged (40 = 2 * 16 + 8)
TILES = 12
CAP = 5000                               # >= 300 Gaussians x 12 tiles
E_CAPACITY = -100


def _scene(n, seed=11):
    """Screen-space splats on the CPU (fixed seed).  n >= 3: row 0 covers the whole image, row 1 can never reach alpha
    1/255 (culled from every tile its box touches), row 2 has radius 0.  n = 1: one splat on a tile corner (4 tiles)."""
    g = torch.Generator().manual_seed(seed)
    xys = torch.rand(n, 2, generator=g) * torch.tensor([float(W), float(H)])
    sigma = 0.8 + 3.0 * torch.rand(n, generator=g)
    opac = 0.2 + 0.7 * torch.rand(n, generator=g)
    if n >= 3:
        xys[0], sigma[0] = torch.tensor([32.0, 20.0]), 12.0
        xys[1], sigma[1], opac[1] = torch.tensor([30.0, 18.0]), 4.0, 1e-4
    else:
        xys[0], sigma[0] = torch.tensor([16.0, 16.0]), 3.0
    radii = torch.ceil(3.0 * sigma).to(torch.int32)
    if n >= 3:
        radii[2] = 0
    conics = torch.stack([1.0 / sigma ** 2, 0.1 * (torch.rand(n, generator=g) - 0.5) / sigma ** 2, 1.0 / sigma ** 2], 1)
    r = radii.float()[:, None]
    lo = ((xys - r) / BLOCK).to(torch.int32).clamp(min=0)
    hi = ((xys + r) / BLOCK + 1.0).to(torch.int32)
    grid = torch.tensor([W // BLOCK, (H + BLOCK - 1) // BLOCK], dtype=torch.int32)
    lo, hi = torch.minimum(lo, grid), torch.minimum(hi.clamp(min=0), grid)
    nth = ((hi - lo).clamp(min=0).prod(1) * (radii > 0)).to(torch.int32)
    sc = dict(xys=xys, depths=1.0 + 9.0 * torch.rand(n, generator=g), radii=radii, conics=conics, nth=nth,
              colors=torch.rand(n, 3, generator=g), opac=opac, bg=torch.tensor([0.1, 0.2, 0.3]))
    return {k: v.contiguous().to(DEV) for k, v in sc.items()}


def _waits(lib, reset=False):
    n = C.c_int64(0)
    lib.sgn_timing_host_wait_us(int(reset), C.byref(n))
    return n.value


def _scratch(lib, n_tiles):
    return torch.zeros(int(lib.sgn_tile_order_scratch_bytes(n_tiles)) // 4, dtype=torch.int32, device=DEV)


def _fwd_all(lib, L, sc, cap, transport, qmask, ro):
    """One sgn_rasterize_fwd_all call; transport: "pinned" | "pageable" | "extra"."""
    n = sc["xys"].shape[0]
    i32, f32 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float32, device=DEV)
    img, Ts, idx = torch.empty(H, W, 3, **f32), torch.empty(H, W, **f32), torch.empty(H, W, **i32)
    ids = torch.empty(cap, **i32)
    bins_and_stats = torch.empty(2, TILES, 2, **i32)
    order = torch.empty(TILES + 2, **i32)
    rows = L.workspace(lib.sgn_raster_workspace_bytes(n, 0, C.byref(ro)), DEV)
    arena = L.workspace(lib.sgn_rasterize_arena_bytes(n, cap), DEV)
    scratch = _scratch(lib, TILES)
    pinned = torch.zeros(8, dtype=torch.int32).pin_memory()
    extra_dev = torch.tensor([4242], **i32)
    n_host = C.c_int64(-7)
    torch.cuda.synchronize()
    _waits(lib, reset=True)
    rc = lib.sgn_rasterize_fwd_all(
        n, L.ptr(sc["xys"]), L.ptr(sc["depths"]), L.ptr(sc["radii"]), L.ptr(sc["conics"]), L.ptr(sc["colors"]),
        L.ptr(sc["opac"]), 0, 1, H, W, BLOCK, L.ptr(sc["bg"]), None, int(qmask), L.ptr(img), L.ptr(Ts), L.ptr(idx), None,
        L.ptr(ids), cap, L.ptr(bins_and_stats[0]), L.ptr(order), L.ptr(bins_and_stats[1]), L.ptr(rows), rows.numel(),
        L.ptr(scratch), 4 * scratch.numel(), L.ptr(arena), arena.numel(),
        None if transport == "pageable" else pinned[0:1].data_ptr(),
        L.ptr(extra_dev) if transport == "extra" else None, pinned[7:8].data_ptr() if transport == "extra" else None,
        C.byref(n_host), L.sort_rank_mode(), 0, C.byref(ro), L.stream_ptr())
    waits = _waits(lib)
    torch.cuda.synchronize()
    count = int(n_host.value)
    return dict(rc=rc, waits=waits, count=count, ids=ids[:max(min(count, cap), 0)].clone(), bins=bins_and_stats[0].clone(),
                img=img, Ts=Ts, idx=idx, extra=int(pinned[7]))


def _same(a, b, what):
    assert a["count"] == b["count"], what
    for k in ("ids", "bins", "img", "Ts", "idx"):
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module")
def lib():
    from sgn_rast import _lib as L
    return L.load()


@pytest.fixture(scope="module", params=[300, 1])
def served(request, lib):
    """The scene, the call-by-call operator path's results on it, and the three transports' results."""
    from sgn_rast import _lib as L, config, ops
    sc = _scene(request.param)
    old = (ops.composite_forward, ops.composite_backward)
    defaults = {name: row[0] for name, row in config.OPTIONS.items() if not any(mod == "opts" for mod, _a in row[2])}
    with config.override(**defaults), L.options(exact_exp=1):
        ro = L.opts().copy()
        try:
            ops.composite_forward = ops.composite_backward = False
            ops.clear_binning_cache()
            ops._depth_state.update(want=False, unused=0)
            assert ops.tile_culling_enabled
            colors = sc["colors"].clone().requires_grad_(True)
            img, _alpha = ops.rasterize_gaussians(sc["xys"], sc["depths"], sc["radii"], sc["conics"], sc["nth"], colors,
                                                  sc["opac"], H, W, BLOCK, sc["bg"], True)
            sv = img.grad_fn.saved_tensors
            qmask = bool(getattr(sv[0], "_sgn_qmask", False)) or bool(img.grad_fn.ro.ids_qmask)
            ref = dict(count=int(sv[0].shape[0]), ids=sv[0].clone(), bins=sv[1].clone(), img=img.detach().clone(),
                       Ts=sv[7].clone(), idx=sv[8].clone())
        finally:
            ops.composite_forward, ops.composite_backward = old
            ops.clear_binning_cache()
        got = {t: _fwd_all(lib, L, sc, CAP, t, qmask, ro) for t in ("pinned", "pageable", "extra")}
        yield dict(sc=sc, ref=ref, got=got, qmask=qmask, ro=ro, L=L)


def test_scene_has_a_wide_and_a_culled_splat(served):
    if served["sc"]["xys"].shape[0] == 1:
        assert served["ref"]["count"] >= 2           # the one splat sits on a tile corner (half of it is a capacity)
        return
    ids = served["ref"]["ids"] & ((1 << 28) - 1)
    assert int((ids == 0).sum()) > 1                 # row 0 spans several tiles (its box covers all twelve)
    assert int(served["sc"]["nth"][1]) > 1 and int((ids == 1).sum()) == 0      # row 1: a box over several tiles, all culled
    assert int((ids == 2).sum()) == 0                # radius 0


def test_forward_is_the_same_on_every_transport(served):
    got, ref = served["got"], served["ref"]
    for t, r in got.items():
        assert r["rc"] == 0 and r["count"] >= 1, t
        assert r["waits"] == 1, (t, r["waits"])                  # one host wait per call, whichever way the count came
        _same(r, got["pinned"], t)
        _same(r, ref, t + " vs call-by-call")
    assert got["extra"]["extra"] == 4242 and got["pinned"]["extra"] == 0


@pytest.mark.parametrize("transport", ["pinned", "pageable"])
def test_capacity_miss_reports_the_count_and_a_retry_succeeds(served, lib, transport):
    true = served["ref"]["count"]
    miss = _fwd_all(lib, served["L"], served["sc"], true // 2, transport, served["qmask"], served["ro"])
    assert miss["rc"] == E_CAPACITY and miss["count"] == true and miss["waits"] == 1
    again = _fwd_all(lib, served["L"], served["sc"], miss["count"], transport, served["qmask"], served["ro"])
    assert again["rc"] == 0 and again["waits"] == 1
    _same(again, served["ref"], transport)


def _window_all(lib, L, sc, full, qmask, ro, pinned_verdict, spoil=False):
    """sgn_rasterize_window_all over the tail window (the last 100 rows) of the 300-row scene's list."""
    n_full, n_win = sc["xys"].shape[0], 100
    lo = n_full - n_win
    w = {k: sc[k][lo:].clone() for k in ("xys", "depths", "radii", "nth", "conics", "colors", "opac")}
    if spoil:
        w["xys"][57, 1] += 0.5
    i32, f32 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float32, device=DEV)
    img, Ts, idx = torch.full((H, W, 3), -5.0, **f32), torch.full((H, W), -5.0, **f32), torch.full((H, W), -5, **i32)
    ids_out, bins_out = torch.empty_like(full["ids"]), torch.empty_like(full["bins"])
    order, stats = torch.empty(TILES + 2, **i32), torch.empty(TILES, 2, **i32)
    rows = L.workspace(lib.sgn_raster_workspace_bytes(n_full, 0, C.byref(ro)), DEV)
    arena = L.workspace(lib.sgn_rasterize_window_arena_bytes(TILES), DEV)
    scratch = _scratch(lib, TILES)
    pinned = torch.zeros(8, dtype=torch.int32).pin_memory()
    cands = (C.c_int32 * 2)(0, lo)
    matched = C.c_int(-9)
    torch.cuda.synchronize()
    _waits(lib, reset=True)
    rc = lib.sgn_rasterize_window_all(
        n_win, n_full, 2, cands, L.ptr(w["xys"]), L.ptr(w["depths"]), L.ptr(w["radii"]), L.ptr(w["nth"]),
        L.ptr(w["conics"]), L.ptr(w["colors"]), L.ptr(w["opac"]), 0, L.ptr(sc["xys"]), L.ptr(sc["depths"]),
        L.ptr(sc["radii"]), L.ptr(sc["nth"]), L.ptr(sc["conics"]), L.ptr(sc["opac"]), full["count"], L.ptr(full["ids"]),
        L.ptr(full["bins"]), int(qmask), H, W, BLOCK, L.ptr(sc["bg"]), 1, None, L.ptr(img), L.ptr(Ts), L.ptr(idx),
        L.ptr(ids_out), L.ptr(bins_out), L.ptr(order), L.ptr(stats), L.ptr(rows), rows.numel(), L.ptr(scratch),
        4 * scratch.numel(), L.ptr(arena), arena.numel(), pinned.data_ptr() if pinned_verdict else None,
        C.byref(matched), C.byref(ro), L.stream_ptr())
    waits = _waits(lib)
    torch.cuda.synchronize()
    return dict(rc=rc, waits=waits, lo=matched.value, img=img, Ts=Ts, idx=idx)


def test_window_verdict_on_both_transports(served, lib):
    if served["sc"]["xys"].shape[0] != 300:
        return
    L, sc, full, qmask, ro = served["L"], served["sc"], served["got"]["pinned"], served["qmask"], served["ro"]
    a = _window_all(lib, L, sc, full, qmask, ro, pinned_verdict=True)
    b = _window_all(lib, L, sc, full, qmask, ro, pinned_verdict=False)
    for r in (a, b):
        assert r["rc"] == 0 and r["lo"] == 200 and r["waits"] == 1
        assert float(r["img"].min()) >= 0.0 and float(r["Ts"].min()) >= 0.0          # every pixel was written
    for k in ("img", "Ts", "idx"):
        assert torch.equal(a[k], b[k]), k
    for pinned_verdict in (True, False):
        r = _window_all(lib, L, sc, full, qmask, ro, pinned_verdict, spoil=True)
        assert r["rc"] == 0 and r["lo"] == -1 and r["waits"] == 1
        assert bool((r["img"] == -5.0).all()) and bool((r["Ts"] == -5.0).all()) and bool((r["idx"] == -5).all())


def _views_all(lib, L, sc, qmask, ro, pinned_count):
    b, n = 2, sc["xys"].shape[0]
    r, tiles, cap = b * n, 2 * TILES, 2 * CAP
    i32, f32 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float32, device=DEV)
    xys = torch.cat([sc["xys"], sc["xys"] + torch.tensor([3.5, -2.25], device=DEV)]).contiguous()
    rep = {k: torch.cat([sc[k], sc[k]]).contiguous() for k in ("depths", "radii", "conics", "colors")}
    logits = torch.logit(sc["opac"]).contiguous()
    img, Ts, idx = torch.empty(b, H, W, 3, **f32), torch.empty(b, H, W, **f32), torch.empty(b, H, W, **i32)
    ids = torch.empty(cap, **i32)
    bins_and_stats = torch.empty(2, tiles, 2, **i32)
    order = torch.empty(tiles + 2, **i32)
    rows = L.workspace(lib.sgn_raster_workspace_bytes(r, 0, None), DEV)
    arena = L.workspace(lib.sgn_rasterize_views_arena_bytes(b, n, cap), DEV)
    scratch = _scratch(lib, tiles)
    pinned = torch.zeros(8, dtype=torch.int32).pin_memory()
    n_host = C.c_int64(-7)
    torch.cuda.synchronize()
    _waits(lib, reset=True)
    rc = lib.sgn_rasterize_views_fwd_all(
        b, n, L.ptr(xys), L.ptr(rep["depths"]), L.ptr(rep["radii"]), L.ptr(rep["conics"]), L.ptr(rep["colors"]),
        L.ptr(logits), 1, H, W, BLOCK, L.ptr(sc["bg"]), int(qmask), L.ptr(img), L.ptr(Ts), L.ptr(idx), None, L.ptr(ids),
        cap, L.ptr(bins_and_stats[0]), L.ptr(order), L.ptr(bins_and_stats[1]), L.ptr(rows), rows.numel(), L.ptr(scratch),
        4 * scratch.numel(), L.ptr(arena), arena.numel(), pinned.data_ptr() if pinned_count else None, C.byref(n_host),
        L.sort_rank_mode(), 0, C.byref(ro), L.stream_ptr())
    waits = _waits(lib)
    torch.cuda.synchronize()
    count = int(n_host.value)
    return dict(rc=rc, waits=waits, count=count, ids=ids[:max(count, 0)].clone(), bins=bins_and_stats[0].clone(), img=img,
                Ts=Ts, idx=idx)


def test_views_forward_on_both_transports(served, lib):
    if served["sc"]["xys"].shape[0] != 300:
        return
    a = _views_all(lib, served["L"], served["sc"], served["qmask"], served["ro"], pinned_count=True)
    b = _views_all(lib, served["L"], served["sc"], served["qmask"], served["ro"], pinned_count=False)
    for r in (a, b):
        assert r["rc"] == 0 and r["waits"] == 1 and r["count"] > served["ref"]["count"]
    _same(a, b, "views")


def test_arena_sizes(lib):
    """Recorded from the commit before the arenas' size and layout became one function."""
    assert lib.sgn_rasterize_arena_bytes(1, 1) == 8448
    assert lib.sgn_rasterize_arena_bytes(300, 5000) == 131072
    assert lib.sgn_rasterize_views_arena_bytes(2, 300, 5000) == 154624
    assert lib.sgn_rasterize_window_arena_bytes(12) == 768

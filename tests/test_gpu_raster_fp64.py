"""GPU (-m gpu): the rasterizer per pixel and per Gaussian against the float64 definition of tests/raster_fp64.py, on every
kernel route — forward: two- / four-wave packed kernel, LDS-batched walk, the linear-mapping kernel of blocks 8 and 5;
backward: MODE 0, the two-kernel scheme, staged walk and scalar chase, both wave reductions; the quadrant-mask and
tile-culling skips; exact and hardware exp; the unpack kernel's sigmoid chain and clamped-colour mask; id ranges with and
without a list window; the depth channel; batched views; both backward clamps.

Every row that is not threshold-adjacent and every pixel that is not is held, per component, to
    |got - exp| <= K 2^-24 (sum of the absolute values of its terms),     exactly 0.0 where that sum is 0,
with K derived on the CPU (tests/test_raster_fp64.py: 4 x the worst ratio of a float32 emulation of the definition and of
the C oracle, which that test holds to the same bound).  Adjacent pixels may differ by one flipped entry.  One 40 x 56
scene (330 Gaussians), one reference per (block, clamp, id range, opacity form), shared by the cases."""
import numpy as np
import pytest
import torch

import raster_fp64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(adapt_bwd=16, batch_bwd=8)        # this size reaches the long-walk kernel and the LDS-staged walk
RO_FIELDS = ("reduce_mode", "adapt_fwd", "adapt_bwd", "batch_fwd", "batch_bwd", "exact_exp")


@pytest.fixture(scope="module", autouse=True)
def _host_state_untouched():
    """The host layer keeps per-stream policy state that outlives a call — the walked-entries statistic behind the
    quadrant-mask policy and the phase of its every-eighth-binning read-back, the depth channel's "auto" counters, the
    capacity estimates — and some sixty tiny renders would shift all of it for every module that runs afterwards.  This
    module runs on state objects of its own and puts the earlier ones back."""
    from sgn_rast import ops, views
    torch.cuda.synchronize()
    saved = (list(ops._states.items()), list(views._STATES.items()), dict(ops.quadrant_mask_stats))
    ops._states.clear()
    views._STATES.clear()
    yield
    torch.cuda.synchronize()
    ops._states.clear()
    ops._states.update(saved[0])
    views._STATES.clear()
    views._STATES.update(saved[1])
    ops.quadrant_mask_stats.update(saved[2])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _check(what, got, ref, table, keep_rows=None, keep_px=None, exp=None, scale=None):
    """Every output of `got` against `ref` (`exp` / `scale`: overrides per name); prints the worst ratio per output, then
    asserts.  -> {name: ratio}"""
    keep_rows = ~ref.adjacent if keep_rows is None else keep_rows
    keep_px = ~ref.adjacent_px if keep_px is None else keep_px
    worst, bad = {}, []
    for name, value in got.items():
        pixel = name in R.PIXEL_OUTPUTS
        k = table[{"v_colors_pre": "v_colors"}.get(name, name)]
        e, s = (exp or {}).get(name), (scale or {}).get(name)
        ratio, nonzero = R.compare(value, ref, name, keep_px if pixel else keep_rows, s, e)
        worst[name] = ratio
        if not ratio <= k:
            bad.append((name, "ratio", ratio, "K", k))
        if nonzero:
            bad.append((name, "elements with an absolute sum of 0 that are not exactly 0.0", nonzero))
        if pixel and (~keep_px).any():
            # a threshold-adjacent pixel: one flipped entry, alpha <= 1/255 + 1e-5, times the largest colour / depth
            e_ = ref.val[name] if e is None else e
            s_ = ref.scale[name] if s is None else s
            top = {"img": 1.0, "alpha": 1.0, "depth": ref.depth_max}[name]
            err = np.abs(np.asarray(value, np.float64).reshape(e_.shape) - e_)[~keep_px]
            lim = (1.0 / 255.0 + 1e-5) * top + k * R.EPS * s_[~keep_px]
            if not (err <= lim).all():
                bad.append((name, "adjacent pixel beyond one flipped entry", float(err.max())))
    print(f"[raster fp64 gpu] {what}: " + ", ".join(f"{n} {r:.1f}/{table[{'v_colors_pre': 'v_colors'}.get(n, n)]}"
                                                    for n, r in worst.items()))
    assert not bad, (what, bad)
    return worst


def _walks(fn):
    """(list length, reverse-walk length) per tile, from what the forward recorded for its node: the deepest list
    position any pixel of the tile composited is where the tile's reverse walk starts (as the launch order reads it)."""
    bins = fn.saved_tensors[1].cpu().long()
    lens = bins[:, 1] - bins[:, 0]
    walk = torch.minimum(lens, (fn.tile_kmax[:, 0].cpu().long() - bins[:, 0] + 1).clamp_min(0))
    return lens, walk


def _assert_route(fn, opts, want):
    """The options reached the node, and the scene sends tiles down the path the case is about.  (Before the backward:
    it frees what the node saved.)"""
    from sgn_rast import config
    for name, v in opts.items():
        if name in RO_FIELDS:
            assert getattr(fn.ro, name) == v, (name, getattr(fn.ro, name), v)
        else:
            assert config.current()[name] == v, name
    lens, walk = _walks(fn)
    ro = fn.ro
    if "qmask" in want:
        assert bool(ro.ids_qmask) == want["qmask"]
    if want.get("two_kernels"):                    # both the long-walk and the short-walk kernel have tiles
        assert bool((walk >= ro.adapt_bwd).any()) and bool(((walk > 0) & (walk < ro.adapt_bwd)).any()), walk.tolist()
    if want.get("staged_bwd"):
        assert bool((walk >= ro.batch_bwd).any())
    if want.get("scalar_bwd"):
        assert bool((walk < ro.batch_bwd).all())
    if want.get("four_waves"):
        assert bool((lens >= ro.adapt_fwd).any()) and bool(((lens > 0) & (lens < ro.adapt_fwd)).any()), lens.tolist()
    if want.get("two_waves"):
        assert bool((lens < ro.adapt_fwd).all())
    if want.get("batched_fwd"):
        assert bool((lens >= ro.batch_fwd).any())
    return lens, walk


def _leaves(sc, opacity):
    return [_t(sc.xys).requires_grad_(True), _t(sc.conics).requires_grad_(True), _t(sc.colors).requires_grad_(True),
            _t(opacity).requires_grad_(True)]


def _fused(sc, logit, id_range, depth, opts, want):
    """`fused.rasterize_gaussians_fused` on the scene's float32 arrays + the backward of the scene's loss
    -> (outputs dict, list length per tile)."""
    from sgn_rast import fused, ops
    xys, conics, colors, opac = lv = _leaves(sc, sc.logits if logit else sc.opacities)
    ops.clear_binning_cache()
    out = fused.rasterize_gaussians_fused(xys, _t(sc.depths), _t(sc.radii), conics, _t(sc.num_tiles_hit), colors, opac,
                                          sc.H, sc.W, sc.block, background=_t(sc.background), return_alpha=True,
                                          id_range=id_range, depth_channel=depth, opacity_is_logit=logit)
    lens, _walk = _assert_route(out[0].grad_fn, opts, want)
    ((out[0] * _t(sc.w_img)).sum() + (out[1] * _t(sc.w_alpha)).sum()).backward()
    torch.cuda.synchronize()
    got = dict(img=_np(out[0]), alpha=_np(out[1]), v_xy=_np(xys.grad), v_conic=_np(conics.grad),
               v_colors=_np(colors.grad))
    got["v_logit" if logit else "v_opacity"] = _np(opac.grad)
    if depth:
        got["depth"] = _np(out[2])
    return got, lens


# name: (block, options, clamp, what the route must show, table)
X1 = dict(exact_exp=1)
ROUTES = {
    # ---- forward: the packed kernel (block 16) two- / four-wave, scalar / LDS-batched, with and without launch order
    "fwd-defaults": (16, dict(X1), 0.99, dict(two_waves=True, scalar_bwd=True), "K"),
    "fwd-four-waves": (16, dict(X1, adapt_fwd=32), 0.99, dict(four_waves=True), "K"),
    "fwd-batched": (16, dict(X1, batch_fwd=8), 0.99, dict(batched_fwd=True, two_waves=True), "K"),
    "fwd-four-waves-batched": (16, dict(X1, adapt_fwd=32, batch_fwd=8), 0.99, dict(four_waves=True, batched_fwd=True), "K"),
    "fwd-four-waves-no-order": (16, dict(X1, adapt_fwd=32, batch_fwd=8, tile_order=False), 0.99,
                                dict(four_waves=True, batched_fwd=True), "K"),
    # ---- forward: raster_fwd_kernel (the linear pixel mapping); backward: MODE 0
    "block8": (8, dict(X1, **SMALL), 0.99, dict(staged_bwd=True), "K"),
    "block5": (5, dict(X1, **SMALL), 0.99, dict(staged_bwd=True), "K"),
    "block8-defaults": (8, dict(X1), 0.99, dict(scalar_bwd=True), "K"),
    # ---- backward launch shapes
    "bwd-mode0-no-order": (16, dict(X1, tile_order=False, **SMALL), 0.99, dict(staged_bwd=True), "K"),
    "bwd-two-kernels-staged": (16, dict(X1, **SMALL), 0.99, dict(two_kernels=True, staged_bwd=True), "K"),
    "bwd-two-kernels-scalar": (16, dict(X1, adapt_bwd=16), 0.99, dict(two_kernels=True, scalar_bwd=True), "K"),
    "bwd-two-kernels-butterfly": (16, dict(X1, reduce_mode=0, **SMALL), 0.99, dict(two_kernels=True), "K"),
    "bwd-mode0-butterfly": (16, dict(X1, reduce_mode=0, tile_order=False, **SMALL), 0.99, {}, "K"),
    "bwd-defaults-butterfly": (16, dict(X1, reduce_mode=0), 0.99, dict(scalar_bwd=True), "K"),
    "bwd-one-stream": (16, dict(X1, concurrent_backward=False, **SMALL), 0.99, dict(two_kernels=True), "K"),
    "bwd-call-by-call": (16, dict(X1, one_call_nodes=False, **SMALL), 0.99, dict(two_kernels=True), "K"),
    # ---- the skip tests, forward and backward
    "qmask-on": (16, dict(X1, quadrant_masks="on", **SMALL), 0.99, dict(qmask=True, two_kernels=True), "K"),
    "qmask-on-defaults": (16, dict(X1, quadrant_masks="on"), 0.99, dict(qmask=True), "K"),
    "qmask-on-mode0": (16, dict(X1, quadrant_masks="on", tile_order=False, **SMALL), 0.99, dict(qmask=True), "K"),
    "qmask-off": (16, dict(X1, quadrant_masks="off", **SMALL), 0.99, dict(qmask=False, two_kernels=True), "K"),
    "culling-off": (16, dict(X1, tile_culling=False, **SMALL), 0.99, dict(qmask=False, culled=False), "K"),
    "culling-off-block8": (8, dict(X1, tile_culling=False, **SMALL), 0.99, dict(culled=False), "K"),
    "culling-on": (16, dict(X1, tile_culling=True, quadrant_masks="off", **SMALL), 0.99, dict(culled=True), "K"),
    # ---- the hardware exp, with its own K
    "hw-exp-two-kernels": (16, dict(exact_exp=0, **SMALL), 0.99, dict(two_kernels=True), "K_HW"),
    "hw-exp-mode0": (16, dict(exact_exp=0, tile_order=False, **SMALL), 0.99, {}, "K_HW"),
    "hw-exp-block8": (8, dict(exact_exp=0, **SMALL), 0.99, {}, "K_HW"),
    "hw-exp-defaults": (16, dict(exact_exp=0), 0.99, {}, "K_HW"),
    # ---- the self-consistent backward clamp
    "clamp-0.999": (16, dict(X1, **SMALL), 0.999, dict(two_kernels=True), "K"),
    "clamp-0.999-block8": (8, dict(X1, **SMALL), 0.999, {}, "K"),
}


def _run_route(name, logit, id_range=None, depth=False):
    from sgn_rast import config, ops
    block, opts, clamp, want, table = ROUTES[name]
    sc, ref = R.reference(block, clamp, id_range, logit)
    with config.override(**opts), ops.upstream_variant(alpha_clamp_bwd=clamp):
        got, lens = _fused(sc, logit, id_range, depth, opts, want)
    if "culled" in want and id_range is None:
        # without the culling the list IS the definition's (the bounding-box list); with it, a proper sub-list
        print(f"[raster fp64 gpu] {name}: {int(lens.sum())} listed entries, the definition's list has "
              f"{int(ref.list_len.sum())}")
        if want["culled"]:
            assert int(lens.sum()) < int(ref.list_len.sum())
        else:
            assert lens.tolist() == ref.list_len.tolist()
    what = f"{name}{', logits' if logit else ''}{', ids ' + str(id_range) if id_range else ''}"
    _check(what, got, ref, getattr(R, table))
    return got, ref


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_equals_the_definition_per_row_and_pixel(route):
    """Probabilities in (`opacity_is_logit=False`): the kernels see the definition's very opacities."""
    _run_route(route, False)


@pytest.mark.parametrize("route", ["fwd-defaults", "bwd-two-kernels-staged", "block8", "block5", "hw-exp-two-kernels",
                                   "clamp-0.999", "qmask-on"])
def test_logit_route_equals_the_definition(route):
    """`opacity_is_logit=True`: the sigmoid in the row build, s (1 - s) in the unpack kernel — the +-12 and -5 rows are
    where it underflows towards 0 (the scale of `v_logit` says what float32 can keep of 1 - s)."""
    got, ref = _run_route(route, True)
    sc = R.make_scene(R.SEED, ROUTES[route][0])
    hi = sc.n_base + np.array([9, 10])                       # logit +12: visible, s (1 - s) = 6.1e-6
    assert ref.visible[hi].all() and (np.abs(got["v_logit"][hi]) < 1e-4 * ref.scale["v_opacity"][hi]).all()
    assert (got["v_logit"][sc.n_base + np.array([11, 12])] == 0).all()      # logit -12: never visible


@pytest.mark.parametrize("route", ["bwd-two-kernels-staged", "fwd-defaults", "block8", "qmask-on"])
@pytest.mark.parametrize("ids", [R.ID_RANGE, R.ID_WINDOW], ids=["shared-list", "list-window"])
def test_id_range_equals_the_definition_of_the_sub_list(route, ids):
    """`id_range` cutting through the cluster: the rows outside stay exactly 0, the ones inside see the sub-list in the
    same relative order — over the shared list (row0 / id tests) and over a compacted list window."""
    from sgn_rast import ops
    before = ops.window_stats["sub_lists"]
    got, ref = _run_route(route, False, id_range=ids)
    assert ops.window_stats["sub_lists"] - before == int(ids == R.ID_WINDOW)
    outside = np.ones(ref.visible.size, bool)
    outside[ids[0]:ids[1]] = False
    for name in ("v_xy", "v_conic", "v_colors", "v_opacity"):
        assert (got[name].reshape(outside.size, -1)[outside] == 0).all(), name


@pytest.mark.parametrize("route", ["fwd-defaults", "fwd-four-waves-batched", "block8", "block5", "hw-exp-two-kernels",
                                   "culling-off"])
def test_depth_channel_equals_the_definition(route):
    """`depth_channel=True`: depth per pixel = sum depth_g alpha T, accumulated by the colour pass."""
    from sgn_rast import ops
    before = ops.depth_stats["accumulated"]
    got, _ref = _run_route(route, False, depth=True)
    assert "depth" in got and ops.depth_stats["accumulated"] == before + 1


@pytest.mark.parametrize("block,opts", [(16, dict(X1)), (16, dict(X1, **SMALL)), (8, dict(X1, **SMALL))],
                         ids=["defaults", "small", "block8"])
def test_clamped_colours_and_sigmoid_proved_on_the_graph(block, opts):
    """`ops.rasterize_gaussians(clamp(pre, min=0), sigmoid(logits))`: the node differentiates straight into `pre` (the
    `colors_pre >= 0` mask of the unpack kernel) and the logits (its sigmoid-OUTPUT chain)."""
    from sgn_rast import config, ops
    sc, ref = R.reference(block, 0.99, None, True)
    xys, conics = _t(sc.xys).requires_grad_(True), _t(sc.conics).requires_grad_(True)
    pre, logits = _t(sc.colors_pre).requires_grad_(True), _t(sc.logits[:, None]).requires_grad_(True)
    with config.override(graph_proofs=True, **opts):
        ops.clear_binning_cache()
        before = dict(ops.activation_proof_stats)
        img, alpha = ops.rasterize_gaussians(xys, _t(sc.depths), _t(sc.radii), conics, _t(sc.num_tiles_hit),
                                             torch.clamp(pre, min=0.0), torch.sigmoid(logits), sc.H, sc.W, block,
                                             background=_t(sc.background), return_alpha=True)
        assert ops.activation_proof_stats["opacity"] == before["opacity"] + 1        # both activations were bypassed
        assert ops.activation_proof_stats["colors"] == before["colors"] + 1
        _assert_route(img.grad_fn, opts, {})
        ((img * _t(sc.w_img)).sum() + (alpha * _t(sc.w_alpha)).sum()).backward()
        torch.cuda.synchronize()
    got = dict(img=_np(img), alpha=_np(alpha), v_xy=_np(xys.grad), v_conic=_np(conics.grad), v_colors_pre=_np(pre.grad),
               v_logit=_np(logits.grad))
    _check(f"graph proofs, block {block}", got, ref, R.K)
    masked = np.asarray(sc.colors_pre) < 0
    assert masked.any() and (got["v_colors_pre"][masked] == 0).all()
    assert (np.abs(ref.val["v_colors"][masked]) > 0).any()              # (the mask hides a gradient that is not 0)


def test_plain_entry_takes_probabilities_and_column_opacities():
    """`ops.rasterize_gaussians` on plain tensors, opacities [N,1]: no activation is folded in."""
    from sgn_rast import config, ops
    sc, ref = R.reference(16, 0.99)
    xys, conics, colors, opac = _leaves(sc, sc.opacities[:, None])
    with config.override(**X1):
        ops.clear_binning_cache()
        img, alpha = ops.rasterize_gaussians(xys, _t(sc.depths), _t(sc.radii), conics, _t(sc.num_tiles_hit), colors, opac,
                                             sc.H, sc.W, 16, background=_t(sc.background), return_alpha=True)
        ((img * _t(sc.w_img)).sum() + (alpha * _t(sc.w_alpha)).sum()).backward()
        torch.cuda.synchronize()
    assert opac.grad.shape == (sc.n, 1)
    _check("plain entry", dict(img=_np(img), alpha=_np(alpha), v_xy=_np(xys.grad), v_conic=_np(conics.grad),
                               v_colors=_np(colors.grad), v_opacity=_np(opac.grad)), ref, R.K)


@pytest.mark.parametrize("opts,clamp", [(dict(X1), 0.99), (dict(X1, **SMALL), 0.99), (dict(X1, **SMALL), 0.999),
                                        (dict(exact_exp=0, **SMALL), 0.99)],
                         ids=["defaults", "small", "small-clamp-0.999", "small-hw-exp"])
def test_batched_views_equal_the_definition_per_view(opts, clamp):
    """`views._RasterViews`, B = 2 views sharing the opacity logits: each view's images per pixel and `v_xy`, `v_conic`,
    `v_colors` per (view, row) against that view's definition; the logits' gradient against the SUM over the views."""
    from sgn_rast import config, ops, views
    (v0, v1), v_logit, v_logit_scale = R.views_reference(16, clamp)
    scs = [v0[0], v1[0]]
    stack = lambda f: _t(np.stack([getattr(s, f) for s in scs]))
    xys, conics, colors = (stack(f).requires_grad_(True) for f in ("xys", "conics", "colors"))
    logits = _t(scs[0].logits).requires_grad_(True)
    assert (scs[0].logits == scs[1].logits).all() and (scs[0].xys[:scs[0].n_base] != scs[1].xys[:scs[0].n_base]).any()
    table = R.K_HW if opts["exact_exp"] == 0 else R.K
    with config.override(**opts), ops.upstream_variant(alpha_clamp_bwd=clamp):
        before = dict(views.stats)
        img, alpha, depth = views._RasterViews.apply(xys, stack("depths"), stack("radii"), conics,
                                                     stack("num_tiles_hit"), colors, logits, _t(scs[0].background),
                                                     R.H, R.W, True)
        ((img * stack("w_img")).sum() + (alpha * stack("w_alpha")).sum()).backward()
        torch.cuda.synchronize()
        assert views.stats["forwards"] == before["forwards"] + 1 and views.stats["backwards"] == before["backwards"] + 1
        ro = img.grad_fn.meta[5]
        for name, v in opts.items():
            assert getattr(ro, name) == v, name
    for b, (sc, ref) in enumerate((v0, v1)):
        _check(f"views {opts}, clamp {clamp}, view {b}",
               dict(img=_np(img[b]), alpha=_np(alpha[b]), depth=_np(depth[b]), v_xy=_np(xys.grad[b]),
                    v_conic=_np(conics.grad[b]), v_colors=_np(colors.grad[b])), ref, table)
    keep = ~(v0[1].adjacent | v1[1].adjacent)
    _check(f"views {opts}, clamp {clamp}, logits summed over the views", dict(v_logit=_np(logits.grad)), v0[1], table,
           keep_rows=keep, exp=dict(v_logit=v_logit), scale=dict(v_logit=v_logit_scale))

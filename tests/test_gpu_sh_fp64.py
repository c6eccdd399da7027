"""GPU: every SH colour kernel per element against the fp64 definition of tests/sh_fp64.py, through the Python surfaces
that reach it and with a random upstream gradient handed to ``torch.autograd.grad`` — no projection, rasteriser or loss:

* ``ops.spherical_harmonics`` on a leaf (sgn_sh_fwd / sgn_sh_bwd; aligned and at a 4-byte storage offset) and on a proven
  ``torch.cat((dc, rest), 1)`` (the split backward sgn_sh_bwd_multi with v_dc, sgn_fourier_dc_bwd for a Fourier part);
* ``fused.spherical_harmonics_fused``, tensor form (sgn_sh_fwd_fused / _bwd_fused) and list form (sgn_sh_fwd_parts /
  _bwd_parts; parts of 0, 1, 63, 64, 65 and 130 rows, F alternating 1 / 5, an idft table wider than every F);
* ``dp._sh_multi_hip`` (sgn_sh_bwd_multi over R views, directions or means + cameras behind a pose table, scale 0.5);
* ``views._SHViews`` (sgn_sh_views_fwd / _bwd) for 1, 3 and 16 cameras.

Floating point, per tensor: ``k`` the kernel's scaled error, ``r`` the fp32 CPU restatements' (the largest over three
operation orders); max k <= 4 max r + 2^-22 — 2 for two independent fp32 roundings of one chain, 2 for the kernel's own
operation order and the device 1/sqrtf — and the median and the 0.99 quantile of k <= 2 x the same quantile of r + 2^-24.
The tolerance comes from the reference at run time.  Exact: bands above the active degree, clamped channels (colour and
gradient), rows with all-zero upstream gradient are zeros; copies give copies; two runs are bit-identical; degree 0
never looks at the direction (zero norm, NaN); view b of the batched forward is the fused call with camera b; aligned
and odd-offset calls agree.  Measured values: profiles/sh_fp64.md.
"""
from types import SimpleNamespace

import pytest
import torch

import sh_fp64 as SF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _d(t):
    return None if t is None else t.to(DEV)


def _leaf(t):
    return t.to(DEV).contiguous().requires_grad_(True)


def _cpu(**kw):
    return SimpleNamespace(**{k: (None if v is None else v.detach().cpu()) for k, v in kw.items()})


# ------------------------------------------------------------------------------------------------- the surfaces
def _run_plain(case, offset=0):
    """ops.spherical_harmonics on a leaf whose storage starts ``offset`` floats into its buffer."""
    from sgn_rast import ops
    src = torch.cat((case.dc[:, :1], case.rest), dim=1)
    buf = torch.empty(src.numel() + 4, device=DEV)
    coeffs = buf[offset: offset + src.numel()].view(src.shape)
    coeffs.copy_(src)
    coeffs.requires_grad_(True)
    assert coeffs.data_ptr() % 16 == 4 * offset
    before = dict(ops.sh_split_stats)
    col = ops.spherical_harmonics(case.deg, case.dirs[0].to(DEV), coeffs)
    assert ops.sh_split_stats == dict(before, dense=before["dense"] + 1), "the dense path was not taken"
    (g,) = torch.autograd.grad(col, coeffs, case.v[0].to(DEV))
    torch.cuda.synchronize()
    return _cpu(colors=col[None], v_c=g)


def _run_split(case):
    """ops.spherical_harmonics on cat((DC, REST), 1): DC a plain leaf over the first rows, then a second plain leaf or a
    Fourier sum; REST one leaf, or one per part."""
    from sgn_rast import ops
    first, second = case.rows
    fourier = case.idft is not None and second > 0
    dcs = [_leaf(case.dc[:first, :1])]
    if second:
        dcs.append(_leaf(case.dc[first:, : (5 if fourier else 1)]))
    rests = [_leaf(case.rest[:first]), _leaf(case.rest[first:])] if (second and fourier) else [_leaf(case.rest)]
    parts = [dcs[0]]
    if second and fourier:
        w = case.idft[1, :5].reshape(5, 1).to(DEV).contiguous()
        parts.append(torch.sum(dcs[1] * w, dim=1, keepdim=True))
    elif second:
        parts.append(dcs[1])
    DC = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
    REST = rests[0] if len(rests) == 1 else torch.cat(rests, dim=0)
    old = ops.sh_split_backward
    ops.sh_split_backward = True
    try:
        before = dict(ops.sh_split_stats)
        col = ops.spherical_harmonics(case.deg, case.dirs[0].to(DEV), torch.cat((DC, REST), dim=1))
        assert ops.sh_split_stats == dict(before, split=before["split"] + 1), "the graph proof did not take the call"
        g = torch.autograd.grad(col, dcs + rests, case.v[0].to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.sh_split_backward = old
    v_dc = torch.zeros(case.n, case.dc.shape[1], 3)
    v_dc[:first, :1] = g[0].cpu()
    if second:
        v_dc[first:, : g[1].shape[1]] = g[1].cpu()
    return _cpu(colors=col[None], v_dc=v_dc, v_rest=torch.cat([x.cpu() for x in g[len(dcs):]], dim=0))


def _run_fused(case, cam=None, post=None):
    from sgn_rast import fused
    dc = _leaf(case.dc)
    rest = _leaf(case.rest) if case.k > 1 else None
    F = case.dc.shape[1]
    idft = None if case.idft is None else case.idft[:, :F].contiguous().to(DEV)      # tensor form: row stride F
    col = fused.spherical_harmonics_fused(case.deg, case.means.to(DEV), _d(case.cams[0] if cam is None else cam), dc,
                                          rest, object_ids=_d(case.ids), idft=idft, poses=_d(case.poses),
                                          post_half_clamp=case.post if post is None else post)
    g = torch.autograd.grad(col, [dc] + ([rest] if rest is not None else []), case.v[0].to(DEV))
    torch.cuda.synchronize()
    return _cpu(colors=col[None], v_dc=g[0], v_rest=g[1] if rest is not None else None)


def _run_parts(case):
    from sgn_rast import fused
    bounds = [0]
    for r in case.rows:
        bounds.append(bounds[-1] + r)
    Fp = [1, 5, 1, 5, 1, 5]
    dcs = [_leaf(case.dc[a:b, :f]) for a, b, f in zip(bounds[:-1], bounds[1:], Fp)]
    rests = [_leaf(case.rest[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    assert case.idft.shape[1] > max(Fp)
    col = fused.spherical_harmonics_fused(case.deg, case.means.to(DEV), case.cams[0].to(DEV), dcs, rests,
                                          idft=case.idft.to(DEV), poses=_d(case.poses), post_half_clamp=case.post)
    g = torch.autograd.grad(col, dcs + rests, case.v[0].to(DEV))
    torch.cuda.synchronize()
    v_dc = torch.zeros(case.n, 5, 3)
    for a, b, f, x in zip(bounds[:-1], bounds[1:], Fp, g[:6]):
        assert x.shape == (b - a, f, 3)
        v_dc[a:b, :f] = x.cpu()
    return _cpu(colors=col[None], v_dc=v_dc, v_rest=torch.cat([x.cpu() for x in g[6:]], dim=0))


def _run_multi(case):
    from sgn_rast import dp
    ids = None if case.ids is None else case.ids.to(DEV)
    v_dc, v_rest = dp._sh_multi_hip(case.deg, case.k, _d(case.dirs), _d(case.means), _d(case.cams), ids, _d(case.poses),
                                    case.v.to(DEV), case.scale)
    torch.cuda.synchronize()
    return _cpu(v_dc=v_dc, v_rest=v_rest)


def _run_views(case):
    from sgn_rast import views
    B = case.cams.shape[0]
    cams = [SimpleNamespace(viewmat=torch.eye(4), cam_pos=case.cams[b], fx=1.0, fy=1.0, cx=0.0, cy=0.0) for b in range(B)]
    dc = _leaf(case.dc)
    rest = _leaf(case.rest) if case.k > 1 else None
    col = views._SHViews.apply(case.deg, case.means.to(DEV), dc, rest, views.cam_table(cams), B)
    g = torch.autograd.grad(col, [dc] + ([rest] if rest is not None else []), case.v.to(DEV))
    torch.cuda.synchronize()
    return _cpu(colors=col, v_dc=g[0], v_rest=g[1] if rest is not None else None)


RUN = {"plain": _run_plain, "split": _run_split, "fused": _run_fused, "parts": _run_parts, "multi": _run_multi,
       "views": _run_views}
NAMES = ("colors", "v_c", "v_dc", "v_rest")


def _same(a, b, what):
    for name in NAMES:
        x, y = getattr(a, name, None), getattr(b, name, None)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), (what, name)


def _check(spec, got, case, ref, r32s):
    label = SF.spec_id(spec)
    fails = SF.check(case, got, ref, r32s, label)
    fails += SF.duplicates_equal(case, {"colors": (getattr(got, "colors", None), 1), "v_c": (getattr(got, "v_c", None), 0),
                                        "v_dc": (getattr(got, "v_dc", None), 0),
                                        "v_rest": (getattr(got, "v_rest", None), 0)}, label)
    assert not fails, "\n".join(fails)


def _case_test(spec):
    case = SF.case_of(spec)
    ref, r32s = SF.definition(case), SF.restatements(case)
    run = RUN[case.kind]
    got = run(case)
    _check(spec, got, case, ref, r32s)
    _same(got, run(case), SF.spec_id(spec) + ": two runs")
    return case, got, ref, r32s


# ------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("spec", SF.specs("plain"), ids=SF.spec_id)
def test_plain_forward_and_backward(spec):
    """Aligned and at a 4-byte storage offset (the dword stage-in); at the grid-stride sizes (SF.GRID_SIZES: the second
    trip of sh_fwd_kernel's prefetching loop, ending in a partial span) the two agree bit for bit."""
    case, got, ref, r32s = _case_test(spec)
    odd = _run_plain(case, offset=1)
    # sgn_sh_fwd caps its grid at GRID_CAP = 1536 blocks of WAVES waves, a 64-row span per wave and trip: more than
    # 1536 * WAVES * 64 rows (WAVES = 4 at K <= 16, 2 at K = 25) send the prefetching loop into a second trip
    if case.n > SF.GRID_CAP * (2 if case.k > 16 else 4) * 64:
        _same(got, odd, "aligned vs odd offset")               # (which is every criterion the aligned call just met)
    else:
        _check(spec, odd, case, ref, r32s)
    _same(odd, _run_plain(case, offset=1), "odd offset: two runs")


@pytest.mark.parametrize("spec", SF.specs("split"), ids=SF.spec_id)
def test_split_backward_over_a_proven_concatenation(spec):
    _case_test(spec)


@pytest.mark.parametrize("spec", SF.specs("fused"), ids=SF.spec_id)
def test_fused_tensor_form(spec):
    _case_test(spec)


@pytest.mark.parametrize("spec", SF.specs("parts"), ids=SF.spec_id)
def test_fused_list_form(spec):
    _case_test(spec)


@pytest.mark.parametrize("spec", SF.specs("multi"), ids=SF.spec_id)
def test_multi_view_backward(spec):
    _case_test(spec)


@pytest.mark.parametrize("spec", SF.specs("views"), ids=SF.spec_id)
def test_batched_views(spec):
    case, got, _ref, _r32s = _case_test(spec)
    B = case.cams.shape[0]
    assert B <= 3 or B == 16
    for b in (range(B) if B <= 3 else (0, 7, 15)):
        one = _run_fused(case, cam=case.cams[b], post=True)
        assert torch.equal(got.colors[b], one.colors[0]), (SF.spec_id(spec), "view", b, "vs the fused call")

"""CPU: the fp64 definition of the SH colour surfaces (tests/sh_fp64.py) checked on its own — the closed-form bases are
orthonormal and agree with the oracle's fp64 recurrences, the explicit gradients are autograd's, a further fp32
evaluation passes the GPU test's criteria against the three restatements, and every case the GPU test runs keeps the
clamp caps from the reference alone.
"""
import math

import numpy as np
import pytest
import torch

import sh_fp64 as SF
from oracle import torch_oracle as TO

POST_KINDS = ("fused", "parts", "views")


def test_closed_form_bases_are_orthonormal_over_the_sphere():
    # 16-point Gauss-Legendre in cos(theta) (exact to polynomial degree 31; a product of two bases has degree 8) times
    # 32 uniform phi (exact below frequency 32)
    ct, wt = np.polynomial.legendre.leggauss(16)
    phi = 2.0 * math.pi * np.arange(32) / 32
    CT, PH = np.meshgrid(ct, phi, indexing="ij")
    ST = np.sqrt(1.0 - CT * CT)
    d = torch.from_numpy(np.stack([ST * np.cos(PH), ST * np.sin(PH), CT], axis=-1).reshape(-1, 3))
    w = torch.from_numpy(np.repeat(wt, 32) * (2.0 * math.pi / 32))
    B = torch.stack(SF.bases(d * 3.7, 4), dim=-1)                          # [512, 25] (un-normalised input)
    gram = (B * w[:, None]).T @ B
    err = float((gram - torch.eye(25, dtype=torch.float64)).abs().max())
    print(f"[sh fp64 cpu] Gram matrix off identity by {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("k,deg", SF.VALID)
def test_closed_forms_agree_with_the_oracles_fp64_recurrences(k, deg):
    case = SF.make_case("plain", 500, k, deg, family="edges", seed=3)
    if deg == 0:
        case.dirs = torch.nan_to_num(case.dirs, nan=1.0) + 1.0             # (the oracle normalises at every degree)
    coeffs = torch.cat((case.dc[:, :1], case.rest), dim=1).double()
    ref = SF.definition(case)
    exp = TO.spherical_harmonics(deg, case.dirs[0].double(), coeffs)
    S = SF.scales(case)
    err = float(SF.scaled_error(ref.colors[0], exp, S.fwd).max())
    print(f"[sh fp64 cpu] ({k}, {deg}): closed forms vs fp64 recurrences {err:.2e}")
    assert err <= 1e-12


def _autograd(case):
    """fp64 autograd through the explicit forward: d sum(colors * v) * scale / d (dc, rest)."""
    dc = case.dc.double().requires_grad_(True)
    rest = case.rest.double().requires_grad_(True)
    B = SF.bases(SF.view_dirs(case), case.deg)
    w = SF.weights(case)
    c0 = (dc * w[:, :, None]).sum(1)
    x = B[0][..., None] * c0
    for k in range(1, (case.deg + 1) ** 2):
        x = x + B[k][..., None] * rest[:, k - 1]
    col = torch.clamp(x + 0.5, min=0.0) if case.post else x
    return torch.autograd.grad((col * case.v.double()).sum() * case.scale, (dc, rest), allow_unused=True)


@pytest.mark.parametrize("spec", [
    dict(kind="plain", n=257, k=25, deg=4, family="edges"),
    dict(kind="fused", n=257, k=16, deg=3, family="edges", F=5, table=True, poses=True, post=True),
    dict(kind="parts", n=323, k=25, deg=2, family="edges", poses=True, post=True),
    dict(kind="multi", n=257, k=16, deg=3, family="generic", V=3, form="means"),
    dict(kind="views", n=257, k=25, deg=4, family="generic", V=3),
    dict(kind="views", n=65, k=1, deg=0, family="generic", V=16),
], ids=SF.spec_id)
def test_explicit_gradients_are_autograd_of_the_explicit_forward(spec):
    case = SF.case_of(spec)
    ref = SF.definition(case)
    g_dc, g_rest = _autograd(case)
    S = SF.scales(case)
    # (autograd's subgradient of the clamp at exactly 0 is 0, as the definition's gate `colour > 0`)
    assert float(SF.scaled_error(ref.v_dc, g_dc, S.bwd_dc).max()) <= 1e-12
    if case.k > 1:
        assert float(SF.scaled_error(ref.v_rest, g_rest, S.bwd[:, None, :]).max()) <= 1e-12
        assert float(ref.v_rest[:, (case.deg + 1) ** 2 - 1:].abs().sum()) == 0.0


def _some_specs():
    out = []
    for kind in ("plain", "split", "fused", "parts", "multi", "views"):
        sp = [s for s in SF.specs(kind) if s["n"] <= 4097]
        out += sp[:: max(1, len(sp) // 12)]
        out += [s for s in sp if s["family"] == "far_object"]
    return out


@pytest.mark.parametrize("spec", _some_specs(), ids=SF.spec_id)
def test_a_further_fp32_evaluation_passes_the_gpu_criteria(spec):
    """The protocol is sound: the recurrences with every sum reversed — an evaluation that is none of the three
    restatements — meets the criteria the kernels are held to."""
    case = SF.case_of(spec)
    ref, r32s = SF.definition(case), SF.restatements(case)
    got = SF.definition(case, torch.float32, "recurrence_reversed")
    if case.kind in ("multi",):
        got.colors = None
    fails = SF.check(case, got, ref, r32s, SF.spec_id(spec))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", POST_KINDS)
def test_every_gpu_case_keeps_the_clamp_caps_from_the_reference_alone(kind):
    """Clamp-adjacent channels at most 1 %, at least 20 % clamped and 20 % not, and no restatement comes closer to the
    clamp than a fourth of the nearest non-adjacent channel: a kernel inside its colour tolerance takes the
    definition's side of every gate that is compared."""
    for spec in SF.specs(kind):
        case = SF.case_of(spec)
        if not case.post:
            continue
        ref = SF.definition(case)
        adj, clamped, neither = SF.clamp_shares(case, ref)
        label = SF.spec_id(spec)
        assert adj <= 0.01 and clamped >= 0.2 and neither >= 0.2, (label, adj, clamped, neither)
        S = SF.scales(case)
        _a, cl = SF.clamp_masks(case, ref, S)
        r = max(float(SF.scaled_error(x.colors, ref.colors, S.fwd[None])[~cl].max()) for x in SF.restatements(case))
        assert SF.gate_margin(case, ref) > 4.0 * r + 2.0 ** -22, (label, SF.gate_margin(case, ref), r)
        if case.n >= 257 and not (case.deg == 0 and case.v.shape[0] > 8):
            assert adj > 0, (label, "no planted clamp-adjacent channel")


def test_families_hold_what_they_promise():
    c = SF.make_case("plain", 257, 16, 3, family="edges")
    d = c.dirs[0]
    assert int(((d != 0).sum(-1) == 1).sum()) >= 6 and int((((d != 0).sum(-1) == 2) & (d.abs().max(-1).values == 1)).sum()) >= 12
    pole = d[18:26]
    assert bool((pole[:, :2].abs().max(-1).values < 1e-3 * pole[:, 2].abs()).all())
    assert c.dup.shape[0] == 32 and bool((c.dup[:, 1] // 64 > c.dup[:, 0] // 64).all())
    assert torch.equal(d[c.dup[:, 0]], d[c.dup[:, 1]])
    zero_rows = ~(c.v != 0).any(0).any(-1)
    assert 0.03 < float(zero_rows.double().mean()) < 0.2
    z = SF.make_case("plain", 65, 1, 0)
    assert bool((z.dirs[0][0] == 0).all()) and bool(torch.isnan(z.dirs[0][2]).all())
    f = SF.make_case("fused", 65, 1, 0, post=True)
    assert torch.equal(f.means[0], f.cams[0])
    far = SF.make_case("fused", 257, 16, 3, family="far_object", F=5, table=True, poses=True, post=True)
    assert float(far.poses[:, 9:12].norm(dim=-1).min()) > 900 and float(SF.view_dirs(far).norm(dim=-1).max()) < 101
    p = SF.make_case("parts", 0, 16, 3, family="edges", poses=True, post=True)
    assert p.rows == list(SF.PARTS_ROWS) and p.Fs[p.ids.long() == 3].unique().tolist() == [5]
    assert bool((p.ids[p.dup[:, 0]] == 3).all()) and bool((p.ids[p.dup[:, 1]] == 5).all())

"""CPU: the fp64 definition of one Adam step (tests/adam_fp64.py) checked on its own — torch's float64 step is the
recurrence of the class's documentation, the float32 yardstick is finite and within a few ulp of it in the scales the
GPU test uses (so that the GPU bound, a multiple of the yardstick's error, cannot go slack), no element is left out of
a comparison, and the cases hold the rows they promise.
"""
import math

import pytest
import torch

import adam_fp64 as AF
from sh_fp64 import _stats

_CASE = []


def _case():
    if not _CASE:
        _CASE.append(AF.make_case())
    return _CASE[0]


@pytest.mark.parametrize("combo", AF.COMBOS, ids=AF.combo_id)
def test_torchs_float64_step_is_the_documented_recurrence(combo):
    t, hyper = combo
    lr, b1, b2, eps = hyper
    c = _case()
    ref = AF.definition(c.p, c.g, c.m, c.v, hyper, t)
    p, g, m, v = (x.double() for x in (c.p, c.g, c.m, c.v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    m_hat, v_hat = m1 / (1.0 - b1 ** t), v1 / (1.0 - b2 ** t)
    p1 = p - lr * m_hat / (v_hat.sqrt() + eps)
    S = AF.scales(c.p, c.g, c.m, c.v, hyper, t, ref)
    assert ref.step == t
    for name, x in zip(AF.NAMES, (p1, m1, v1)):
        err = float(AF.scaled_error(x, getattr(ref, name), getattr(S, name)).max())
        assert err <= 1e-14, (name, err)


@pytest.mark.parametrize("combo", AF.COMBOS, ids=AF.combo_id)
def test_the_float32_yardstick_is_finite_and_a_few_ulp_from_the_definition(combo):
    t, hyper = combo
    c = _case()
    ref, r32 = AF.definition(c.p, c.g, c.m, c.v, hyper, t), AF.yardstick(c.p, c.g, c.m, c.v, hyper, t)
    S = AF.scales(c.p, c.g, c.m, c.v, hyper, t, ref)
    for name in AF.NAMES:
        x = getattr(r32, name)
        assert x.dtype is torch.float32 and x.shape == (AF.N,) and bool(torch.isfinite(x).all()), name
        r = AF.scaled_error(x, getattr(ref, name), getattr(S, name))
        assert r.shape == (AF.N,)                                  # no element is left out
        med, p99, mx = _stats(r)
        print(f"[adam fp64 cpu] {AF.combo_id(combo)} {name}: median {med / AF.U:.3f} p99 {p99 / AF.U:.3f} max {mx / AF.U:.3f}"
              f" (units of 2^-24)")
        assert mx <= 16.0 * AF.U and med <= AF.U, (name, med / AF.U, mx / AF.U)
    # the yardstick passes the GPU test's rule against itself, on all rows and on the update alone
    for mask in (None, c.p0):
        fails, _ = AF.compare(r32, r32, ref, S, mask)
        assert not fails, fails


def test_scaled_error_counts_every_element():
    ref, S = torch.tensor([1.0, 0.0, 2.0, 4.0], dtype=torch.float64), torch.tensor([2.0, 0.0, 1.0, 1.0], dtype=torch.float64)
    e = AF.scaled_error(torch.tensor([2.0, 0.25, math.nan, math.inf]), ref, S)
    assert e.tolist() == [0.5, 0.25, math.inf, math.inf]          # scaled; absolute where the scale is 0; not finite


@pytest.mark.parametrize("n", [1, 3, 5, 4097, AF.N])
def test_cases_hold_the_rows_they_promise(n):
    c = AF.make_case(n, seed=3)
    k = min(AF.SPECIAL, n // 20)
    assert all(x.dtype is torch.float32 and x.shape == (n,) for x in (c.p, c.m, c.v, c.g))
    assert int(c.p0.sum()) == n // 8 and bool((c.p[c.p0] == 0).all()) and bool((c.p[~c.p0] != 0).all())
    assert len(set(torch.cat((c.zero, c.reset, c.tiny)).tolist())) == 3 * k
    assert bool((c.v >= 0).all())
    for x in (c.g, c.m, c.v):
        assert bool((x[c.zero] == 0).all())
    assert bool((c.g[c.reset] == 0).all()) and bool((c.v[c.reset] == 0).all()) and bool((c.m[c.reset] != 0).all())
    if n == AF.N:
        assert k == 50 and 0 < int(c.p0[c.zero].sum()) < k           # some zero rows inside the p = 0 rows, some not
        a = c.g[c.tiny].double().abs()
        assert bool((a >= 0.99e-23).all()) and bool((a <= 1.01e-19).all())
        g2 = c.g[c.tiny] * c.g[c.tiny]                                # in float32: denormal or 0
        assert bool((g2 < 2.0 ** -126).all()) and bool((g2 == 0).any()) and bool((g2 > 0).any())
        assert bool((c.v[c.tiny[: k // 2]] > 0).all()) and bool((c.v[c.tiny[k // 2:]] == 0).all())
        lg = c.g[~c.p0].abs().log10()
        assert float(lg.max()) > -1.0 and float(lg.median()) < -3.5   # gradients over nine decades

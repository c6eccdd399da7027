"""One Adam step as a definition, and the per-element statistics its tests use (CPU, torch).

Definition.  One ``step()`` of ``torch.optim.Adam`` on float64 copies on the CPU, from a preset state
``{"step": t - 1, "exp_avg": m, "exp_avg_sq": v}``: torch's own class, nothing restated (tests/test_adam_fp64.py checks
it against the recurrence of the class's documentation).  Yardstick: the same step of the same class in float32 on the
CPU — the thing ``FusedAdam`` claims to follow.  ``step_once`` runs either, or ``FusedAdam`` on the device.

Error scales (fp64), per element, with inputs ``p, m, v, g`` and the definition's ``v'``:

    exp_avg     |d| / max(|m|, |g|)
    exp_avg_sq  |d| / max(v, g^2, 2^-126)              the smallest normal: one denormal step counts as one ulp
    param       |d| / max(|p|, step_size max(|m|, |g|) / denom),   step_size = lr / (1 - beta1^t),
                                                      denom = sqrt(v') / sqrt(1 - beta2^t) + eps

The parameter's scale carries the conditioning of ``m + (1 - beta1)(g - m)``: where ``g`` nearly cancels ``m`` the update
is small against what it was computed from, and float32 itself is hundreds of ulp of the update away.  Where a scale is
0 (``g = m = 0``) the error is taken absolute.  A NaN or an infinity in the compared tensor is an infinite error.

Rows of a case (``make_case``): ``p ~ N(0,1)``, ``m ~ 1e-3 N``, ``v = (1e-3 N)^2``, ``g = N 10^k`` with k uniform in
-9..0; the first ``n // 8`` rows have ``p = 0`` exactly, so that the update itself is the output; and, at seeded places
(some of them among the ``p = 0`` rows), ``zero``: ``g = m = v = 0`` (the parameter must not move); ``reset``:
``v = 0, g = 0, m != 0`` (``exp_avg_sq`` reset by densification: eps alone is the denominator); ``tiny``: ``|g|`` in
1e-23..1e-19 (``g^2`` is denormal or underflows) — half of them over ordinary moments, half over ``m = v = 0`` (a reset
row whose gradient vanishes: ``v'`` itself is denormal or 0).
"""
import math
from types import SimpleNamespace

import torch

from sh_fp64 import _stats

N = 20000
STEPS = (1, 2, 25, 1000, 30000)
HYPERS = ((1.6e-4, 0.9, 0.999, 1e-15), (0.05, 0.9, 0.999, 1e-15), (1e-3, 0.8, 0.99, 1e-8))      # lr, beta1, beta2, eps
COMBOS = [(t, h) for t in STEPS for h in HYPERS]
NAMES = ("param", "exp_avg", "exp_avg_sq")
U = 2.0 ** -24
SPECIAL = 50                                  # rows per special class (fewer where a tensor is shorter than 20 x that)


def combo_id(c):
    t, (lr, b1, b2, eps) = c
    return f"t{t}-lr{lr:g}-b{b1:g}-{b2:g}-eps{eps:g}"


def make_case(n=N, seed=0):
    """The four float32 inputs [n] and the row classes (index tensors ``zero``, ``reset``, ``tiny``; mask ``p0``)."""
    gen = torch.Generator().manual_seed(7919 * seed + n)
    r = lambda: torch.randn(n, generator=gen)
    p, m, v = r(), 1e-3 * r(), (1e-3 * r()) ** 2
    g = r() * 10.0 ** (torch.rand(n, generator=gen) * 9.0 - 9.0)
    p[: n // 8] = 0.0
    k = min(SPECIAL, n // 20)
    where = torch.randperm(n, generator=gen)[: 3 * k]
    zero, reset, tiny = where[:k], where[k: 2 * k], where[2 * k:]
    g[zero] = 0.0; m[zero] = 0.0; v[zero] = 0.0
    g[reset] = 0.0; v[reset] = 0.0
    sign = torch.where(torch.rand(k, generator=gen) < 0.5, -1.0, 1.0)
    g[tiny] = sign * 10.0 ** (torch.rand(k, generator=gen, dtype=torch.float64) * 4.0 - 23.0).float()
    m[tiny[k // 2:]] = 0.0; v[tiny[k // 2:]] = 0.0
    return SimpleNamespace(n=n, p=p, m=m, v=v, g=g, zero=zero, reset=reset, tiny=tiny, p0=torch.arange(n) < n // 8)


def step_once(opt_cls, p, g, m, v, hyper, t, dtype=torch.float32, device="cpu"):
    """One ``step()`` of ``opt_cls`` (torch.optim.Adam or FusedAdam) on copies of the inputs, from the preset state of
    step ``t - 1``.  Returns (param, exp_avg, exp_avg_sq) on the CPU and ``state["step"]`` as a float."""
    lr, b1, b2, eps = hyper
    to = lambda x: x.to(device=device, dtype=dtype).clone()
    prm = torch.nn.Parameter(to(p))
    prm.grad = to(g)
    opt = opt_cls([prm], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[prm] = {"step": torch.tensor(float(t - 1)), "exp_avg": to(m), "exp_avg_sq": to(v)}
    opt.step()
    st = opt.state[prm]
    return SimpleNamespace(param=prm.detach().cpu(), exp_avg=st["exp_avg"].cpu(), exp_avg_sq=st["exp_avg_sq"].cpu(),
                           grad=prm.grad.cpu(), step=float(st["step"]))


def definition(p, g, m, v, hyper, t):
    return step_once(torch.optim.Adam, p, g, m, v, hyper, t, dtype=torch.float64)


def yardstick(p, g, m, v, hyper, t):
    return step_once(torch.optim.Adam, p, g, m, v, hyper, t, dtype=torch.float32)


def scales(p, g, m, v, hyper, t, ref):
    """fp64 error scales of the three outputs, from the inputs and the definition's ``exp_avg_sq``."""
    lr, b1, b2, eps = hyper
    p, g, m, v = (x.double() for x in (p, g, m, v))
    s_m = torch.maximum(m.abs(), g.abs())
    s_v = torch.maximum(torch.maximum(v, g * g), torch.full((), 2.0 ** -126, dtype=torch.float64))
    denom = ref.exp_avg_sq.double().sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    s_p = torch.maximum(p.abs(), (lr / (1.0 - b1 ** t)) * s_m / denom)
    return SimpleNamespace(param=s_p, exp_avg=s_m, exp_avg_sq=s_v)


def scaled_error(x, ref, S):
    """``|x - ref| / S`` in fp64 over EVERY element; absolute where S is 0; infinite where ``x`` is not finite."""
    x = x.double()
    e = (x - ref.double()).abs() / torch.where(S == 0, torch.ones_like(S), S)
    return torch.where(torch.isfinite(x), e, torch.full((), math.inf, dtype=torch.float64))


def compare(got, r32, ref, S, mask=None, label=""):
    """The project's floating-point rule (tests/sh_fp64.py) for the three outputs on the rows ``mask`` (all rows without
    one): k the scaled error of ``got``, r that of the float32 yardstick; max k <= 4 max r + 2^-22, median and 0.99
    quantile of k <= 2 x the same quantile of r + 2^-24.  Returns (violations, {name: (k stats, r stats)})."""
    fails, figures = [], {}
    for name in NAMES:
        k = scaled_error(getattr(got, name), getattr(ref, name), getattr(S, name))
        r = scaled_error(getattr(r32, name), getattr(ref, name), getattr(S, name))
        assert k.shape == r.shape == getattr(ref, name).shape, (label, name)
        if mask is not None:
            k, r = k[mask], r[mask]
        if k.numel() == 0:
            continue
        ks, rs = _stats(k), _stats(r)
        caps = (2.0 * rs[0] + U, 2.0 * rs[1] + U, 4.0 * rs[2] + 4.0 * U)
        figures[name] = (ks, rs)
        print(f"[adam fp64] {label} {name}: elements {k.numel()} (units of 2^-24) median k {ks[0] / U:.3f} r {rs[0] / U:.3f}"
              f"  p99 k {ks[1] / U:.3f} r {rs[1] / U:.3f}  max k {ks[2] / U:.3f} r {rs[2] / U:.3f}")
        fails += [f"{label} {name}: {what} k = {kv / U:.3f} > cap {cap / U:.3f} (r = {rv / U:.3f}), units of 2^-24"
                  for what, kv, cap, rv in zip(("median", "p99", "max"), ks, caps, rs) if not kv <= cap]
    return fails, figures

"""The SH colour surfaces written out as a definition, and the per-element statistics their tests use (CPU, torch).

Bases.  The 25 real spherical harmonics of a normalised direction as closed-form Cartesian polynomials, constants from
``sqrt`` and ``pi`` in fp64, order ``l`` then ``m = -l..l``, sign ``(-1)^|m|`` times the usual real SH (gsplat's).  The
kernels, the C oracle and ``oracle.torch_oracle._sh_bases`` all evaluate Sloan's recurrences; nothing here does, except
the fp32 restatement that is named after them.

One ``Case`` describes every surface (plain, fused, parts, multi, views): per view ``r`` a direction per row — given, or
``(R m + t if poses else m) - cam_r`` with the pose row laid out as ``[R row-major (9), t (3), quaternion (4)]`` — the
coefficients ``c_0 = sum_f dc[f] idft[object, f]`` (unit weight without a table) and ``c_k = rest[k - 1]``, and

    colour_r = sum_{k < nb} B_k(dir_r) c_k,  nb = (deg + 1)^2,  then ``max(x + 0.5, 0)`` with ``post``
    v_c[k]   = scale * sum_r B_k(dir_r) g_r,  g_r = v_r where the definition's colour_r > 0 (all of v_r without post),
               exactly 0 for k >= nb
    v_dc[f]  = idft[object, f] * v_c[0],  v_rest[k - 1] = v_c[k]

``definition(case)`` evaluates that in fp64 (closed forms); the same function in fp32 in three operation orders
(``ORDERS``: the closed forms, the recurrences, the closed forms with every sum reversed and the normalisation as a
division) are the "restatements" whose own distance to fp64 sets the tolerances of the GPU test at run time; every
statistic of the restatement error is the largest over them.

Error scales (fp64).  ``|got - ref| / S`` per element: forward ``S = sum_f |dc_f||w_f| + sum_{1 <= k < nb} |c_k|`` (+ 0.5
with post); backward ``S = |scale| sum_r |v_r|``, times ``|w_f|`` for ``v_dc``.  The bases are bounded by 1.

Clamp.  With post, a channel whose fp64 ``x + 0.5`` lies within ``2^-18 S`` of 0 is clamp-adjacent: its colour is
compared like any other, its gradient must equal the gated or the ungated definition.  Below ``-2^-18 S`` the channel is
clamped: colour and gradient exactly 0.  ``clamp_shares`` counts both from the reference alone.

DC scale.  With N(0,1) coefficients the pre-clamp colour is N(0, nb / 4 pi): at degree 0 (sigma 0.28) only 3.8 % of the
channels fall below -0.5, at degree 1 (0.56) 19 % — no seed reaches the 20 % of clamped channels the gate's test asks
for.  The families that can be clamped therefore draw the DC term from N(0, 4^2) at degrees 0 and 1 (33 % clamped); the
error scale S carries the factor.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import torch_oracle as TO

VALID = [(k, d) for k in (1, 4, 9, 16, 25) for d in range(5) if (d + 1) ** 2 <= k]      # the 15 valid (k, deg)
ADJ = 2.0 ** -18
ORDERS = {"closed": ("closed", False), "recurrence": ("recurrence", False), "reversed": ("closed", True)}
EXTRA_ORDER = {"recurrence_reversed": ("recurrence", True)}     # a further evaluation (test_sh_fp64.py)
PARTS_ROWS = (0, 1, 63, 64, 65, 130)
CAM0 = (0.5, -0.25, 1.0)


# ---------------------------------------------------------------------------------------------- the bases
def closed_bases(x, y, z, deg):
    """The (deg + 1)^2 bases of the unit vector (x, y, z), as a list of tensors shaped like x."""
    s, pi = math.sqrt, math.pi
    xx, yy, zz = x * x, y * y, z * z
    b = [0.5 * s(1.0 / pi) * torch.ones_like(x)]
    if deg >= 1:
        c = s(3.0 / (4.0 * pi))
        b += [-c * y, c * z, -c * x]
    if deg >= 2:
        c = 0.5 * s(15.0 / pi)
        b += [c * (x * y), -c * (y * z), 0.25 * s(5.0 / pi) * (3.0 * zz - 1.0), -c * (x * z),
              0.25 * s(15.0 / pi) * (xx - yy)]
    if deg >= 3:
        a3, a2, a1 = 0.25 * s(35.0 / (2.0 * pi)), 0.5 * s(105.0 / pi), 0.25 * s(21.0 / (2.0 * pi))
        b += [-a3 * (y * (3.0 * xx - yy)), a2 * (x * y * z), -a1 * (y * (5.0 * zz - 1.0)),
              0.25 * s(7.0 / pi) * (z * (5.0 * zz - 3.0)), -a1 * (x * (5.0 * zz - 1.0)),
              0.25 * s(105.0 / pi) * (z * (xx - yy)), -a3 * (x * (xx - 3.0 * yy))]
    if deg >= 4:
        a4, a3, a2, a1 = 0.75 * s(35.0 / pi), 0.75 * s(35.0 / (2.0 * pi)), 0.75 * s(5.0 / pi), 0.75 * s(5.0 / (2.0 * pi))
        b += [a4 * (x * y * (xx - yy)), -a3 * (y * z * (3.0 * xx - yy)), a2 * (x * y * (7.0 * zz - 1.0)),
              -a1 * (y * z * (7.0 * zz - 3.0)), (3.0 / 16.0) * s(1.0 / pi) * (35.0 * zz * zz - 30.0 * zz + 3.0),
              -a1 * (x * z * (7.0 * zz - 3.0)), 0.375 * s(5.0 / pi) * ((xx - yy) * (7.0 * zz - 1.0)),
              -a3 * (x * z * (xx - 3.0 * yy)),
              (3.0 / 16.0) * s(35.0 / pi) * (xx * (xx - 3.0 * yy) - yy * (3.0 * xx - yy))]
    return b


def bases(dirs, deg, kind="closed", divide=False):
    """[..., 3] un-normalised directions -> list of (deg + 1)^2 tensors [...].  Degree 0 never looks at ``dirs``."""
    shape = dirs.shape[:-1]
    if deg == 0:
        return [torch.full(shape, 0.5 * math.sqrt(1.0 / math.pi), dtype=dirs.dtype)]
    if kind == "recurrence":
        return [b.reshape(shape) for b in TO._sh_bases(dirs.reshape(-1, 3), deg)]
    x, y, z = dirs.unbind(-1)
    ss = x * x + y * y + z * z
    if divide:
        nrm = torch.sqrt(ss)
        x, y, z = x / nrm, y / nrm, z / nrm
    else:
        inv = 1.0 / torch.sqrt(ss)
        x, y, z = x * inv, y * inv, z * inv
    return closed_bases(x, y, z, deg)


def _sum(terms, rev=False):
    terms = terms[::-1] if rev else terms
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


# ---------------------------------------------------------------------------------------------- the definition
def view_dirs(case, dtype=torch.float64, rev=False):
    """[V, n, 3] directions of every view."""
    if case.dirs is not None:
        return case.dirs.to(dtype)
    m = case.means.to(dtype)
    if case.poses is not None:
        P = case.poses.to(dtype)[case.ids.long()]
        c = m.unbind(-1)
        m = torch.stack([_sum([P[:, 3 * j] * c[0], P[:, 3 * j + 1] * c[1], P[:, 3 * j + 2] * c[2], P[:, 9 + j]], rev)
                         for j in range(3)], dim=-1)
    return m[None] - case.cams.to(dtype)[:, None, :]


def weights(case, dtype=torch.float64):
    """[n, F] Fourier weight of every row (0 beyond the row's own Fourier dimension)."""
    n, F = case.dc.shape[0], case.dc.shape[1]
    if case.idft is None:
        w = torch.ones(n, F, dtype=dtype)
    else:
        w = case.idft.to(dtype)[case.ids.long()][:, :F]
    return torch.where(torch.arange(F)[None, :] < case.Fs[:, None], w, torch.zeros((), dtype=dtype))


def definition(case, dtype=torch.float64, order="closed"):
    """colors / pre [V, n, 3] (``pre``: the value the clamp sees, or the colour itself without post), and with
    ``case.v``: v_c [n, K, 3], v_dc [n, F, 3], v_rest [n, K - 1, 3]."""
    kind, rev = {**ORDERS, **EXTRA_ORDER}[order]
    nb, K = (case.deg + 1) ** 2, case.k
    B = bases(view_dirs(case, dtype, rev), case.deg, kind, divide=rev)
    dc, w = case.dc.to(dtype), weights(case, dtype)
    F = dc.shape[1]
    c0 = _sum([dc[:, f] * w[:, f, None] for f in range(F)], rev)
    rest = case.rest.to(dtype)
    x = _sum([B[0][..., None] * c0] + [B[k][..., None] * rest[:, k - 1] for k in range(1, nb)], rev)
    out = SimpleNamespace(B=B)
    out.pre = x + 0.5 if case.post else x
    out.colors = torch.clamp(out.pre, min=0.0) if case.post else x
    if case.v is not None:
        v = case.v.to(dtype)
        g = torch.where(out.colors > 0, v, torch.zeros((), dtype=dtype)) if case.post else v
        V = g.shape[0]
        v_c = torch.zeros(dc.shape[0], K, 3, dtype=dtype)
        for k in range(nb):
            v_c[:, k] = _sum([B[k][r][:, None] * g[r] for r in range(V)], rev) * case.scale
        out.v_c, out.v_rest = v_c, v_c[:, 1:]
        out.v_dc = w[:, :, None] * v_c[:, 0][:, None, :]
    return out


def restatements(case):
    """The definition in fp32 on the CPU, once per operation order of ``ORDERS``."""
    return [definition(case, torch.float32, order) for order in ORDERS]


def scales(case):
    """fp64 error scales: forward [n, 3]; backward [n, 3] (v_rest, v_c) and [n, F, 3] (v_dc)."""
    nb = (case.deg + 1) ** 2
    w = weights(case).abs()
    S = (case.dc.double().abs() * w[:, :, None]).sum(1) + case.rest.double()[:, : nb - 1].abs().sum(1)
    out = SimpleNamespace(fwd=S + (0.5 if case.post else 0.0), w=w)
    if case.v is not None:
        out.bwd = case.v.double().abs().sum(0) * abs(case.scale)
        out.bwd_dc = out.bwd[:, None, :] * w[:, :, None]
    return out


def clamp_masks(case, ref, S):
    """(adjacent, clamped) [V, n, 3] from the fp64 reference alone; all False without post."""
    if not case.post:
        z = torch.zeros_like(ref.pre, dtype=torch.bool)
        return z, z
    return ref.pre.abs() <= ADJ * S.fwd, ref.pre < -ADJ * S.fwd


def clamp_shares(case, ref=None):
    """(share of clamp-adjacent channels, of clamped ones, of channels that are neither)."""
    ref = definition(case) if ref is None else ref
    adj, clamped = clamp_masks(case, ref, scales(case))
    a, c = float(adj.double().mean()), float(clamped.double().mean())
    return a, c, 1.0 - a - c


def gate_margin(case, ref=None):
    """The smallest ``|x + 0.5| / S`` over the channels that are NOT clamp-adjacent (inf without post): an evaluation whose
    scaled colour error stays below it takes the definition's side of the clamp on every such channel."""
    if not case.post:
        return math.inf
    ref = definition(case) if ref is None else ref
    S = scales(case)
    m = ref.pre.abs() / S.fwd
    m = m[m > ADJ]
    return float(m.min()) if m.numel() else math.inf


# ---------------------------------------------------------------------------------------------- the statistics
def scaled_error(x, ref, S):
    """``|x - ref| / S`` in fp64; where S is 0 the element is compared for equality (0 if equal, inf if not)."""
    e = (x.detach().cpu().double() - ref.double()).abs_()
    zero = S == 0
    e.div_(torch.where(zero, torch.ones_like(S), S))
    if bool(zero.any()):
        e = torch.where(zero.expand_as(e) & (e != 0), torch.full((), math.inf, dtype=e.dtype), e)
    bad = e != e
    return torch.where(bad, torch.full((), math.inf, dtype=e.dtype), e) if bool(bad.any()) else e


def _stats(e):
    """(median, 0.99 quantile, max) of a 1-d error tensor — order statistics at rank ceil(q (N - 1)), no interpolation."""
    a = e.numpy()
    n = a.shape[0]
    ranks = [int(math.ceil(q * (n - 1))) for q in (0.5, 0.99)]
    p = np.partition(a, ranks)
    return float(p[ranks[0]]), float(p[ranks[1]]), float(a.max())


def compare_float(name, x, r64, r32s, S, mask, label=""):
    """The floating-point criteria for one tensor on the elements ``mask``: k the scaled error of ``x`` against the fp64
    tensor, r that of each fp32 restatement; max k <= 4 max r + 2^-22, median and 0.99 quantile of k <= 2 x the same
    quantile of r + 2^-24, every statistic of r the largest over the restatements.  Returns (violations, the cap on
    max k)."""
    idx = torch.nonzero(mask.expand_as(r64).reshape(-1))[:, 0]
    if idx.numel() == 0:
        return [], 2.0 ** -22
    k = scaled_error(x, r64, S).reshape(-1)[idx]
    rs = [scaled_error(a, r64, S).reshape(-1)[idx] for a in r32s]
    ks, rstat = _stats(k), [max(v) for v in zip(*[_stats(r) for r in rs])]
    caps = (2.0 * rstat[0] + 2.0 ** -24, 2.0 * rstat[1] + 2.0 ** -24, 4.0 * rstat[2] + 2.0 ** -22)
    u = 2.0 ** -24
    print(f"[sh fp64] {label} {name}: elements {int(k.numel())} (units of 2^-24) median k {ks[0] / u:.3f} r {rstat[0] / u:.3f}"
          f"  p99 k {ks[1] / u:.3f} r {rstat[1] / u:.3f}  max k {ks[2] / u:.3f} r {rstat[2] / u:.3f}")
    fails = [f"{label} {name}: {what} k = {kv / u:.3f} > cap {cap / u:.3f} (r = {rv / u:.3f}), units of 2^-24"
             for what, kv, cap, rv in zip(("median", "p99", "max"), ks, caps, rstat) if not kv <= cap]
    return fails, caps[2]


def check(case, got, ref, r32s, label=""):
    """Every criterion of the GPU test for one evaluation ``got`` of ``case`` (a namespace with any of ``colors``
    [V, n, 3], ``v_dc`` [n, F, 3], ``v_rest`` [n, K - 1, 3], ``v_c`` [n, K, 3]; entries of ``v_dc`` beyond a row's own
    Fourier dimension are not read).  Returns the list of violations."""
    fails = []
    S = scales(case)
    nb, K = (case.deg + 1) ** 2, case.k
    adj, clamped = clamp_masks(case, ref, S)
    x = getattr(got, "colors", None)
    if x is not None:
        x = x.detach().cpu()
        if not bool(torch.isfinite(x).all()):
            fails.append(f"{label} colors: not finite")
        if bool((x[clamped] != 0).any()):
            fails.append(f"{label} colors: a clamped channel is not exactly 0")
        fails += compare_float("colors", x, ref.colors, [r.colors for r in r32s], S.fwd[None], ~clamped, label)[0]
    if case.v is None:
        return fails
    nz = case.v != 0
    sure = nz & ~adj & ~clamped                 # views that certainly pass their gradient on
    maybe = (nz & adj).any(0)                   # [n, 3]: some view of this channel may go either way
    live = sure.any(0) & ~maybe
    dead = ~sure.any(0) & ~maybe                # zero upstream in every view that is not clamped
    zero_rows = ~nz.any(0).any(-1)
    f_ok = torch.arange(case.dc.shape[1])[None, :] < case.Fs[:, None]                   # [n, F]
    tensors = {"v_rest": (S.bwd[:, None, :], torch.arange(max(K - 1, 0)) < nb - 1, None),
               "v_c": (S.bwd[:, None, :], torch.arange(K) < nb, None),
               "v_dc": (S.bwd_dc, None, f_ok)}
    caps = {}
    for name, (St, band_ok, fmask) in tensors.items():
        x = getattr(got, name, None)
        if x is None or x.numel() == 0:
            continue
        x = x.detach().cpu()
        valid = torch.ones(x.shape[:2], dtype=torch.bool) if fmask is None else fmask
        if not bool(torch.isfinite(x[valid]).all()):
            fails.append(f"{label} {name}: not finite")
        if band_ok is not None:
            valid = valid & band_ok[None, :]
            if bool((x[:, ~band_ok] != 0).any()):
                fails.append(f"{label} {name}: a band above the active degree is not exactly 0")
        if bool((x[zero_rows] != 0).any()):
            fails.append(f"{label} {name}: a row with all-zero upstream gradient is not all zero")
        if bool((x[valid[:, :, None] & dead[:, None, :]] != 0).any()):
            fails.append(f"{label} {name}: the gradient of a clamped channel is not exactly 0")
        fl, caps[name] = compare_float(name, x, getattr(ref, name), [getattr(r, name) for r in r32s], St,
                                       valid[:, :, None] & live[:, None, :], label)
        fails += fl
    # clamp-adjacent channels: the gated or the ungated definition, view by view
    Bst = torch.stack(ref.B, dim=-1)                                                   # [V, n, nb]
    w = weights(case)
    v64 = case.v.double()
    for i, c in torch.nonzero(maybe).tolist():
        views = torch.nonzero(nz[:, i, c] & adj[:, i, c])[:, 0].tolist()
        assert len(views) <= 8, (label, "clamp-adjacent views of one channel", len(views))
        base = sure[:, i, c].double() * v64[:, i, c]
        ok = False
        for bits in range(1 << len(views)):
            g = base.clone()
            for j, r in enumerate(views):
                if bits >> j & 1:
                    g[r] = v64[r, i, c]
            vc = torch.zeros(K, dtype=torch.float64)
            vc[:nb] = (Bst[:, i, :] * g[:, None]).sum(0) * case.scale
            good = True
            for name, (St, _b, _f) in tensors.items():
                x = getattr(got, name, None)
                if x is None or x.numel() == 0:
                    continue
                x = x.detach().cpu().double()
                if name == "v_dc":
                    Fi = int(case.Fs[i])
                    e = scaled_error(x[i, :Fi, c], w[i, :Fi] * vc[0], S.bwd_dc[i, :Fi, c])
                else:
                    e = scaled_error(x[i, :, c], vc[1:] if name == "v_rest" else vc, S.bwd[i, c].expand(x.shape[1]))
                good = good and bool((e <= caps.get(name, 2.0 ** -22)).all())
            ok = ok or good
        if not ok:
            fails.append(f"{label}: row {i} channel {c} (clamp-adjacent) matches neither the gated nor the ungated gradient")
    return fails


def duplicates_equal(case, tensors, label=""):
    """Violations of: the rows ``dup[:, 1]`` are bit-identical to the rows ``dup[:, 0]`` they copy (row axis -2 of
    [V, n, 3] colours, 0 of gradients)."""
    fails = []
    if case.dup.numel() == 0:
        return fails
    for name, (t, axis) in tensors.items():
        if t is None or t.numel() == 0:
            continue
        t = t.detach().cpu()
        if not torch.equal(t.index_select(axis, case.dup[:, 0]), t.index_select(axis, case.dup[:, 1])):
            fails.append(f"{label} {name}: a copied row differs from the row it copies")
    return fails


# ---------------------------------------------------------------------------------------------- input families
def _unit(g, n):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return d / d.norm(dim=-1, keepdim=True)


def _generic_dirs(n, g, lo=-3.0):
    return torch.randn(n, 3, generator=g) * 10.0 ** (torch.rand(n, 1, generator=g) * (4.0 - lo) + lo)


def _edge_dirs(g):
    """26 rows: the six axis directions, the twelve coordinate-plane diagonals, eight near-pole rows."""
    rows = []
    for a in range(3):
        for s in (1.0, -1.0):
            e = [0.0, 0.0, 0.0]
            e[a] = s
            rows.append(e)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                e = [0.0, 0.0, 0.0]
                e[a], e[b] = sa, sb
                rows.append(e)
    d = torch.tensor(rows)
    z = torch.tensor([1.0, -1.0] * 4) * 10.0 ** (torch.rand(8, generator=g) * 4.0 - 2.0)
    pole = torch.stack([1e-4 * z * torch.randn(8, generator=g), 1e-4 * z * torch.randn(8, generator=g), z], dim=-1)
    return torch.cat([d, pole])


def _rotations(M, g):
    q, r = torch.linalg.qr(torch.randn(M, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    q[:, :, 0] *= torch.linalg.det(q)[:, None]
    q[0] = torch.eye(3, dtype=torch.float64)
    return q


def pose_table(R, t):
    """[M, 16] rows: R row-major, t, an (unused) identity quaternion."""
    M = R.shape[0]
    return torch.cat([R.reshape(M, 9), t, torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=R.dtype).expand(M, 4)], 1).float()


def make_case(kind, n, k, deg, family="generic", seed=0, F=1, table=False, poses=False, post=False, V=1, form="dirs",
              fourier=False):
    """One seeded case.  kind: plain | split | fused | parts | multi | views.
    plain / split: directions are given (split: DC = a plain leaf over the first rows, then — with ``fourier`` — a Fourier
    sum over the others); fused: ``F`` with ``table`` (ids + an idft table wider than F), ``poses`` (ids + pose table);
    parts: PARTS_ROWS, F alternating 1 / 5, part = object; multi: ``form`` dirs | means; views: V cameras, post on."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * n + 3 * k + deg)
    if kind == "parts":
        rows = list(PARTS_ROWS)
        n = sum(rows)
    if kind == "views":
        post = True
    posed = poses or (kind == "multi" and form == "means")
    given = kind in ("plain", "split") or (kind == "multi" and form == "dirs")
    V = V if kind in ("multi", "views") else 1
    # directions of view 0
    if family == "far_object":
        d0 = (_unit(g, n) * 10.0 ** (torch.rand(n, 1, generator=g, dtype=torch.float64) + 1.0)).float()
    else:
        # (behind a pose table a direction is ``R m + t - cam`` with |t| ~ 3: below length 1 it is all cancellation, which is
        # the far_object family's subject — the posed generic rows keep to 10^U(0, 4))
        d0 = _generic_dirs(n, g, lo=0.0 if posed else -3.0)
        if family == "edges":
            e = _edge_dirs(g)[:n]
            d0[: e.shape[0]] = e
    if deg == 0 and not posed:
        idx = torch.arange(n)
        d0[idx % 5 == 0] = 0.0                                           # zero norm: degree 0 must never look at it
        if kind == "plain":
            d0[idx % 5 == 2] = math.nan
    # copies: the first rows again at the end, in a later 64-row span (and, for the parts, in a later part)
    d = 0 if n < 65 else min(32, n - 64)
    if kind == "parts":
        d = 20
    dup = torch.stack([torch.arange(d), torch.arange(n - d, n)], dim=1) if d else torch.zeros(0, 2, dtype=torch.int64)
    case = SimpleNamespace(kind=kind, n=n, k=k, deg=deg, post=bool(post), scale=0.5 if kind == "multi" else 1.0,
                           dirs=None, means=None, cams=None, ids=None, poses=None, idft=None, dup=dup, rows=None,
                           family=family)
    # objects
    M = 6 if kind == "parts" else 4
    if kind == "parts":
        case.rows = rows
        ids = torch.repeat_interleave(torch.arange(M, dtype=torch.int32), torch.tensor(rows))
        Fp = torch.tensor([1, 5, 1, 5, 1, 5])
        # the copies: the first 20 rows of part 3 again at the end of part 5; both parts share their pose and idft rows
        lo = sum(rows[:3])
        case.dup = dup = torch.stack([torch.arange(lo, lo + d), torch.arange(n - d, n)], dim=1)
    elif kind == "split":
        first = max(1, n // 3) if n > 1 else 1
        ids = torch.cat([torch.zeros(first, dtype=torch.int32), torch.ones(n - first, dtype=torch.int32)])
        Fp = torch.tensor([1, 5 if fourier else 1])
        case.rows = [first, n - first]
        if d:                                    # copies inside the second part
            case.dup = dup = torch.stack([torch.arange(first, first + d), torch.arange(n - d, n)], dim=1)
            assert first + d <= n - d
    else:
        ids = torch.randint(0, M, (n,), generator=g).to(torch.int32)
        Fp = torch.full((M,), F)
    use_ids = kind in ("parts", "split") or table or posed
    if use_ids:
        case.ids = ids
    Fmax = int(Fp.max()) if use_ids else F
    case.Fs = Fp[ids.long()] if use_ids else torch.full((n,), F)
    if kind == "parts" or table or (kind == "split" and fourier):
        case.idft = torch.randn(M, Fmax + 3, generator=g)
        if kind == "split":
            case.idft = case.idft[:, :Fmax].contiguous()
            case.idft[0] = 1.0
    if not given:
        if family == "far_object":
            centre = 1e3 * torch.tensor([0.6, -0.5, 0.62], dtype=torch.float64)
            t = centre + 5.0 * torch.randn(M, 3, generator=g, dtype=torch.float64)
            cam0 = centre + torch.tensor([3.0, 1.0, -2.0], dtype=torch.float64)
        else:
            t = 3.0 * torch.randn(M, 3, generator=g, dtype=torch.float64)
            t[0] = 0.0
            cam0 = torch.tensor(CAM0, dtype=torch.float64)
        cams = [cam0] + [cam0 + torch.round(8.0 * torch.randn(3, generator=g, dtype=torch.float64)) / 4.0
                         for _ in range(V - 1)]
        case.cams = torch.stack(cams).float()
        world = case.cams[0].double() + d0.double()
        if posed:
            R = _rotations(M, g)
            if kind == "parts":
                R[5], t[5] = R[3], t[3]
            case.poses = pose_table(R, t)
            world = torch.einsum("nji,nj->ni", R[ids.long()], world - t[ids.long()])       # R^T (world - t)
        case.means = world.float()
    else:
        case.dirs = torch.stack([d0] + [_generic_dirs(n, g) for _ in range(V - 1)])
    if kind == "parts" and case.idft is not None:
        case.idft[5] = case.idft[3]
    # coefficients and upstream gradients
    dc_scale = 4.0 if (deg <= 1 and kind in ("fused", "parts", "views")) else 1.0
    case.dc = dc_scale * torch.randn(n, Fmax, 3, generator=g)
    case.dc = torch.where((torch.arange(Fmax)[None, :] < case.Fs[:, None])[:, :, None], case.dc, torch.zeros(()))
    case.rest = torch.randn(n, k - 1, 3, generator=g)
    v = torch.randn(V, n, 3, generator=g)
    v[:, torch.rand(n, generator=g) < 0.1] = 0.0
    if V > 1:
        v[torch.rand(V, n, generator=g) < 0.05] = 0.0
    case.v = v
    # planted clamp-adjacent channels: every 97th row, channel 0 of view 0 put onto the clamp's threshold (not at degree
    # 0 for more than 8 views: there every view sees the same colour, and `check` tries each subset of adjacent views)
    if case.post and n >= 97 and not (deg == 0 and V > 8):
        rows_p = torch.arange(48, n - d, 97)
        pre = definition(case).pre[0, rows_p, 0]
        b0w = 0.5 * math.sqrt(1.0 / math.pi) * weights(case)[rows_p, 0]
        case.dc[rows_p, 0, 0] = (case.dc[rows_p, 0, 0].double() - pre / b0w).float()
    # the copies
    if dup.numel():
        src, dst = dup[:, 0], dup[:, 1]
        for name in ("means", "dc", "rest"):
            t_ = getattr(case, name)
            if t_ is not None:
                t_[dst] = t_[src]
        for name in ("dirs", "v"):
            t_ = getattr(case, name)
            if t_ is not None:
                t_[:, dst] = t_[:, src]
        if case.ids is not None and kind not in ("parts", "split"):
            case.ids[dst] = case.ids[src]
            case.Fs[dst] = case.Fs[src]
    return case


# ---------------------------------------------------------------------------------------------- the cases of the GPU test
# n = 257: four full spans plus one row (a second block whose first wave is partial), every valid (k, deg), on the edge
# rows; the sizes around one span and 4097 at three (k, deg) on generic rows.
SIZES = [(257, k, d, "edges") for k, d in VALID] + \
        [(n, k, d, "generic") for n in (1, 63, 64, 65, 4097) for k, d in ((16, 3), (25, 4), (1, 0))]
# sh_fwd_kernel's grid is capped at 1536 blocks of WAVES waves (4 at K <= 16, 2 at K = 25), one 64-row span per wave and
# trip: the prefetching loop takes a second trip from n > 1536 * WAVES * 64 rows on.  + 65: that trip's first block
# holds one full span and a one-row span.
GRID_CAP = 1536
GRID_SIZES = [(GRID_CAP * 4 * 64 + 65, 16, 3, "generic"), (GRID_CAP * 2 * 64 + 65, 25, 4, "generic")]
# spec id -> seed, where seed 0 does not keep the clamp shares / the gate margin (test_sh_fp64.py checks every case)
SEEDS = {"fused-n1-k1-d0-generic-F5-poses0-post1-table1": 1, "fused-n1-k1-d0-generic-F5-poses1-post1-table1": 3,
         "parts-n323-k9-d1-edges-poses1-post1": 1, "views-n1-k16-d3-generic-V16": 1, "views-n1-k25-d4-generic-V16": 1,
         "views-n1-k1-d0-generic-V3": 1}


def spec_id(s):
    extra = "".join(f"-{key}{int(val) if isinstance(val, bool) else val}" for key, val in sorted(s.items())
                    if key not in ("kind", "n", "k", "deg", "family"))
    return f"{s['kind']}-n{s['n']}-k{s['k']}-d{s['deg']}-{s['family']}{extra}"


def specs(kind):
    """The keyword sets of ``make_case`` that the GPU test runs for one surface."""
    base = [dict(kind=kind, n=n, k=k, deg=d, family=f) for n, k, d, f in SIZES]
    far = dict(kind=kind, n=257, k=16, deg=3, family="far_object")
    if kind == "plain":
        return base + [dict(kind=kind, n=n, k=k, deg=d, family=f) for n, k, d, f in GRID_SIZES]
    if kind == "split":
        return [dict(s, fourier=fo) for s in base if s["k"] > 1 for fo in (False, True)]
    if kind == "fused":
        out = [dict(s, F=F, table=tb, poses=po, post=ps) for s in base for F, tb in ((1, False), (5, True))
               for po in (False, True) for ps in (False, True)]
        return out + [dict(far, F=F, table=tb, poses=True, post=ps) for F, tb in ((1, False), (5, True))
                      for ps in (False, True)]
    if kind == "parts":
        out = [dict(kind=kind, n=sum(PARTS_ROWS), k=k, deg=d, family="edges", poses=po, post=ps) for k, d in VALID
               if k > 1 for po in (False, True) for ps in (False, True)]
        return out + [dict(far, n=sum(PARTS_ROWS), poses=True, post=ps) for ps in (False, True)]
    if kind == "multi":
        return [dict(s, V=V, form=fm) for s in base for V in (1, 3) for fm in ("dirs", "means")]
    if kind == "views":
        return [dict(s, V=V) for s in base for V in (1, 3, 16)]
    raise KeyError(kind)


def case_of(spec):
    return make_case(seed=SEEDS.get(spec_id(spec), 0), **spec)

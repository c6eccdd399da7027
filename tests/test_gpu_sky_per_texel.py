"""GPU (-m gpu): the sky cube-map kernels (csrc/cubemap.hip) texel by texel against an fp64 sum over the oracle's taps.

The existing sky tests compare the texture gradient in rel-L2, because their reference builds the ray directions with a
matmul and the kernel with FMAs.  Here both sides see the same directions bit for bit (`c_oracle.sky_dirs` restates the
kernels' `sky_dir` operation by operation; the forward comparison below checks it), so the bilinear taps are identical
and the only legitimate error in the texture gradient is fp32 summation order.  Per touched texel t, with the
contributions w*g of the oracle's taps (`c_oracle.cube_taps`):

    |v_tex[t] - sum w*g| <= (n_t + 2) 2^-24 sum |w*g|      (n_t + 4 for sky_blend: w * (g * (1 - a)) rounds twice more)

and every texel no tap reaches must be exactly 0.  That bound holds whichever order the segmented scan, the LDS window
and the global atomics add in, and it fails on a lost or doubled run sum, a dropped sign or a channel mix-up.

The views (tests/sky_views.py; tests/test_sky_views.py shows on the CPU that each reaches its target) cover the
reference's configuration (1920x1280, fx = 2000, R = 1024, eval and jittered), magnified and minified lookups, face
seams and cube corners, invalid directions on tiles' corner pixels, C in {1, 2, 4, 5, 8} and the layouts.
"""
import numpy as np
import pytest
import torch

import sky_views as SV

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
VIEWS = SV.all_views()
CASES = [(name, entry) for name, v in VIEWS.items() for entry in v.entries]
_TAPS = {}


@pytest.fixture(scope="module")
def sky():
    from sgn_rast import _lib, sky as S
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return S


def _camera_taps(CO, v):
    """(dirs [n,3], off [n,4], w [n,4]) of the view's camera (the fused kernels' directions), cached for one view."""
    if v.name not in _TAPS:
        _TAPS.clear()
        d = CO.sky_dirs(v.h, v.w, v.fx, v.fy, v.cx, v.cy, v.c2w(), v.jitter)
        _TAPS[v.name] = (d,) + CO.cube_taps(d, v.R)
    return _TAPS[v.name]


def _upstream(n, C, seed):
    """Signed values (the kernel skips zero run sums, so signs matter), a block of exact zeros, a few large entries."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, C, generator=g)
    v[n // 5: n // 5 + max(1, n // 10)] = 0.0
    v[torch.randint(0, n, (max(2, n // 4000),), generator=g)] *= 1000.0
    return v


def _family(name):
    return name.split("/")[0]


def _check_texture_grad(v_tex, off, w, gpix, R, C, slack, label):
    """v_tex (device, 6*R*R*C) against the fp64 sum of w * gpix over the taps; returns the largest |err| / bound."""
    T = 6 * R * R
    off = off.numpy().reshape(-1).astype(np.int64)
    ok = off >= 0
    idx = off[ok]
    wk = w.numpy().reshape(-1)[ok].astype(np.float64)
    pix = np.repeat(np.arange(off.size // 4), 4)[ok]
    cnt = np.bincount(idx, minlength=T)
    touched = np.nonzero(cnt)[0]
    touched_d = torch.from_numpy(touched).to(DEV)
    vt = v_tex.detach().reshape(T, C)
    got = vt[touched_d].double().cpu().numpy()
    worst = 0.0
    for c in range(C):
        contrib = wk * gpix[pix, c]
        ref = np.bincount(idx, contrib, T)[touched]
        M = np.bincount(idx, np.abs(contrib), T)[touched]
        bound = (cnt[touched] + slack) * U * M
        err = np.abs(got[:, c] - ref)
        bad = np.nonzero(err > bound)[0]
        if bad.size:
            j = bad[np.argmax(err[bad] / np.maximum(bound[bad], 1e-300))]
            t = int(touched[j])
            raise AssertionError(
                f"{label}: {bad.size} of {touched.size} touched texels outside the bound in channel {c}; worst texel "
                f"{t} (face {t // (R * R)}, iy {t % (R * R) // R}, ix {t % R}): got {got[j, c]!r} want {ref[j]!r} "
                f"bound {bound[j]:.3g} (n {cnt[t]}, sum|wg| {M[j]:.3g})")
        live = bound > 0
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
    mask = torch.ones(T, dtype=torch.bool, device=DEV)
    mask[touched_d] = False
    stray = int((vt[mask] != 0).sum())
    assert stray == 0, f"{label}: {stray} non-zero cells on texels no tap reaches"
    return worst


def _report(name, entry, ratio):
    print(f"\nSKY_PER_TEXEL {_family(name)} {name} {entry} max|err|/bound {ratio:.3g}")


@pytest.mark.parametrize("name,entry", CASES, ids=[f"{n}:{e}" for n, e in CASES])
def test_sky_kernels_per_texel(sky, c_oracle, name, entry):
    CO = c_oracle
    v = VIEWS[name]
    seed = sum(map(ord, name + entry))                      # (stable across processes, unlike hash())
    g = torch.Generator().manual_seed(seed)
    R, C = v.R, v.C
    jit = None if v.jitter is None else v.jitter.to(DEV)
    if entry == "texture":
        dirs = v.texture_dirs(CO)
        B = dirs.shape[0]
        tex = torch.randn(B, 6, R, R, C, generator=g)
        t_d = tex.to(DEV).requires_grad_(True)
        out = sky.texture(t_d, dirs.to(DEV))
        n = dirs[0].reshape(-1, 3).shape[0]
        gout = torch.stack([_upstream(n, C, seed + b) for b in range(B)], 0)
        out.backward(gout.reshape(out.shape).to(DEV))
        ratio = 0.0
        for b in range(B):
            d = dirs[b].reshape(-1, 3)
            want = CO.cube_texture_f32(tex[b], d)
            got = out[b].detach().reshape(-1, C).cpu()
            assert torch.equal(got, want), (b, int((got != want).sum()))
            off, w = CO.cube_taps(d, R)
            ratio = max(ratio, _check_texture_grad(t_d.grad[b], off, w, gout[b].double().numpy(), R, C, 2,
                                                   f"{name}:texture[{b}]"))
        _report(name, entry, ratio)
        return

    d, off, w = _camera_taps(CO, v)
    n = v.h * v.w
    tex = torch.randn(6, R, R, C, generator=g)
    t_d = tex.to(DEV).requires_grad_(True)
    sky_ref = CO.cube_texture_f32(tex, d)
    gout = _upstream(n, C, seed)
    if entry == "sky":
        out = sky.sky_color(t_d, v.h, v.w, v.fx, v.fy, v.cx, v.cy, v.c2w(DEV), jit)
        got = out.detach().reshape(-1, C).cpu()
        assert torch.equal(got, sky_ref), int((got != sky_ref).sum())
        out.backward(gout.reshape(v.h, v.w, C).to(DEV))
        _report(name, entry, _check_texture_grad(t_d.grad, off, w, gout.double().numpy(), R, C, 2, f"{name}:sky"))
        return

    assert entry == "blend" and C == 3
    rgb = torch.rand(n, 3, generator=g) * 1.4               # some above the clamp
    rgb[torch.randint(0, n, (max(2, n // 1000),), generator=g)] = 1.0   # the clamp passes the gradient at 1
    alpha = torch.rand(n, generator=g)
    alpha[: n // 8] = 1.0
    alpha[n // 8: n // 4] = 0.0
    r_d = rgb.reshape(v.h, v.w, 3).to(DEV).requires_grad_(True)
    a_d = alpha.reshape(v.h, v.w).to(DEV).requires_grad_(True)
    out, s_out = sky.sky_blend(t_d, r_d, a_d, v.fx, v.fy, v.cx, v.cy, v.c2w(DEV), jit)
    got_s = s_out.reshape(-1, 3).cpu()
    assert torch.equal(got_s, sky_ref), int((got_s != sky_ref).sum())
    want = CO.sky_blend_f32(sky_ref, rgb, alpha)
    got = out.detach().reshape(-1, 3).cpu()
    assert torch.equal(got, want), int((got != want).sum())
    out.backward(gout.reshape(v.h, v.w, 3).to(DEV))
    # v_rgb: g * a where rgb <= 1 (one rounding, same as torch's), 0 above the clamp
    v_rgb = r_d.grad.reshape(-1, 3).cpu()
    assert torch.equal(v_rgb, torch.where(rgb <= 1, gout * alpha[:, None], torch.zeros(()))), "v_rgb"
    # v_alpha: sum_c g (min(r,1) - sky), an fmaf chain over the three channels
    g64, r64, s64 = gout.double(), rgb.double().clamp(max=1.0), sky_ref.double()
    va_ref = (g64 * (r64 - s64)).sum(1)
    va_bound = 8 * U * (g64.abs() * (r64.abs() + s64.abs())).sum(1)
    va_err = (a_d.grad.reshape(-1).cpu().double() - va_ref).abs()
    bad = va_err > va_bound
    assert not bool(bad.any()), (int(bad.sum()), float((va_err / va_bound.clamp(min=1e-300)).max()))
    gpix = (g64 * (1.0 - alpha.double())[:, None]).numpy()
    _report(name, entry, _check_texture_grad(t_d.grad, off, w, gpix, R, C, 4, f"{name}:blend"))

"""CPU: the rolling-shutter model on the oracle alone (tests/rolling_shutter_oracle.py: the contract of
include/sgn_rast.h restated in torch, and the time-sliced truth) — zero motion is the identity bit for bit, the
compensated render beats the global-shutter one against the truth on the four motions of profiles/rolling_shutter.md, the
margin recovers Gaussians that sit just off the image at mid-exposure — and what needs no GPU of the product: the host's
``ValueError``s and the C entries' argument checks (the non-NULL "pointers" below are never dereferenced: every call
returns at its argument checks)."""
import ctypes
import math

import pytest
import torch

import rolling_shutter_oracle as RO
import test_abi as TA
from oracle import torch_oracle as O
from sgn_rast import scenes, shutter

# measured on this oracle in float64 (profiles/rolling_shutter.md): gains over the uncompensated render of 14.90, 27.80,
# 15.47 and 13.87 dB on the four motions, 10.84 dB of margin 16 over margin 0 on the top 8 rows; the thresholds are the
# smallest measured value minus 3 dB
MOTION_GAIN_DB = 10.8
MARGIN_GAIN_DB = 7.8


def _f64(cam, raw):
    cam = scenes.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat.double(), cam.cam_pos.double())
    return cam, {k: v.double() for k, v in raw.items()}


def _projection(cam, raw, rs=None):
    means, scales, quats, _ = RO._activated(raw)
    return O.project_gaussians(means, scales, 1, quats, cam.viewmat[:3], cam.fx, cam.fy,
                               *shutter.projection_frame(cam, rs), RO.BLOCK)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("axis", ["rows", "cols"])
@pytest.mark.parametrize("duration", [0.03, -0.03])
def test_zero_motion_is_the_identity_bit_for_bit(axis, duration):
    cam, raw = RO.scene()
    xys, depths, radii, conics, _, nth, _ = _projection(cam, raw)
    assert xys.dtype == torch.float32 and int((radii > 0).sum()) > 100 and int((radii == 0).sum()) > 0
    rs = shutter.RollingShutter((0, 0, 0), (0, 0, 0), duration, axis, margin=0)
    out = RO.apply(xys, depths, radii, conics, cam, rs)
    for got, want in zip(out[:5], (xys, depths, radii, conics, nth)):
        assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", list(RO.MOTIONS))
def test_compensated_render_beats_global_shutter_against_time_sliced_truth(name):
    lin, ang, T, axis = RO.MOTIONS[name]
    cam, raw = _f64(*RO.scene())
    rs = shutter.RollingShutter(lin, ang, T, axis)
    truth = RO.truth_image(O, raw, cam, rs, band_kw=True)
    plain, comp = RO.psnr(RO.plain_image(O, raw, cam), truth), RO.psnr(RO.compensated_image(O, raw, cam, rs), truth)
    print(f"[rolling shutter oracle] {name}: uncompensated {plain:.2f} dB, compensated {comp:.2f} dB, gain {comp - plain:.2f}")
    assert comp - plain >= MOTION_GAIN_DB, (plain, comp)


def test_margin_recovers_gaussians_just_off_the_image():
    lin, ang, T, axis = RO.EDGE_MOTION
    cam, raw = _f64(*RO.edge_scene())
    truth = RO.truth_image(O, raw, cam, shutter.RollingShutter(lin, ang, T, axis), band_kw=True)[:8]
    got = {m: RO.psnr(RO.compensated_image(O, raw, cam, shutter.RollingShutter(lin, ang, T, axis, margin=m))[:8], truth)
           for m in (0, 8, 16)}
    plain = RO.psnr(RO.plain_image(O, raw, cam)[:8], truth)
    print(f"[rolling shutter oracle] top 8 rows: uncompensated {plain:.2f} dB, margin 0 / 8 / 16: "
          f"{got[0]:.2f} / {got[8]:.2f} / {got[16]:.2f} dB")
    assert got[16] - got[0] >= MARGIN_GAIN_DB, got
    assert got[0] > plain


def test_radius_is_conservative_and_exact_without_motion():
    """ceil(r sigma) against the exact 3-sigma radius of the sheared footprint, float64: never below it."""
    lin, ang, T, axis = RO.MOTIONS["fast"]
    cam, raw = _f64(*RO.scene())
    rs = shutter.RollingShutter(lin, ang, T, axis, margin=0)
    xys, depths, radii, conics, _, _, _ = _projection(cam, raw, rs)
    out = RO.apply(xys, depths, radii, conics, cam, rs)
    alive = out[5].alive
    q = out[3][alive]
    det = q[:, 0] * q[:, 2] - q[:, 1] ** 2
    mid = 0.5 * (q[:, 0] + q[:, 2]) / det                     # covariance = conic^-1: its larger eigenvalue
    lam = mid + torch.sqrt(torch.clamp(mid * mid - 1.0 / det, min=0.0))
    assert bool((out[2][alive].double() >= 3.0 * torch.sqrt(lam) - 1e-9).all())
    assert bool((out[2][alive] >= radii[alive]).all())


def test_viewmat_at_is_the_exponential_of_the_camera_twist():
    cam = scenes.make_camera(64, 48, 60.0, yaw=0.3)
    rs = shutter.RollingShutter((1.0, 0.5, 4.0), (0.2, -0.4, 0.1), 0.03)
    assert torch.equal(shutter.viewmat_at(cam, rs, 0.0), cam.viewmat)
    c64 = scenes.Camera(64, 48, 60.0, 60.0, 32.0, 24.0, cam.viewmat.double(), cam.cam_pos)
    # a one-parameter group: the step to 2 t is the step to t taken twice, and the step to -t undoes it
    inv0 = torch.linalg.inv(c64.viewmat)
    s1, s2, sm = (shutter.viewmat_at(c64, rs, t) @ inv0 for t in (0.01, 0.02, -0.01))
    assert float((s1 @ s1 - s2).abs().max()) < 1e-12 and float((s1 @ sm - torch.eye(4, dtype=torch.float64)).abs().max()) < 1e-12
    # first order: a world point's camera-frame velocity is -l - w x p
    l, w = shutter.camera_twist(cam, rs)
    p = torch.tensor([0.4, -0.2, 5.0, 1.0], dtype=torch.float64)
    h = 1e-3
    pc = (c64.viewmat @ p)[:3]
    vel = ((shutter.viewmat_at(c64, rs, h) @ p)[:3] - (shutter.viewmat_at(c64, rs, -h) @ p)[:3]) / (2 * h)
    assert float((vel - (-l - torch.linalg.cross(w, pc))).abs().max()) < 1e-5


# ---------------------------------------------------------------- the host's errors, before anything launches

@pytest.mark.parametrize("kw", [dict(axis="diagonal"), dict(axis=0), dict(margin=-1), dict(margin=1.5),
                                dict(duration=math.nan), dict(duration=math.inf), dict(lin_vel=(0.0, math.nan, 0.0)),
                                dict(ang_vel=(0.0, 0.0, math.inf)), dict(lin_vel=(0.0, 1.0))])
def test_rolling_shutter_is_validated_on_the_host(kw):
    args = dict(lin_vel=(0.0, 0.0, 1.0), ang_vel=(0.0, 0.1, 0.0), duration=0.03)
    args.update(kw)
    with pytest.raises(ValueError):
        shutter.RollingShutter(**args)


def test_entries_refuse_what_is_not_a_rolling_shutter():
    from sgn_rast import step
    cam, raw = RO.scene(8)
    P = step.leaf_params(raw)
    for call in (lambda: step.render(P, cam, 0, rolling_shutter="rows"),
                 lambda: step.render_fused(P, cam, 0, rolling_shutter=0.03),
                 lambda: step.render_eval(P, cam, torch.zeros(3), rolling_shutter=(1, 2, 3)),
                 lambda: step.train_step(P, cam, torch.zeros(48, 64, 3), torch.zeros(48, 64), rolling_shutter=True),
                 lambda: step.render_scene_graph([P], torch.zeros(1, 16), torch.ones(1, 1), cam, rolling_shutter="x"),
                 lambda: step.render_fused(P, cam, 0, object_velocities=torch.zeros(1, 3))):
        with pytest.raises(ValueError):
            call()
    rs = shutter.RollingShutter((0, 0, 1), (0, 0, 0), 0.03)
    z = torch.zeros
    with pytest.raises(ValueError):
        shutter.apply(z(4, 2), z(4), z(4, dtype=torch.int32), z(4, 3), z(4, dtype=torch.int32), cam, rs, 16,
                      object_ids=z(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        shutter.apply(z(4, 3), z(4), z(4, dtype=torch.int32), z(4, 3), z(4, dtype=torch.int32), cam, rs, 16)


# ---------------------------------------------------------------- the C entries' argument checks (no GPU)

NAMES = ("sgn_rolling_shutter_fwd", "sgn_rolling_shutter_bwd")
P_ = 1          # a non-NULL pointer


def _lib():
    from sgn_rast import _lib
    return _lib, _lib.load()


def _st(**kw):
    from sgn_rast import _lib
    s = _lib.Shutter()
    s.fx = s.fy = 60.0
    s.cx, s.cy, s.duration, s.clip_thresh = 32.0, 24.0, 0.03, 0.01
    s.img_h, s.img_w, s.block_width = 48, 64, 16
    for k, v in kw.items():
        setattr(s, k, v)
    return ctypes.byref(s)


def _fwd(lib, n=4, ins=(P_,) * 4, ids=None, table=None, m=0, st=None, outs=(P_,) * 5):
    return lib.sgn_rolling_shutter_fwd(n, *ins, ids, table, m, st if st is not None else _st(), *outs, None)


def _bwd(lib, n=4, ins=(P_,) * 4, ids=None, table=None, m=0, st=None, vs=(P_, None, P_), outs=(P_,) * 3):
    return lib.sgn_rolling_shutter_bwd(n, *ins, ids, table, m, st if st is not None else _st(), *vs, *outs, None)


def test_entries_are_declared_exported_and_bound():
    L, lib = _lib()
    fns = TA._header_functions()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in zip(NAMES, (15, 16)):
        assert name in fns and name in L.SIGNATURES, name
        assert fns[name] == nargs and len(L.SIGNATURES[name][1]) == nargs, name
        assert hasattr(raw, name) and getattr(lib, name).restype is ctypes.c_int, name
    assert ctypes.sizeof(L.Shutter) == 18 * 4            # the struct of include/sgn_rast.h, field for field


def test_nothing_to_do_returns_before_any_launch():
    _, lib = _lib()
    assert _fwd(lib, n=0, ins=(None,) * 4, outs=(None,) * 5) == 0
    assert _bwd(lib, n=0, ins=(None,) * 4, vs=(None,) * 3, outs=(None,) * 3) == 0


@pytest.mark.parametrize("call,name", [(_fwd, NAMES[0]), (_bwd, NAMES[1])])
def test_bad_arguments_are_refused_with_a_message(call, name):
    _, lib = _lib()
    bad = [dict(n=-1), dict(st=_st(axis=2)), dict(st=_st(img_h=0)), dict(st=_st(block_width=32)),
           dict(st=_st(block_width=1)), dict(st=_st(fx=0.0)), dict(st=_st(margin=-1.0)),
           dict(ids=P_), dict(table=P_, m=3), dict(ids=P_, table=P_, m=0)]
    for k in range(4):
        ins = [P_] * 4
        ins[k] = None
        bad.append(dict(ins=tuple(ins)))
    n_out = 5 if call is _fwd else 3
    for k in range(n_out):
        outs = [P_] * n_out
        outs[k] = None
        bad.append(dict(outs=tuple(outs)))
    if call is _bwd:
        bad += [dict(vs=(None, None, P_)), dict(vs=(P_, None, None))]
    for kw in bad:
        assert call(lib, **kw) < 0, kw
        assert name.encode() in lib.sgn_last_error(), (kw, lib.sgn_last_error())
    assert lib.sgn_rolling_shutter_fwd(4, P_, P_, P_, P_, None, None, 0, None, P_, P_, P_, P_, P_, None) == -2

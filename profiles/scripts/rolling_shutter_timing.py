"""The rolling-shutter kernel pair at 1 M rows beside the same pass written as torch expressions on the device
(tests/rolling_shutter_oracle.py run on device tensors, forward and autograd backward).  Run it once under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/scripts/rolling_shutter_timing.py`,
in a run of its own, for the per-kernel figures of profiles/rolling_shutter.md; the device-event medians it prints
itself need no profiler."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "street-gaussians-ns_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import rolling_shutter_oracle as RO  # noqa: E402
from sgn_rast import fused, scenes, shutter  # noqa: E402

DEV = "cuda"
N = 1_000_000
CALLS, BLOCKS = 20, 5


def timed(fn):
    """Median over BLOCKS of the device-event time of CALLS calls, per call, in microseconds."""
    for _ in range(3):
        fn()
    per = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / CALLS)
    return statistics.median(per)


def main():
    cam = scenes.make_camera(1920, 1280, 2000.0, device=DEV)
    raw = scenes.make_gaussians(N, scenes.make_camera(1920, 1280, 2000.0), seed=0, device=DEV)
    rs = shutter.RollingShutter((0.3, 0.0, 6.0), (0.0, 0.6, 0.0), 0.03)
    with torch.no_grad():
        xys, depths, radii, conics, _, nth, _ = fused.project_gaussians_fused(
            raw["means"], raw["log_scales"], raw["quats"], cam.viewmat[:3, :], cam.fx, cam.fy,
            *shutter.projection_frame(cam, rs), 16)
    ids = (torch.arange(N, device=DEV) % 3).to(torch.int32)
    vel = torch.tensor([[0.0, 0.0, 0.0], [4.0, 0.0, 1.0], [-2.0, 0.0, 5.0]], device=DEV)
    v = (torch.randn(N, 2, device=DEV), torch.randn(N, device=DEV), torch.randn(N, 3, device=DEV))
    print(f"rows {N}, visible after the projection {int((radii > 0).sum())}")

    for name, kw in (("camera only", {}), ("object table", dict(object_ids=ids, object_velocities=vel))):
        x, d, q = (t.clone().requires_grad_(True) for t in (xys, depths, conics))
        with torch.no_grad():
            t_fwd = timed(lambda: shutter.apply(x, d, radii, q, nth, cam, rs, 16, **kw))
        out = shutter.apply(x, d, radii, q, nth, cam, rs, 16, **kw)
        print(f"{name}: visible after the pass {int((out[2] > 0).sum())}")
        t_bwd = timed(lambda: torch.autograd.backward((out[0], out[1], out[3]), v, retain_graph=True))
        print(f"{name}: sgn_rolling_shutter_fwd {t_fwd:.2f} us  sgn_rolling_shutter_bwd {t_bwd:.2f} us per call "
              f"(host launch + autograd node included)")

    # the same pass as torch expressions on the device
    cam_c = RO.cam_cpu(cam)
    lin, ang = (t.to(DEV) for t in RO.camera_velocities(cam_c, rs))
    x, d, q = (t.clone().requires_grad_(True) for t in (xys, depths, conics))
    expr = lambda: RO.shear(x, d, radii, q, cam_c, lin, ang, rs.duration, rs.axis, margin=rs.margin)
    with torch.no_grad():
        t_fwd = timed(expr)
    out = expr()
    t_bwd = timed(lambda: torch.autograd.backward((out[0], out[1], out[3]), v, retain_graph=True))
    print(f"torch expressions: forward {t_fwd:.1f} us  backward {t_bwd:.1f} us per call")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()

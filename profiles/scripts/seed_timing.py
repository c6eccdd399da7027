"""LiDAR seeding timing (csrc/seed.hip via sgn_rast.seed.seed_sweep) on the MI355X: one Waymo-sized call — 180 k points,
32 boxes, a 1920x1280 image — device-event and wall time after warm-up, median of --reps, next to the wall time of the
numpy restatement (tests/seed_oracle.py, float32) on the same host, with the bytes one call moves and the GB/s that
implies.  The outputs are compared with the oracle's on the way.  Each step runs in a child process under its own time
limit; a step that fails ends the run.  Prints one JSON line.

    python profiles/scripts/seed_timing.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "street-gaussians-ns_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

N, BOXES, WIDTH, HEIGHT = 180_000, 32, 1920, 1280
STEP_LIMIT_S = {"gpu": 240, "oracle": 240}


def inputs():
    import seed_oracle as SO
    sc = SO.scene(N, BOXES, 2024, width=WIDTH, height=HEIGHT, focal=1440.0, cx=951.6, cy=634.4)
    return SO, sc, SO.image(3, HEIGHT, WIDTH)


def step_oracle(reps):
    import numpy as np
    SO, sc, img = inputs()
    SO.seed_sweep(sc, img)
    t = []
    for _ in range(max(3, reps // 4)):
        t0 = time.perf_counter()
        out = SO.seed_sweep(sc, img)
        t.append(time.perf_counter() - t0)
    return {"oracle_wall_ms_median": round(1e3 * float(np.median(t)), 2), "oracle_totals_tail": out["totals"][-2:],
            "oracle_object_rows": out["offsets"][-1]}


def step_gpu(reps):
    import numpy as np
    import torch
    from sgn_rast import seed
    assert torch.cuda.is_available(), "seed_timing needs the GPU"
    SO, sc, img = inputs()
    pts, imgd = torch.from_numpy(sc["points"]).cuda(), torch.from_numpy(img).cuda()
    cam = seed.SeedCamera(sc["w2c"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["width"], sc["height"])
    call = lambda: seed.seed_sweep(pts, sc["l2w"], sc["boxes"], cam, imgd, min_z=sc["min_z"])
    for _ in range(3):
        obj, bg = call()
    torch.cuda.synchronize()
    exp = SO.seed_sweep(sc, img)
    same = (obj.offsets == exp["offsets"] and torch.equal(obj.local.cpu(), torch.from_numpy(exp["local"]))
            and torch.equal(obj.rgb.cpu(), torch.from_numpy(exp["obj_rgb"]))
            and torch.equal(obj.src.cpu(), torch.from_numpy(exp["obj_src"]))
            and torch.equal(bg.world.cpu(), torch.from_numpy(exp["world"]))
            and torch.equal(bg.rgb.cpu(), torch.from_numpy(exp["bg_rgb"]))
            and torch.equal(bg.src.cpu(), torch.from_numpy(exp["bg_src"])) and bg.n_live == exp["totals"][-1])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    wall = []
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[2 * r].record()
        call()
        ev[2 * r + 1].record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    ms = [ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(reps)]
    m, k = obj.offsets[-1], bg.world.shape[0]
    ok_rows = int(torch.unique(torch.cat([obj.src, bg.src])).numel())
    nblk = (N + 255) // 256
    moved = {"points_read_twice": 2 * 12 * N, "verdict_words_written_and_read": 2 * 12 * N,
             "block_counts_written_scanned_read": 4 * 4 * nblk * (BOXES + 2), "pixels_read": 3 * ok_rows,
             "rows_written": 19 * (m + k), "src_widened_to_int64": 12 * (m + k)}
    total = sum(moved.values())
    med = float(np.median(ms))
    return {"device": torch.cuda.get_device_name(0), "n": N, "boxes": BOXES, "image": [HEIGHT, WIDTH],
            "object_rows": m, "background_rows": k, "live": bg.n_live, "equals_float32_oracle": bool(same),
            "gpu_ms_median": round(med, 4), "gpu_ms_min": round(float(np.min(ms)), 4),
            "wall_ms_median": round(1e3 * float(np.median(wall)), 4), "bytes_moved": moved, "bytes_total": total,
            "implied_GBps": round(total / (med * 1e-3) / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None, help="run one step in this process")
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"gpu": step_gpu, "oracle": step_oracle}[a.step](a.reps)))
        return 0
    res = {}
    for step in ("gpu", "oracle"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {STEP_LIMIT_S[step]} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"step {step} failed (exit {p.returncode}); stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return p.returncode or 1
        res.update(json.loads(p.stdout.strip().splitlines()[-1]))
    res["oracle_over_gpu_wall"] = round(res["oracle_wall_ms_median"] / res["wall_ms_median"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

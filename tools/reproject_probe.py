#!/usr/bin/env python3
"""Cost of reprojecting the previous view's frame on the headline scene: Cornell 800x800 (depth 16,
aTolerance 0), a progressive session of the moved camera after one 32-sample step, blended with
the previous camera's frame by pr.reprojected(). Timed with HIP events (Camera.reproject_times):
the guide passes, the gather kernel and the whole device span - first call of a session (both
views' guide passes) and a later call (the session's guides kept) - beside the wall time of the
call with its copies, and of cam.reproject() on host frames. Each after warm-up, three repeats,
median. One JSON line."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

RO = {"width": 800, "samples": 256, "depth": 16, "aTolerance": 0}
MOVE = (0.5, 0.2, -0.2)
STEP, WARMUP, REPEATS = 32, 2, 3


def main():
    import numpy as np
    import raytracer_amd as rt
    sd = rt.generate_scene_data({"type": "cornell"})
    moved = {**sd, "camera": {**sd["camera"], "from": [a + b for a, b in zip(sd["camera"]["from"], MOVE)]}}
    prev_cam = rt.create_camera_from_scene_data(sd, {**RO, "samples": STEP})
    cam = rt.create_camera_from_scene_data(moved, RO)
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    prad = np.zeros((H, W, 3), np.float32)
    fresh = np.zeros((H, W, 3), np.float32)
    out = np.zeros((H, W, 3), np.float32)
    wgt = np.zeros((H, W), np.float32)
    prev_cam.render(rgb, radiance=prad)
    runs = []
    for r in range(WARMUP + REPEATS):
        with cam.progressive() as pr:
            pr.step(STEP, rgb, radiance=fresh)
            t0 = time.perf_counter()
            pr.reprojected(prev_cam, prad, rgb, out, wgt)
            first_wall = (time.perf_counter() - t0) * 1e3
            first = cam.reproject_times()
            t0 = time.perf_counter()
            pr.reprojected(prev_cam, prad, rgb, out, wgt)
            again_wall = (time.perf_counter() - t0) * 1e3
            again = cam.reproject_times()
        t0 = time.perf_counter()
        cam.reproject(prev_cam, prad, radiance=fresh, samples=STEP, rgb=rgb, out=out, weight_out=wgt)
        host_wall = (time.perf_counter() - t0) * 1e3
        host = cam.reproject_times()
        if r >= WARMUP:
            runs.append({"first_guide_ms": first["guide_ms"], "first_reproject_ms": first["reproject_ms"],
                         "first_total_ms": first["total_ms"], "first_wall_ms": first_wall,
                         "again_guide_ms": again["guide_ms"], "again_reproject_ms": again["reproject_ms"],
                         "again_total_ms": again["total_ms"], "again_wall_ms": again_wall,
                         "camera_guide_ms": host["guide_ms"], "camera_reproject_ms": host["reproject_ms"],
                         "camera_total_ms": host["total_ms"], "camera_wall_ms": host_wall})
    res = {k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]}
    res.update({"build": rt.build_id(), "frame": f"{W}x{H}", "step_samples": STEP,
                "share": round(float((wgt > 0).mean()), 4)})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the variance-guided preview beside the existing filter's, in one run: Cornell 800x800
(depth 16, aTolerance 0), a progressive session after one 32-sample step. Timed with HIP events
(Camera.denoise_times) on a later call of the session (guides kept): each level of
pr.denoised() and of pr.denoised(variance=True), the variance pass (the variance-guided call's
guide span once the guides are kept), the whole device span and the wall time of either call,
and the wall time of pr.variance(). Each after warm-up, three repeats, median. One JSON line."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

RO = {"width": 800, "samples": 256, "depth": 16, "aTolerance": 0}
STEP, WARMUP, REPEATS = 32, 2, 3


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    import numpy as np
    import raytracer_amd as rt
    sd = rt.generate_scene_data({"type": "cornell"})
    cam = rt.create_camera_from_scene_data(sd, RO)
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    var = np.zeros((H, W), np.float32)
    runs = []
    for r in range(WARMUP + REPEATS):
        with cam.progressive() as pr:
            pr.step(STEP, rgb)
            pr.denoised(rgb, rad)                       # (the session's guide pass)
            old_wall = timed(lambda: pr.denoised(rgb, rad))
            old = cam.denoise_times()
            pr.denoised(rgb, rad, variance=True)
            new_wall = timed(lambda: pr.denoised(rgb, rad, variance=True))
            new = cam.denoise_times()
            map_wall = timed(lambda: pr.variance(var))
        if r >= WARMUP:
            runs.append({"old_total_ms": old["total_ms"], "old_wall_ms": old_wall, "var_total_ms": new["total_ms"],
                         "var_wall_ms": new_wall, "variance_pass_ms": new["guide_ms"], "variance_map_wall_ms": map_wall,
                         **{f"old_level{k}_ms": v for k, v in enumerate(old["level_ms"])},
                         **{f"var_level{k}_ms": v for k, v in enumerate(new["level_ms"])}})
    out = {k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]}
    out.update({"build": rt.build_id(), "levels": len(new["level_ms"]), "lds_staged_levels": [0, 1],
                "frame": f"{W}x{H}", "step_samples": STEP})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

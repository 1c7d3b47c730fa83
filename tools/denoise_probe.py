#!/usr/bin/env python3
"""Cost of the denoised preview on the headline scene: Cornell 800x800 (depth 16, aTolerance 0),
a progressive session after one 32-sample step. Timed with HIP events (Camera.denoise_times):
the guide pass, each filter level and the whole device span of pr.denoised() - first call of a
session (guide pass included) and a later call (guides kept) - beside the wall time of the call
and of the 32-sample step itself. Each after warm-up, three repeats, median. One JSON line."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

RO = {"width": 800, "samples": 256, "depth": 16, "aTolerance": 0}
STEP, WARMUP, REPEATS = 32, 2, 3


def main():
    import numpy as np
    import raytracer_amd as rt
    sd = rt.generate_scene_data({"type": "cornell"})
    cam = rt.create_camera_from_scene_data(sd, RO)
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    runs = []
    for r in range(WARMUP + REPEATS):
        with cam.progressive() as pr:
            t0 = time.perf_counter()
            pr.step(STEP, rgb)
            step_wall = (time.perf_counter() - t0) * 1e3
            step_path, step_accum = cam.kernel_times()
            t0 = time.perf_counter()
            pr.denoised(rgb)
            first_wall = (time.perf_counter() - t0) * 1e3
            first = cam.denoise_times()
            t0 = time.perf_counter()
            pr.denoised(rgb)
            again_wall = (time.perf_counter() - t0) * 1e3
            again = cam.denoise_times()
        if r >= WARMUP:
            runs.append({"step_wall_ms": step_wall, "step_kernels_ms": step_path + step_accum,
                         "guide_ms": first["guide_ms"], "first_total_ms": first["total_ms"],
                         "first_wall_ms": first_wall, "again_total_ms": again["total_ms"],
                         "again_wall_ms": again_wall,
                         **{f"level{k}_ms": v for k, v in enumerate(again["level_ms"])}})
    out = {k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]}
    levels = sum(v for k, v in out.items() if k.startswith("level"))
    out.update({"build": rt.build_id(), "levels": len(again["level_ms"]), "levels_sum_ms": round(levels, 4),
                "guide_plus_levels_ms": round(out["guide_ms"] + levels, 4),
                "lds_staged_levels": [0, 1], "frame": f"{W}x{H}", "step_samples": STEP})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the sub-pixel coverage pass at 800 px: Cornell 800x800 (brute force), spheres-500
800x800 and rain 800 px (the tree), K = 2 and 4. Timed with HIP events (Camera.coverage_time)
around render_coverage's pass, beside the guide pass (Camera.denoise_times of a denoise call) and,
on Cornell, the four filter levels and the whole device span of a denoise call with and without
hold_edges. Each after two warm-ups, three repeats, median. One JSON line per scene."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

SCENES = [("cornell", {"type": "cornell"}, {"width": 800}),
          ("spheres500", {"type": "spheres", "options": {"count": 500, "seed": 42}}, {"width": 800, "aspect": 1}),
          ("rain", {"type": "rain", "options": {"seed": 42}}, {"width": 800})]
WARMUP, REPEATS = 2, 3


def main():
    import numpy as np
    import raytracer_amd as rt
    for name, cfg, ro in SCENES:
        cam = rt.create_camera_from_scene_data(rt.generate_scene_data(cfg), {**ro, "samples": 4, "depth": 8})
        H, W = cam.image_height, cam.image_width
        rad = np.full((H, W, 3), 0.5, np.float32)
        runs = []
        for r in range(WARMUP + REPEATS):
            row = {}
            for k in (2, 4):
                cov = cam.render_coverage(k=k)
                row[f"coverage_k{k}_ms"] = cam.coverage_time()
                row[f"mixed_k{k}"] = float(cov["mixed"].mean())
            cam.denoise(rad, out=rad)
            t = cam.denoise_times()
            row.update(guide_ms=t["guide_ms"], levels_sum_ms=sum(t["level_ms"]), denoise_total_ms=t["total_ms"])
            cam.denoise(rad, out=rad, hold_edges=4)
            row.update(denoise_hold4_total_ms=cam.denoise_times()["total_ms"], hold4_coverage_ms=cam.coverage_time())
            rad[:] = 0.5
            if r >= WARMUP:
                runs.append(row)
        out = {k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]}
        out.update(scene=name, frame=f"{W}x{H}", build=rt.build_id())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

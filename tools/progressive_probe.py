#!/usr/bin/env python3
"""Cost of progressive rendering on the headline config (Cornell 800x800 spp 256 depth 16,
aTolerance 0): (a) a one-shot render_region, (b) a session in 1 step of 256, (c) a session in
8 steps of 32. Each after warm-up, three repeats, median: wall ms per frame and the
kernel_times() split (path / accumulate ms, summed over a session's steps). One JSON line per
variant, then the per-step walls of (c)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

RO = {"width": 800, "samples": 256, "depth": 16, "aTolerance": 0}
WARMUP, REPEATS = 2, 3


def main():
    import numpy as np
    import raytracer_amd as rt
    sd = rt.generate_scene_data({"type": "cornell"})
    cam = rt.create_camera_from_scene_data(sd, RO)
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)

    def one_shot():
        t0 = time.perf_counter()
        cam.render_region(rgb, (0, 0, W, H))
        wall = (time.perf_counter() - t0) * 1e3
        p, a = cam.kernel_times()
        return wall, p, a, [wall]

    def session(steps):
        def run():
            t0 = time.perf_counter()
            walls, p, a = [], 0.0, 0.0
            with cam.progressive() as pr:
                t_begin = (time.perf_counter() - t0) * 1e3
                for n in steps:
                    t1 = time.perf_counter()
                    pr.step(n, rgb)
                    walls.append((time.perf_counter() - t1) * 1e3)
                    kp, ka = cam.kernel_times()
                    p, a = p + kp, a + ka
            return (time.perf_counter() - t0) * 1e3, p, a, [t_begin] + walls
        return run

    ref = None
    for name, fn in (("one_shot", one_shot), ("session_1x256", session([256])), ("session_8x32", session([32] * 8))):
        runs = []
        for r in range(WARMUP + REPEATS):
            res = fn()
            if r >= WARMUP:
                runs.append(res)
        wall, p, a = (float(np.median([x[k] for x in runs])) for k in range(3))
        if name == "one_shot":
            ref = rgb.copy()
        out = {"variant": name, "build": rt.build_id(), "wall_ms": round(wall, 3), "path_ms": round(p, 3),
               "accum_ms": round(a, 3), "walls_ms": [round(x[0], 3) for x in runs],
               "kernel": cam.last_kernel(), "frame_equals_one_shot": bool((rgb == ref).all())}
        if name != "one_shot":  # begin, then each step (median over the repeats)
            out["begin_and_step_walls_ms"] = [round(float(np.median([x[3][k] for x in runs])), 3)
                                              for k in range(len(runs[0][3]))]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

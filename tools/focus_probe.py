#!/usr/bin/env python3
"""Cost of a focused step on the headline scene: Cornell 800x800 (depth 16, aTolerance 0), a
progressive session after one 32-sample step. Timed with HIP events: the selection's device span
(score pass, four digit passes, compaction: focus_info's select_ms) for the session's variance and
for an uploaded map as the score, and the path + settle / resolve passes (kernel_times) of a
focused step of LEN samples at permille 250 against a plain step of LEN samples - beside the wall
time of each call with its copies. Every measurement on a session of its own after step(32), 2
warm-ups, median of 3. One JSON line."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

RO = {"width": 800, "samples": 256, "depth": 16, "aTolerance": 0}
FIRST, LEN, PERMILLE, WARMUP, REPEATS = 32, 8, 250, 2, 3


def main():
    import numpy as np
    import raytracer_amd as rt
    sd = rt.generate_scene_data({"type": "cornell"})
    cam = rt.create_camera_from_scene_data(sd, RO)
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rows = {"plain": [], "focus_variance": [], "focus_map": []}
    for r in range(WARMUP + REPEATS):
        for name in rows:
            with cam.progressive() as pr:
                pr.step(FIRST, rgb)
                score = pr.variance() if name == "focus_map" else None
                t0 = time.perf_counter()
                if name == "plain":
                    pr.step(LEN, rgb)
                else:
                    pr.focus(LEN, rgb, score=score, permille=PERMILLE)
                wall = (time.perf_counter() - t0) * 1e3
                path, settle = cam.kernel_times()
                row = {"wall_ms": wall, "path_ms": path, "settle_resolve_ms": settle}
                if name != "plain":
                    info = pr.focus_info
                    row.update(select_ms=info["select_ms"], selected=info["selected"], active=info["active"])
                if r >= WARMUP:
                    rows[name].append(row)
    res = {"build": rt.build_id(), "frame": f"{W}x{H}", "first_step": FIRST, "len": LEN, "permille": PERMILLE}
    for name, runs in rows.items():
        res[name] = {k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

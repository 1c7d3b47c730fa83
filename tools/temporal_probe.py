#!/usr/bin/env python3
"""Cost of accumulating a view onto a device-resident history on the headline scene: Cornell
800x800 (depth 16, aTolerance 0), a progressive session of the moved camera after one 32-sample
step, accumulated by pr.accumulated() onto a history that holds the previous camera's view. Timed
with HIP events (History.times): the guide + variance passes, the gather kernel, the filter and the
whole device span - without a filter and with filter_levels = 4 - beside the wall time of the call
with its copies, and beside pr.reprojected()'s numbers (tools/reproject_probe.py) measured in the
same process. Each after warm-up, three repeats, median. One JSON line."""
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
    prev_cam = rt.create_camera_from_scene_data(sd, {**RO, "seed": 1000})
    cam = rt.create_camera_from_scene_data(moved, {**RO, "seed": 1001})
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    prad = np.zeros((H, W, 3), np.float32)
    out = np.zeros((H, W, 3), np.float32)
    wgt = np.zeros((H, W), np.float32)
    runs = []
    with rt.History() as hist:
        with prev_cam.progressive() as pq:
            pq.step(STEP, rgb, radiance=prad)
            pq.accumulated(hist)
        for r in range(WARMUP + REPEATS):
            with cam.progressive() as pr:
                pr.step(STEP)
                pr.accumulated(hist, rgb, out, commit=False)          # the session's guide pass
                row = {}
                for key, levels in (("plain", 0), ("filtered", 4)):
                    t0 = time.perf_counter()
                    pr.accumulated(hist, rgb, out, commit=False, weight_out=wgt, filter_levels=levels)
                    row[f"{key}_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    row.update({f"{key}_{k}": v for k, v in hist.times().items()})
                t0 = time.perf_counter()
                pr.reprojected(prev_cam, prad, rgb, out, wgt)
                row["reproject_wall_ms"] = (time.perf_counter() - t0) * 1e3
                t = cam.reproject_times()
                row.update(reproject_gather_ms=t["reproject_ms"], reproject_total_ms=t["total_ms"])
            if r >= WARMUP:
                runs.append(row)
        res = {k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]}
        res.update({"build": rt.build_id(), "frame": f"{W}x{H}", "step_samples": STEP,
                    "share": round(float((wgt > 0).mean()), 4), "history_bytes": hist.info["bytes"]})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of accumulating a view onto a device-resident history through specular chains, 800 pixels
wide, on the default scene (800x450) and the mirror room (Cornell with a mirror for a back wall,
800x800): depth 16, aTolerance 0, a progressive session of the moved camera after one 32-sample
step, accumulated by pr.accumulated() onto a history that holds the previous camera's view - without
and with guides="specular" (each on a history of its own, committed the same way). Timed with HIP
events (History.times): the guide + variance passes (with the chain walk), the gather kernel, the
filter and the whole device span - the session's first call (its guide passes) and a later call
(guides kept), without a filter and with filter_levels = 4. Two warm-ups, three repeats, median.
One JSON line per scene."""
import copy
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

RO = {"width": 800, "samples": 256, "depth": 16, "aTolerance": 0}
MOVE = (0.5, 0.2, -0.2)
STEP, WARMUP, REPEATS = 32, 2, 3


def mirror_room(rt):
    sd = copy.deepcopy(rt.generate_scene_data({"type": "cornell"}))
    sd["materials"].append({"id": "mirror", "material": {"type": "metal", "color": [0.9, 0.9, 0.9], "fuzz": 0}})
    sd["objects"][2]["material"] = "mirror"
    return sd


def main():
    import numpy as np
    import raytracer_amd as rt
    for name, sd in (("default", rt.generate_scene_data({"type": "default"})), ("mirror_room", mirror_room(rt))):
        moved = {**sd, "camera": {**sd["camera"], "from": [a + b for a, b in zip(sd["camera"]["from"], MOVE)]}}
        prev_cam = rt.create_camera_from_scene_data(sd, {**RO, "seed": 1000})
        cam = rt.create_camera_from_scene_data(moved, {**RO, "seed": 1001})
        H, W = cam.image_height, cam.image_width
        rgb = np.zeros((H, W, 3), np.uint8)
        out = np.zeros((H, W, 3), np.float32)
        wgt = np.zeros((H, W), np.float32)
        kind = np.zeros((H, W), np.uint8)
        res = {}
        for tag, kw in (("plain", {}), ("chains", {"guides": "specular"})):
            runs = []
            with rt.History() as hist:
                with prev_cam.progressive() as pq:
                    pq.step(STEP)
                    pq.accumulated(hist, **kw)
                for r in range(WARMUP + REPEATS):
                    row = {}
                    with cam.progressive() as pr:
                        pr.step(STEP)
                        for call in ("first", "again"):
                            pr.accumulated(hist, rgb, out, commit=False, weight_out=wgt, **kw)
                            row.update({f"{tag}_{call}_{k}": v for k, v in hist.times().items() if k != "filter_ms"})
                        pr.accumulated(hist, rgb, out, commit=False, weight_out=wgt, filter_levels=4,
                                       **({**kw, "kind": kind} if kw else {}))
                        row.update({f"{tag}_filtered_{k}": v for k, v in hist.times().items()})
                    if r >= WARMUP:
                        runs.append(row)
                res.update({k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]})
                res[f"{tag}_share"] = round(float((wgt > 0).mean()), 4)
                res[f"{tag}_history_bytes"] = hist.info["bytes"]
        res.update({"scene": name, "build": rt.build_id(), "frame": f"{W}x{H}", "step_samples": STEP,
                    "kind2_share": round(float((kind == 2).mean()), 4)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

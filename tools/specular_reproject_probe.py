#!/usr/bin/env python3
"""Cost of reprojecting the previous view's frame through specular chains, 800 pixels wide, on the
default scene (800x450) and the mirror room (Cornell with a mirror for a back wall, 800x800): depth
16, aTolerance 0, a progressive session of the moved camera after one 32-sample step, blended with
the previous camera's frame by pr.reprojected(), without and with guides="specular". Timed with HIP
events (Camera.reproject_times): the guide passes, the gather kernel and the whole device span -
first call of a session (both views' guide passes: two without, four with the chains) and a later
call (the session's guides kept: the previous view's only). Each after warm-up, three repeats,
median. One JSON line per scene."""
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
        prev_cam = rt.create_camera_from_scene_data(sd, {**RO, "samples": STEP})
        cam = rt.create_camera_from_scene_data(moved, RO)
        H, W = cam.image_height, cam.image_width
        rgb = np.zeros((H, W, 3), np.uint8)
        prad = np.zeros((H, W, 3), np.float32)
        out = np.zeros((H, W, 3), np.float32)
        wgt = np.zeros((H, W), np.float32)
        kind = np.zeros((H, W), np.uint8)
        prev_cam.render(rgb, radiance=prad)
        runs = []
        for r in range(WARMUP + REPEATS):
            row = {}
            for tag, kw in (("first_hit", {}), ("chains", {"guides": "specular", "kind": kind})):
                with cam.progressive() as pr:
                    pr.step(STEP, rgb)
                    for call in ("first", "again"):
                        pr.reprojected(prev_cam, prad, rgb, out, wgt, **kw)
                        t = cam.reproject_times()
                        row.update({f"{tag}_{call}_guide_ms": t["guide_ms"], f"{tag}_{call}_gather_ms": t["reproject_ms"],
                                    f"{tag}_{call}_total_ms": t["total_ms"]})
                row[f"{tag}_share"] = float((wgt > 0).mean())
            if r >= WARMUP:
                runs.append(row)
        res = {k: round(float(np.median([x[k] for x in runs])), 4) for k in runs[0]}
        res.update({"scene": name, "build": rt.build_id(), "frame": f"{W}x{H}", "step_samples": STEP,
                    "kind2_share": round(float((kind == 2).mean()), 4)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

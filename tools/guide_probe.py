#!/usr/bin/env python3
"""Cost of the guide pass through the specular chain against the first-hit pass:
800x800, Cornell and the default scene, `guide_ms` of Camera.denoise_times() (HIP events around the
guide pass of cam.denoise) for guides="first_hit", "specular" and max_fuzz 0.25; 2 warm-ups, median
of 3. Also how many pixels the walk continued and its longest chain. One JSON line per scene."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

WARMUP, REPEATS = 2, 3
MODES = {"first_hit": "first_hit", "specular": "specular", "specular_fuzz0.25": {"max_fuzz": 0.25}}


def main():
    import numpy as np
    import raytracer_amd as rt
    for name in ("cornell", "default"):
        sd = rt.generate_scene_data({"type": name})
        cam = rt.create_camera_from_scene_data(sd, {"width": 800, "samples": 4, "depth": 8, "aTolerance": 0})
        H, W = cam.image_height, cam.image_width
        rad = np.zeros((H, W, 3), np.float32)
        cam.render(np.zeros((H, W, 3), np.uint8), radiance=rad)
        out = {"scene": name, "frame": f"{W}x{H}", "build": rt.build_id()}
        for tag, guides in MODES.items():
            ms = []
            for r in range(WARMUP + REPEATS):
                cam.denoise(rad, out=np.empty_like(rad), guides=guides)
                if r >= WARMUP:
                    ms.append(cam.denoise_times()["guide_ms"])
            out[f"{tag}_guide_ms"] = round(float(np.median(ms)), 4)
        for tag, kw in (("specular", {}), ("specular_fuzz0.25", {"max_fuzz": 0.25})):
            k = cam.render_guides(through_specular=True, **kw)["chain"] & 0xff
            out[f"{tag}_pixels_k1"] = round(float((k >= 1).mean()), 4)
            out[f"{tag}_k_max"] = int(k.max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

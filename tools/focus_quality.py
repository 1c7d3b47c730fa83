#!/usr/bin/env python3
"""What focused steps are worth at an equal sample budget, on the GPU (DESIGN.md §15's table).
Per scene: session U takes step(2 B); session F takes step(B) and then four focus(B, permille =
240) - never more samples than U (RenderStats). Error = display-domain MSE (mean squared error of
sqrt(clip(c, 0, 1)), tests/denoise_ref.py) against a one-shot frame of 1024 samples rendered with
ANOTHER seed, so the truth shares no sample with either session. F is run with the session's own
variance as the score and with the variance-guided filter's variance_out (recomputed before
every focused step). depth 8, aTolerance 0. One JSON line per scene and budget: mse of U, and F /
U for both scores, raw and through pr.denoised(variance=True)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))
sys.path.insert(0, str(ROOT / "tests"))

ROWS = [("cornell", {"width": 96}), ("cornell", {"width": 128}), ("default", {"width": 128}),
        ("rain_seed42", {"width": 128})]
BUDGETS = (8, 32)
PERMILLE, TRUTH_SPP = 240, 1024


def main():
    import numpy as np
    import raytracer_amd as rt
    from denoise_ref import display_mse
    for name, ro in ROWS:
        sd = json.loads((ROOT / "tests/golden" / f"scene_{name}.json").read_text())["scene"]
        ro = {**ro, "depth": 8, "aTolerance": 0, "samples": 512, "seed": 1}
        truth_cam = rt.create_camera_from_scene_data(sd, {**ro, "samples": TRUTH_SPP, "seed": 2})
        H, W = truth_cam.image_height, truth_cam.image_width
        truth = np.zeros((H, W, 3), np.float32)
        truth_cam.render(np.zeros((H, W, 3), np.uint8), radiance=truth)
        for b in BUDGETS:
            row = {"scene": name, "frame": f"{W}x{H}", "uniform_spp": 2 * b, "build": rt.build_id()}
            for variant in ("uniform", "session_variance", "filtered_variance"):
                cam = rt.create_camera_from_scene_data(sd, ro)
                rad = np.zeros((H, W, 3), np.float32)
                with cam.progressive() as pr:
                    if variant == "uniform":
                        st = pr.step(2 * b, radiance=rad)
                    else:
                        pr.step(b)
                        for _ in range(4):
                            score = None
                            if variant == "filtered_variance":
                                score = np.zeros((H, W), np.float32)
                                pr.denoised(variance=True, variance_out=score)
                            st = pr.focus(b, radiance=rad, score=score, permille=PERMILLE)
                    den = pr.denoised(variance=True)
                    var_sum = float(pr.variance().astype(np.float64).sum())
                row[variant] = {"samples": int(st.samples["total"]), "mse": display_mse(rad, truth),
                                "mse_denoised": display_mse(den, truth), "variance_sum": var_sum}
            u = row["uniform"]
            for variant in ("session_variance", "filtered_variance"):
                f = row[variant]
                assert f["samples"] <= u["samples"]
                f["mse_ratio"] = round(f["mse"] / u["mse"], 4)
                f["mse_denoised_ratio"] = round(f["mse_denoised"] / u["mse_denoised"], 4)
                f["variance_sum_ratio"] = round(f["variance_sum"] / u["variance_sum"], 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

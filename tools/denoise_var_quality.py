#!/usr/bin/env python3
"""What variance guidance is worth, CPU only (DESIGN.md §11's table): the NumPy restatements of
the existing filter (tests/denoise_ref.py) and of the variance-guided one
(tests/denoise_var_ref.py) on oracle frames against a converged oracle frame. Error = mean
squared error of sqrt(clip(c, 0, 1)); printed: after / before. The noisy frame and its variance
come from the oracle's sample window 2.. (denoise_var_ref.oracle_window). depth 8, aTolerance 0,
default filter parameters unless --sigma-variance is given."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

ROWS = [("cornell", {"width": 128}, 1024, (4, 8, 32, 128)),
        ("default", {"width": 128}, 512, (4, 32)),
        ("rain_seed42", {"width": 128}, 512, (8, 32)),
        ("spheres500_seed42", {"width": 96, "aspect": 1}, 512, (32,))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigma-variance", type=float, default=2.0)
    a = ap.parse_args()
    import pyoracle
    from denoise_ref import denoise_ref, display_mse, oracle_guides
    from denoise_var_ref import denoise_var_ref, oracle_window
    pyoracle.build()
    for name, ro, conv_spp, spps in ROWS:
        sd = json.loads((ROOT / "tests/golden" / f"scene_{name}.json").read_text())["scene"]
        ro = {**ro, "depth": 8, "aTolerance": 0}
        conv = pyoracle.render(sd, {**ro, "samples": conv_spp}, threads=16)["radiance"]
        n, P, dist, obj, _ = oracle_guides(pyoracle, sd, {**ro, "samples": 4})
        for spp in spps:
            noisy, var = oracle_window(pyoracle, sd, ro, spp)
            before = display_mse(noisy, conv)
            old = display_mse(denoise_ref(noisy, n, P, dist, obj), conv) / before
            new = display_mse(denoise_var_ref(noisy, var, n, P, dist, obj, sigma_variance=a.sigma_variance)[0],
                              conv) / before
            print(json.dumps({"scene": name, "frame": f"{conv.shape[1]}x{conv.shape[0]}", "spp": spp,
                              "converged_spp": conv_spp, "mse_before": before, "existing": round(old, 4),
                              "variance_guided": round(new, 4), "sigma_variance": a.sigma_variance}), flush=True)


if __name__ == "__main__":
    main()

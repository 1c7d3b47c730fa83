#!/usr/bin/env python3
"""What the edge hold is worth, CPU only (DESIGN.md's coverage table): the NumPy restatements of the
plain filter (tests/denoise_ref.py) and the variance-guided one (tests/denoise_var_ref.py), without
the hold and with it for K = 2 and 4 (tests/coverage_ref.py), on oracle frames against a converged
oracle frame. Error = mean squared error of sqrt(clip(c, 0, 1)); printed: after / before. The noisy
frame and its variance come from the oracle's sample window 2.. (denoise_var_ref.oracle_window).
depth 8, aTolerance 0, default filter parameters; scenes and sizes as tools/denoise_var_quality.py."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

ROWS = [("rain_seed42", {"width": 128}, 512, (8, 32)),
        ("spheres500_seed42", {"width": 96, "aspect": 1}, 512, (8, 32)),
        ("cornell", {"width": 128}, 1024, (4, 32)),
        ("default", {"width": 128}, 512, (8, 32))]


def main():
    import pyoracle
    from coverage_ref import coverage_ref, hold_ref, mixed_of
    from denoise_ref import denoise_ref, display_mse, oracle_guides
    from denoise_var_ref import denoise_var_ref, oracle_window
    pyoracle.build()
    for name, ro, conv_spp, spps in ROWS:
        sd = json.loads((ROOT / "tests/golden" / f"scene_{name}.json").read_text())["scene"]
        ro = {**ro, "depth": 8, "aTolerance": 0}
        conv = pyoracle.render(sd, {**ro, "samples": conv_spp}, threads=16)["radiance"]
        n, P, dist, obj, _ = oracle_guides(pyoracle, sd, {**ro, "samples": 4})
        masks = {k: mixed_of(coverage_ref(pyoracle, sd, {**ro, "samples": 4}, k), k) for k in (2, 4)}
        for spp in spps:
            noisy, var = oracle_window(pyoracle, sd, ro, spp)
            before = display_mse(noisy, conv)
            plain = denoise_ref(noisy, n, P, dist, obj)
            guided = denoise_var_ref(noisy, var, n, P, dist, obj)[0]
            row = {"scene": name, "frame": f"{conv.shape[1]}x{conv.shape[0]}", "spp": spp, "converged_spp": conv_spp,
                   "mse_before": before, "plain": round(display_mse(plain, conv) / before, 4),
                   "variance_guided": round(display_mse(guided, conv) / before, 4)}
            for k, m in masks.items():
                row[f"plain_hold{k}"] = round(display_mse(hold_ref(plain, noisy, m), conv) / before, 4)
                row[f"variance_guided_hold{k}"] = round(display_mse(hold_ref(guided, noisy, m), conv) / before, 4)
                row[f"mixed{k}"] = round(float(m.mean()), 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

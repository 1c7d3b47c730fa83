#!/usr/bin/env python3
"""What guides through the specular chain are worth, CPU only (DESIGN.md §16's table): the NumPy
restatements of the plain and the variance-guided filter (tests/denoise_ref.py,
tests/denoise_var_ref.py) on oracle frames, steered by the first-hit guides (oracle_guides) and by
the restated walk (tests/guide_walk_ref.py, max_fuzz 0 and 0.25), against a 1024-sample oracle frame
of another seed. Error = mean squared error of sqrt(clip(c, 0, 1)); printed per scene: the raw
frame's error, and after / raw for each filter, over the whole frame and over the pixels the walk
continued at least once (k >= 1) only. depth 8, aTolerance 0, default filter parameters. The noisy
frame and its variance come from the oracle's sample window 2.. (denoise_var_ref.oracle_window).
One JSON line per row."""
import argparse
import copy
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

CONVERGED_SPP, CONVERGED_SEED = 1024, 977
ROWS = [("default", {"width": 128}, (8, 32)),
        ("mirror_room", {"width": 96}, (8,)),
        ("rain_seed42", {"width": 128}, (8,)),
        ("spheres500_seed42", {"width": 96, "aspect": 1}, (8,))]


def golden(name):
    return json.loads((ROOT / "tests/golden" / f"scene_{name}.json").read_text())["scene"]


def mirror_room():
    """Cornell's JSON with its back wall (the third quad) a fuzz-0 metal."""
    sd = copy.deepcopy(golden("cornell"))
    sd["materials"].append({"id": "mirror", "material": {"type": "metal", "color": [0.9, 0.9, 0.9], "fuzz": 0}})
    sd["objects"][2]["material"] = "mirror"
    return sd


def mse(a, b, mask=None):
    with np.errstate(all="ignore"):
        da, db = np.sqrt(np.clip(a.astype(np.float64), 0, 1)), np.sqrt(np.clip(b.astype(np.float64), 0, 1))
    e = ((da - db) ** 2).mean(-1)
    return float(e.mean() if mask is None else e[mask].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", action="append", help="only these rows (default: all)")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import pyoracle
    from denoise_ref import denoise_ref, oracle_guides
    from denoise_var_ref import denoise_var_ref, oracle_window
    from guide_walk_ref import guide_walk_ref
    pyoracle.build()
    for name, ro, spps in ROWS:
        if a.scene and name not in a.scene:
            continue
        sd = mirror_room() if name == "mirror_room" else golden(name)
        ro = {**ro, "depth": 8, "aTolerance": 0}
        conv = pyoracle.render(sd, {**ro, "samples": CONVERGED_SPP, "seed": CONVERGED_SEED},
                               threads=a.threads)["radiance"]
        first = oracle_guides(pyoracle, sd, ro)[:4]
        walks = {mf: guide_walk_ref(pyoracle, sd, ro, 8, mf) for mf in (0.0, 0.25)}
        for spp in spps:
            noisy, var = oracle_window(pyoracle, sd, ro, spp)
            raw = mse(noisy, conv)
            fh = {"plain": denoise_ref(noisy, *first), "variance": denoise_var_ref(noisy, var, *first)[0]}
            row = {"scene": name, "frame": f"{conv.shape[1]}x{conv.shape[0]}", "spp": spp,
                   "converged_spp": CONVERGED_SPP, "mse_raw": raw,
                   **{f"first_hit_{k}": round(mse(v, conv) / raw, 4) for k, v in fh.items()}}
            for mf, w in walks.items():
                mask = (w[4] & 0xff) >= 1
                sp = {"plain": denoise_ref(noisy, *w[:4]), "variance": denoise_var_ref(noisy, var, *w[:4])[0]}
                tag = f"fuzz{mf:g}"
                row[f"{tag}_pixels_k1"] = round(float(mask.mean()), 4)
                for k in sp:
                    row[f"{tag}_specular_{k}"] = round(mse(sp[k], conv) / raw, 4)
                    if mask.any():
                        raw_m = mse(noisy, conv, mask)
                        row[f"{tag}_k1_first_hit_{k}"] = round(mse(fh[k], conv, mask) / raw_m, 4)
                        row[f"{tag}_k1_specular_{k}"] = round(mse(sp[k], conv, mask) / raw_m, 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What carrying the view history through specular chains is worth, CPU only (DESIGN.md §18's
table): the NumPy restatements (tests/temporal_ref.py, tests/specular_temporal_ref.py,
denoise_var_ref.py) on oracle frames, oracle first-hit guides and the restated walk
(tests/guide_walk_ref.py). Views k = 0 .. n-1 have `from` moved by k (0.125, 0.05, -0.05), 4 samples
per view (or --spp), seed 1000 + k, depth 8, aTolerance 0; truth is the last view at spp 1024 of
another seed. Error = mean squared error of sqrt(clip(c, 0, 1)) relative to the last view's fresh
frame, at the last view: the plain history ("plain") and the history through the chains ("chains"),
over the frame and over the k >= 1 pixels only ("k1_*"), unfiltered and through the variance-guided
filter (the plain one on the first-hit guides, the other on the chain guides). Also the share of
k >= 1 pixels, of those with a history, and their mean history length. Nothing is random. One JSON
line per row."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))

# (name, scene, width, aspect, views, max_fuzz)
ROWS = [("mirror room", "mirror_room", 64, None, 5, 0.0),
        ("default", "default", 128, None, 5, 0.0),
        ("cornell (glass ball)", "cornell", 64, None, 5, 0.0),
        ("spheres-200 (mirror balls)", "spheres200", 64, 1, 5, 0.0),
        ("sky-lit planar mirror facing a wall", "analytic", 32, None, 5, 0.0)]


def spheres200():
    import raytracer_amd as rt                       # the scene generator is host code
    return rt.generate_scene_data({"type": "spheres", "options": {"count": 200, "seed": 42}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--row", action="append", help="only these rows (default: all)")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import pyoracle
    from specular_reproject_ref import analytic_scene, golden_scene, mirror_room
    from specular_temporal_ref import oracle_trial
    pyoracle.build()
    scenes = {"mirror_room": mirror_room, "analytic": analytic_scene, "spheres200": spheres200}
    for name, scene, width, aspect, views, max_fuzz in ROWS:
        if a.row and name not in a.row:
            continue
        sd = scenes[scene]() if scene in scenes else golden_scene(scene)
        q = oracle_trial(pyoracle, sd, width, views=views, spp=a.spp, threads=a.threads, aspect=aspect, max_fuzz=max_fuzz)
        print(json.dumps({"scene": name, "views": views, "spp": a.spp, "max_fuzz": max_fuzz,
                          **{k: (round(v, 4) if isinstance(v, float) and k != "mse_fresh" else v) for k, v in q.items()}}),
              flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What reprojecting through specular chains is worth, CPU only (DESIGN.md §17's table): the NumPy
restatements (tests/reproject_ref.py, tests/specular_reproject_ref.py) on oracle frames, oracle
first-hit guides and the restated walk (tests/guide_walk_ref.py). View A is the scene's camera at
spp 256; view B has `from` moved, rendered fresh at spp 4 and blended with A's reprojected frame;
truth is B at spp 1024. depth 8, aTolerance 0, default parameters. Error = mean squared error of
sqrt(clip(c, 0, 1)). Printed per row: the share of pixels with k >= 1, of those with a history,
blend error / fresh error over the frame without ("first_hit") and with the chains ("chains"),
and over the k >= 1 pixels only ("k1_chains"); then the same for point_pixels 1 / 2 / 8 and for
through = 1 (mirrors only) beside the default 15. One JSON line per row."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

MOVE, SMALL = (0.5, 0.2, -0.2), (0.1, 0.05, -0.05)
VARIANTS = [{"point_pixels": 1.0}, {"point_pixels": 2.0}, {"point_pixels": 8.0}, {"through": 1}]
# (name, scene, width, aspect, move, max_fuzz)
ROWS = [("default", "default", 128, None, MOVE, 0.0),
        ("default, max_fuzz 0.25", "default", 128, None, MOVE, 0.25),
        ("mirror room", "mirror_room", 64, None, MOVE, 0.0),
        ("mirror room, small move", "mirror_room", 64, None, SMALL, 0.0),
        ("cornell", "cornell", 64, None, MOVE, 0.0),
        ("planar mirror facing a wall", "analytic", 32, None, MOVE, 0.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", action="append", help="only these rows (default: all)")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import pyoracle
    from specular_reproject_ref import analytic_scene, golden_scene, mirror_room, oracle_quality
    pyoracle.build()
    scenes = {"mirror_room": mirror_room, "analytic": analytic_scene}
    for name, scene, width, aspect, move, max_fuzz in ROWS:
        if a.row and name not in a.row:
            continue
        sd = scenes[scene]() if scene in scenes else golden_scene(scene)
        q = oracle_quality(pyoracle, sd, width, move, threads=a.threads, aspect=aspect, max_fuzz=max_fuzz,
                           variants=VARIANTS)
        rnd = lambda d: {k: (round(v, 4) if isinstance(v, float) and k != "mse_fresh" else v) for k, v in d.items()}  # noqa: E731
        row = {"scene": name, "move": list(move), "max_fuzz": max_fuzz, **rnd({k: v for k, v in q.items() if k != "variants"}),
               "variants": [rnd(v) for v in q["variants"]]}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

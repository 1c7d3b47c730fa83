#!/usr/bin/env python3
"""What reprojecting a previous view's frame is worth, CPU only (DESIGN.md §13's table): the
NumPy restatement (tests/reproject_ref.py) on oracle frames and oracle guides. View A is the
scene's camera at spp 256; view B has `from` moved, rendered fresh at spp 4 (or --fresh) and
blended with A's reprojected frame; truth is B at spp 1024. depth 8, aTolerance 0, default
parameters. Error = mean squared error of sqrt(clip(c, 0, 1)); printed: the share of pixels
with a history and blend error / fresh error. One JSON line per row."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

MOVES = [(0.1, 0.05, -0.05), (0.5, 0.2, -0.2), (1.5, 0.5, -0.5)]
ROWS = [("cornell", 64, MOVES[1:2]), ("cornell", 96, MOVES), ("default", 128, MOVES[1:2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fresh", type=int, default=4)
    a = ap.parse_args()
    import pyoracle
    from reproject_ref import oracle_quality
    pyoracle.build()
    for name, width, moves in ROWS:
        sd = json.loads((ROOT / "tests/golden" / f"scene_{name}.json").read_text())["scene"]
        for move in moves:
            q = oracle_quality(pyoracle, sd, width, move, spp_fresh=a.fresh)
            print(json.dumps({"scene": name, "frame": q["frame"], "move": list(move), "fresh_spp": a.fresh,
                              "share": round(q["share"], 4), "mse_fresh": q["mse_fresh"],
                              "ratio": round(q["ratio"], 4)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What accumulating across views is worth, CPU only (DESIGN.md §14's table): the NumPy
restatements (tests/temporal_ref.py, reproject_ref.py, denoise_var_ref.py) on oracle frames and
oracle guides. Views k = 0 .. n-1 have `from` moved by k (0.125, 0.05, -0.05), 4 samples per view
(or --spp), seed 1000 + k, depth 8, aTolerance 0; truth is the last view at spp 1024. Error = mean
squared error of sqrt(clip(c, 0, 1)) relative to the last view's fresh frame, at the last view, of:
chained reproject; the length-weighted accumulation; fresh + variance-guided filter; chained
reproject + the filter with the fresh variance; accumulation + the filter with the accumulated
variance. Nothing is random. One JSON line per row."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

ROWS = [("cornell", 64, 5), ("cornell", 64, 9), ("cornell", 96, 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    a = ap.parse_args()
    import pyoracle
    from temporal_ref import oracle_trial
    pyoracle.build()
    for name, width, views in ROWS:
        sd = json.loads((ROOT / "tests/golden" / f"scene_{name}.json").read_text())["scene"]
        q = oracle_trial(pyoracle, sd, width, views=views, spp=a.spp)
        print(json.dumps({"scene": name, "frame": q["frame"], "views": views, "spp": a.spp, "mse_fresh": q["mse_fresh"],
                          **{k: round(q[k], 4) for k in ("chained", "accumulated", "fresh_filtered", "chained_filtered",
                                                         "accumulated_filtered")}}), flush=True)


if __name__ == "__main__":
    main()

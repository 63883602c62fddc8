"""Measures what the default blur_ratio of mi355_sharp_params rests on, with the numpy restatement (tests/sharp_ref.py) on the seeded strips of
tests/sharp_patterns.py (blur_strip: 8 frames of 160 x 120 cut from a tests/synth texture, N(0, 2) noise and a gain in [0.95, 1.05] per frame,
frame 3 blurred by a separable Gaussian), and writes profiles/sharp_quality.json.  No GPU.

    python profiles/sharp_quality.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import oracle_lib                       # noqa: E402
from tests import sharp_patterns as sp             # noqa: E402

BLURRED = 3


def main():
    orc = oracle_lib.load_oracle()
    out = {"frames": 8, "frame": "160x120", "step": sp.QUALITY_STEP, "noise_sigma": 2, "gain_range": [0.95, 1.05], "blurred_frame": BLURRED,
           "seeds": list(sp.QUALITY_SEEDS), "pairs": "every frame with its next two", "offsets": "whole pixels", "per_sigma": {}}
    lowest_unblurred = []
    for seed in sp.QUALITY_SEEDS:
        er, st = sp.measure_strip(orc, seed, None, blurred=BLURRED)
        lowest_unblurred.append(float(er.min()))
    for sigma in sp.QUALITY_SIGMAS:
        row = {"blurred_exp_rel": [], "lowest_unblurred_exp_rel": []}
        for seed in sp.QUALITY_SEEDS:
            er, st = sp.measure_strip(orc, seed, sigma, blurred=BLURRED)
            row["blurred_exp_rel"].append(float(er[BLURRED]))
            row["lowest_unblurred_exp_rel"].append(float(np.delete(er, BLURRED).min()))
            lowest_unblurred.append(row["lowest_unblurred_exp_rel"][-1])
        out["per_sigma"]["%g" % sigma] = row
    out["min_lattice_points_per_pair"] = int(st["n"].min())
    lo = min(lowest_unblurred)
    hi15 = max(out["per_sigma"]["1.5"]["blurred_exp_rel"])
    out["lowest_unblurred_exp_rel"] = lo
    out["sigma_1.5_exp_rel_highest_seed"] = hi15
    out["separated_in_every_seed"] = all(u > b for u, b in zip(out["per_sigma"]["1.5"]["lowest_unblurred_exp_rel"], out["per_sigma"]["1.5"]["blurred_exp_rel"]))
    out["geometric_mean"] = float(np.sqrt(lo * hi15))
    out["blur_ratio_default"] = round(out["geometric_mean"], 2)
    out["margin_unblurred_over_default"] = lo / out["blur_ratio_default"]
    out["margin_default_over_sigma_1.5"] = out["blur_ratio_default"] / hi15
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "sharp_quality.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("lowest_unblurred_exp_rel", "sigma_1.5_exp_rel_highest_seed", "geometric_mean", "blur_ratio_default")}))


if __name__ == "__main__":
    main()

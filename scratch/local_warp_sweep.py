"""Sweep behind the defaults of mi355_default_local_warp_params (DESIGN, "local registration"): the numpy reference
(tests/local_warp_ref.py) on the synthetic surveys of tests/local_warp_cases.py, CPU only.

    python scratch/local_warp_sweep.py

Per parameter set, over the survey seeds: ratio = rms canvas disagreement of the ties after / before on the survey with smooth per-frame
fields of 2 px; harm = the largest |D| on the planar survey with 0.5 px of tie noise (what the step invents where there is nothing to fix).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import local_warp_cases as lc  # noqa: E402

SEEDS = (1, 2, 3, 4, 5)


def measure(**p):
    ratios, harms = [], []
    for seed in SEEDS:
        s = lc.survey(seed=seed, amp=2.0)
        _, grids, _ = lc.register(s, **p)
        ratios.append(lc.disagreement(s, grids) / lc.disagreement(s))
        s = lc.survey(seed=seed, amp=0.0, noise=0.5)
        _, grids, _ = lc.register(s, **p)
        harms.append(float(np.abs(grids).max()))
    return ratios, harms


def main():
    print("| smooth | prior | max_residual | max_shift | ratio mean (min .. max) | harm px mean (max) |")
    print("|---|---|---|---|---|---|")
    sets = [dict(smooth=sm, prior=pr) for sm in (0.0, 0.5, 2.0, 8.0, 32.0) for pr in (0.05, 0.25, 1.0, 4.0)]
    sets += [dict(max_residual=v) for v in (2.0, 4.0, 16.0)] + [dict(max_shift=v) for v in (1.0, 2.0, 4.0, 16.0)]
    sets += [dict(grid_x=4, grid_y=3), dict(grid_x=16, grid_y=12)]
    for p in sets:
        q = dict(lc.lr.DEFAULTS, **p)
        r, hm = measure(**p)
        tag = " grid %dx%d" % (q["grid_x"], q["grid_y"]) if "grid_x" in p else ""
        print("| %g | %g | %g | %g%s | %.3f (%.3f .. %.3f) | %.3f (%.3f) |" % (q["smooth"], q["prior"], q["max_residual"], q["max_shift"], tag,
                                                                            np.mean(r), min(r), max(r), np.mean(hm), max(hm)))


if __name__ == "__main__":
    main()

"""The parameter sweep behind pair verification's defaults (DESIGN, "pair verification"): the numpy reference (tests/verify_ref.py) on the
synthetic surveys of tests/verify_cases.py -- grid36, strip40d and the sparse +-2 strip -- seeds 1..5, at 5, 10 and 20 % wrong pairs.
Per parameter set and layout: wrong pairs kept / right pairs lost / frames lost, summed over the seeds, and the runs that were exact
(no wrong pair kept, no right pair lost, every frame labelled).  CPU only.

    python scratch/verify_sweep.py [--mutations]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import verify_cases as vc, verify_ref as vr  # noqa: E402

VARIANTS = [("defaults", {}), ("cycle_tol 3", dict(cycle_tol=3.0)), ("cycle_tol 12", dict(cycle_tol=12.0)), ("gate_abs 1.5", dict(gate_abs=1.5)),
            ("gate_abs 6", dict(gate_abs=6.0)), ("gate_k 2", dict(gate_k=2.0)), ("gate_k 8", dict(gate_k=8.0)), ("bridges 0", dict(bridges=0))]
MUTATIONS = [("n_ok >= 1 rule", dict(majority=False)), ("failed pairs bridge", dict(bridge_failed=True)), ("gate_k ignored", dict(use_gate_k=False))]


def main():
    variants = VARIANTS + (MUTATIONS if "--mutations" in sys.argv else [])
    for name in ("grid36", "strip40d", "strip30s"):
        for pct in (5, 10, 20):
            surveys = [vc.survey(name, seed, pct) for seed in (1, 2, 3, 4, 5)]
            for label, kw in variants:
                kw_, lr, fl, exact = 0, 0, 0, []
                for s in surveys:
                    out = vr.verify(s["recs"], s["n"], **kw)
                    a, b, c = int((out["kept"] & s["wrong"]).sum()), int((~out["kept"] & ~s["wrong"]).sum()), s["n"] - int(out["label"].sum())
                    kw_, lr, fl = kw_ + a, lr + b, fl + c
                    if a == 0 and b == 0 and c == 0:
                        exact.append(s["seed"])
                print("%-9s %2d %%  %-20s wrong kept %2d  right lost %3d  frames lost %2d  exact seeds %s" % (name, pct, label, kw_, lr, fl, exact), flush=True)


if __name__ == "__main__":
    main()

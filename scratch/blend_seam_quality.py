"""Quality of the multiband blend along optimised seams on the CPU restatement (tests/blend_seam_ref.py): on the crafted scenes of
tests/blend_seam_patterns.py, seamcut_ref.seam_disagreement of the owner map before (FindMasksByDistMap) and after (under the cell map), the
label stage's report and how the rectangle the seam runs through is owned.  Writes profiles/blend_seam_quality.json.  No GPU.

    python scratch/blend_seam_quality.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import blend_seam_patterns as bp      # noqa: E402
from tests import blend_seam_ref as bs           # noqa: E402
from tests import oracle_lib as ol               # noqa: E402
from tests import seamcut_ref as sc              # noqa: E402


def main():
    orc = ol.load_oracle()
    cases = {}
    for name in sorted(bp.CRAFTED):
        case, _, r = bp.reference(orc, name)
        s = r["set"]
        maps = bs.sample_maps(s, len(case.imgs))
        x, y, w, h = bp.crafted_rect(name)
        before, after = s["best"][y:y + h, x:x + w], r["best"][y:y + h, x:x + w]
        cases[name] = dict(params=case.p, report=r["report"],
                           disagreement_before=sc.seam_disagreement(maps, bs.owner_frames(s, s["best"])),
                           disagreement_after=sc.seam_disagreement(maps, bs.owner_frames(s, r["best"])),
                           rect=[x, y, w, h], rect_owned_before=[int((before == k).sum()) for k in (0, 1)],
                           rect_owned_after=[int((after == k).sum()) for k in (0, 1)], pixels_changed=int((s["best"] != r["best"]).sum()))
    out = dict(what="seam disagreement of the blend's owner map before / after the cell map, CPU restatement, library default costs", cases=cases)
    path = os.path.join(ROOT, "profiles", "blend_seam_quality.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in cases.items():
        print(k, v["disagreement_before"], "->", v["disagreement_after"], v["report"])


if __name__ == "__main__":
    main()

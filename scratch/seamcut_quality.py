"""Measures what the optimised seamlines (tests/seamcut_ref.py, the numpy restatement; the build gives the same bytes) do to the full-resolution
seam disagreement, and writes profiles/seamcut_quality.json.  No GPU.

    python scratch/seamcut_quality.py [OUT.json]

  * the search behind the crafted scenes of tests/seamcut_patterns.py and behind the diff_weight default: two or three 64 x 96 frames, frame 1
    24 px right of frame 0 (mid-seam at x = 43.5), a white rectangle that frame 1 alone has (moved) or that frame 0 has 6 px further left
    (relief), over a grid of positions, widths, heights and third-frame offsets.  A placement counts when the seamline render gives each of
    two frames at least 15 % of the rectangle asked about (frame 1's copy, or either copy in the relief case); it is a hit for a cost set when
    the seamcut render gives the rectangle one owner and the seam disagreement falls;
  * seamline and seamcut disagreement and the label report of every multi-frame case of tests/seamcut_patterns.py at its own parameters."""
import itertools
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from tests import gain_ref as gr, oracle_lib, seamcut_patterns as sp, seamcut_ref as sc, seamline_ref as sr  # noqa: E402
from tests.synth import texture  # noqa: E402

W, H, DX = 64, 96, 24
COSTS = [dict(diff_weight=1), dict(diff_weight=2), dict(diff_weight=4), dict(diff_weight=1, seam_penalty=8), dict(diff_weight=2, seam_penalty=8)]
OFF3 = ((12, 40), (12, 56), (40, 60))


def placements(relief):
    if relief:
        return itertools.product((44, 46, 48, 36, 38), (8, 12, 16, 20), ((40, 16), (36, 24), (44, 8)))
    return itertools.product((40, 36, 32), (8, 12, 16, 20, 24), ((44, 8), (40, 16), (44, 4), (36, 24)))


def search(orc):
    out = {}
    for frames, relief in itertools.product((2, 3), (False, True)):
        key = "%d frames, %s" % (frames, "relief" if relief else "moved object")
        counted, hits, found = 0, [0] * len(COSTS), []
        for (x0, rw, (y0, rh)), off3 in itertools.product(placements(relief), OFF3 if frames == 3 else OFF3[:1]):
            offs = [(0, 0), (DX, 0), off3][:frames]
            imgs = sp._cuts(texture(W + 40, H + 60, seed=301), offs, W, H)
            imgs[1][y0:y0 + rh, x0 - DX:x0 - DX + rw] = 255
            if relief:
                imgs[0][y0:y0 + rh, x0 - 6:x0 - 6 + rw] = 255
            h9s = sp._translations(offs)
            maps = gr.frame_sample_maps(orc, imgs, h9s)
            wmaps = sr.weight_maps(orc, imgs, h9s, 0, maps)
            s_owner = sr.pick(maps, wmaps)[1]
            before = sc.seam_disagreement(maps, s_owner)
            cand = sc.candidates(maps, wmaps, 2, 4)
            for xa in ((x0 - 6, x0) if relief else (x0,)):
                _, c = np.unique(s_owner[y0:y0 + rh, xa:xa + rw], return_counts=True)
                if len(c) < 2 or np.sort(c)[-2] < 0.15 * rw * rh or before == 0:
                    continue
                counted += 1
                for i, kw in enumerate(COSTS):
                    cells, rep = sc.labels(*cand, sc.params(level=2, **kw))
                    own = sc.render(maps, wmaps, cells, 2)[1]
                    after = sc.seam_disagreement(maps, own)
                    if len(np.unique(own[y0:y0 + rh, xa:xa + rw])) == 1 and after < before:
                        hits[i] += 1
                        if kw == dict(diff_weight=sc.DEFAULTS["diff_weight"]):
                            found.append({"rect_of_frame_1": [x0, y0, rw, rh], "asked_about_x": xa, "third_frame": list(off3) if frames == 3 else None,
                                          "seamline": before, "seamcut": after})
        out[key] = {"placements_astride": counted, "hits": {json.dumps(kw): h for kw, h in zip(COSTS, hits)}, "hits_at_the_default": found}
        print(key, counted, hits, file=sys.stderr, flush=True)
    return out


def cases(orc):
    out = {}
    for name in ("crafted2", "crafted3", "relief2", "relief3", "symmetric2", "projective", "skipped_level3", "level5", "staircase", "nine_depth4",
                 "nine_depth8", "twins", "twins_differ"):
        imgs, h9s, p, r = sp.reference(orc, name)
        s_owner = sr.pick(r["maps"], r["wmaps"])[1]
        out[name] = {"params": p, "seamline": sc.seam_disagreement(r["maps"], s_owner), "seamcut": sc.seam_disagreement(r["maps"], r["owner"]), "report": r["report"]}
    return out


def main():
    orc = oracle_lib.load_oracle()
    rec = {"what": __doc__, "cost_defaults": {k: sc.DEFAULTS[k] for k in ("data_weight", "diff_weight", "seam_penalty", "miss_cost")},
           "cases": cases(orc), "search": search(orc)}
    print(json.dumps(rec["cases"], indent=1))
    with open(sys.argv[1] if len(sys.argv) > 1 else "profiles/seamcut_quality.json", "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

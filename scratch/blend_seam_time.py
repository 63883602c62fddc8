"""Times the multiband blend along optimised seams (csrc/blend_seam.hip) at the default parameters next to the plain multiband blend on the
same frames and transforms in the same process, and writes a JSON record (profiles/blend_seam_time.json).

    python scratch/blend_seam_time.py [OUT.json] [--quick] [--c5]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout).  --c5: also 2000 frames on the block layout (72 GB of frames).  Per survey:
the wall time of the whole mi355_mosaic_blended_seam_dev and mi355_mosaic_blended_dev calls (one warm-up call, then 5 timed ones of each,
alternating, the profile brackets off) and their ratio; then, brackets on, the kernel time per call of the classes "warp" (validity masks and
chip pixels), "distmap" (the maxima and the owned boxes), "blend_seam_candidates", "seam_labels" and "owner" of either call; the label
stage's report.  --quick: 60 frames."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout, block_layout, affine3  # noqa: E402

W, H = 4000, 3000
CLASSES = ("warp", "distmap", "blend_seam_candidates", "seam_labels", "owner")


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def survey(ctx, A, gains, seed, label, rec, reps=5):
    F = len(A)
    note(label, "frames", F)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], seed, k, float(gains[k]), 2.0)
    ctx.synchronize()
    h9s = np.stack([np.linalg.inv(affine3(A[0])) @ affine3(a) for a in A]).reshape(F, 9).astype(np.float32)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    keep = im.resample_by_overlap(wv, hv, h9s, 0.7)
    cw, ch, cws = im.blend_layout(wv, hv, h9s, keep)
    p = im.seamcut_params()
    gw, gh = im.blend_seam_grid(wv, hv, h9s, p.level, keep)
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    cells = torch.empty((gh * gw,), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()

    def seam():
        ctx.MosaicBlendedSeamDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, keep=keep, band=5, params=p)

    def plain():
        out, _, _, _ = ctx.MosaicBlendedDev(ptrs, wv, hv, wsv, h9s, keep=keep, band=5)      # (a canvas of its own from torch's cached blocks)
        del out

    r = {"frames": F, "kept": int(np.asarray(keep).sum()), "frame": "%dx%d" % (W, H), "canvas": "%dx%d" % (cw, ch), "grid": "%dx%d" % (gw, gh),
         "params": {k: getattr(p, k) for k in ("ramp", "level", "depth", "data_weight", "diff_weight", "seam_penalty", "miss_cost")}}
    seam(); plain()                                                         # warm-up: every ctx buffer is sized
    ts, tp = [], []
    for _ in range(reps):
        for call, t in ((seam, ts), (plain, tp)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    r["blended_seam_call_ms"], r["blended_call_ms"] = ts, tp
    r["blended_seam_call_ms_median"], r["blended_call_ms_median"] = float(np.median(ts)), float(np.median(tp))
    r["seam_over_plain"] = r["blended_seam_call_ms_median"] / r["blended_call_ms_median"]
    for name, call in (("blended_seam", seam), ("blended", plain)):
        ctx.profile_enable(True)
        call()
        ctx.profile_reset()
        for _ in range(3):
            call()
        ctx.synchronize()
        r[name + "_kernel_ms"] = {c: ctx.profile_get(c)[0] / 3 for c in CLASSES}
        ctx.profile_enable(False)
    r["report"] = ctx.BlendSeamCellsDev(ptrs, wv, hv, wsv, h9s, cells.data_ptr(), gw, gh, keep=keep, params=p)
    r["cells_moved_fraction"] = r["report"]["changed"] / float(gw * gh)
    note(label, json.dumps(r))
    rec[label] = r
    del frames, canvas, cells
    torch.cuda.empty_cache()


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    ctx = im.Context(0)
    rec = {}
    F = 60 if quick else 500
    A, gains = frame_layout(F, W, H)
    survey(ctx, A, gains, 0xC0FFEE, "c3", rec)
    if out:                                                                 # (kept even if the larger survey does not fit)
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    if "--c5" in sys.argv:
        A5 = block_layout(2000, W, H)
        survey(ctx, A5, 1 + np.random.default_rng(8).uniform(-0.05, 0.05, 2000), 0xC5C5C5, "c5_block_2000", rec)
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

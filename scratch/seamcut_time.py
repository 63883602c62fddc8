"""Times the three stages of the optimised seamlines (csrc/seamcut.hip) at the default parameters next to the seamline render and the depth-4
median render on the same frames and transforms in the same process, and writes a JSON record (profiles/seamcut_time.json).

    python scratch/seamcut_time.py [OUT.json] [--quick] [--c5]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout).  --c5: also 2000 frames on the block layout (72 GB of frames).  Per survey:
kernel time from the library's profile brackets (classes "seam_candidates", "seam_labels", "seamcut", "seamline" and "median"; one warm-up
call, then 5 timed ones), the wall time of the calls, the label stage's report, and the ratios DESIGN 5 states its expectation in.
--quick: 60 frames."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout, block_layout, affine3  # noqa: E402

W, H = 4000, 3000


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
    cw, ch, cws, _ = im.mosaic_layout(wv, hv, h9s)
    p = im.seamcut_params()
    gw, gh = im.seam_grid(wv, hv, h9s, p.level)
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    cand = torch.empty((gh * gw * 32,), dtype=torch.uint8, device="cuda")
    cells = torch.empty((gh * gw,), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()

    def timed(call, cls):
        ctx.profile_enable(True)
        call()                                                              # warm-up
        ctx.profile_reset()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        ms, n, _ = ctx.profile_get(cls)
        ctx.profile_enable(False)
        return ms / reps, float(np.median(t))                               # kernel time per call (all launches of the class), wall

    r = {"frames": F, "frame": "%dx%d" % (W, H), "canvas": "%dx%d" % (cw, ch), "grid": "%dx%d" % (gw, gh),
         "params": {k: getattr(p, k) for k in ("ramp", "level", "depth", "data_weight", "diff_weight", "seam_penalty", "miss_cost")}}
    sk, r["seamline_call_ms_median"] = timed(lambda: ctx.MosaicSeamlineDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "seamline")
    mk, r["median_depth4_call_ms_median"] = timed(lambda: ctx.MosaicMedianDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, depth=4), "median")
    ck, r["candidates_call_ms_median"] = timed(lambda: ctx.SeamCandidatesDev(ptrs, wv, hv, wsv, h9s, cand.data_ptr(), gw, gh, params=p), "seam_candidates")
    report = [None]

    def labels():
        report[0] = ctx.SeamLabelsDev(cand.data_ptr(), gw, gh, cells.data_ptr(), params=p)
    lk, r["labels_call_ms_median"] = timed(labels, "seam_labels")
    rk, r["render_call_ms_median"] = timed(
        lambda: ctx.MosaicSeamCutDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, d_cells=cells.data_ptr(), params=p), "seamcut")
    r["seamline_kernel_ms"], r["median_depth4_kernel_ms"] = sk, mk
    r["candidates_kernel_ms"], r["labels_kernel_ms"], r["render_kernel_ms"] = ck, lk, rk
    r["report"] = report[0]
    r["cells_moved_fraction"] = report[0]["changed"] / float(gw * gh)
    r["candidates_over_median4"], r["labels_over_median4"], r["render_over_seamline"] = ck / mk, lk / mk, rk / sk
    note(label, json.dumps(r))
    rec[label] = r
    del frames, canvas, cand, cells
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

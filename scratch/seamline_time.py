"""Times the seamline render (csrc/seamline.hip) next to the unblended and the weighted (feather) render on the same frames and transforms in
the same process, and writes a JSON record (profiles/seamline_time.json).

    python scratch/seamline_time.py [OUT.json] [--quick] [--c5]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout).  --c5: also 2000 frames on the block layout (72 GB of frames).  Per survey:
kernel time of the three renders from the library's profile brackets (classes "warp", "feather" and "seamline"; one warm-up call, then 5
timed ones), the wall time of the calls, the seamline render with both maps and as maps alone, the ownership pass a withheld frame costs
(mi355_mosaic_seamline_cover), the number of frames that own a pixel, and the mean number of contributing frames per covered canvas pixel
taken from the render's own count map.  --quick: 60 frames (the rocprofv3 run)."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout, block_layout, affine3  # noqa: E402

W, H = 4000, 3000


def survey(ctx, A, gains, seed, label, rec, reps=5):
    F = len(A)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], seed, k, float(gains[k]), 2.0)
    ctx.synchronize()
    h9s = np.stack([np.linalg.inv(affine3(A[0])) @ affine3(a) for a in A]).reshape(F, 9).astype(np.float32)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    cw, ch, cws, _ = im.mosaic_layout(wv, hv, h9s)
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    owner = torch.empty((ch, cw), dtype=torch.int16, device="cuda")
    count = torch.empty((ch, cw), dtype=torch.int16, device="cuda")
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
        return ms / reps, float(np.median(t)), n / reps                     # kernel time per call (all launches of the class), wall, launches per call

    uk, uc, _ = timed(lambda: ctx.MosaicImagesRefinedDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "warp")
    fk, fc, _ = timed(lambda: ctx.MosaicFeatheredDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "feather")
    sk, sc, _ = timed(lambda: ctx.MosaicSeamlineDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "seamline")
    mk, mc, _ = timed(lambda: ctx.MosaicSeamlineDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, d_owner=owner.data_ptr(),
                                                    d_count=count.data_ptr()), "seamline")
    ok, oc, _ = timed(lambda: ctx.MosaicSeamlineDev(None, wv, hv, None, h9s, 0, cw, ch, cws, d_owner=owner.data_ptr(), d_count=count.data_ptr()), "seamline")
    need = [None]

    def cover():
        need[0] = ctx.SeamlineCover(wv, hv, h9s)
    ck, cc, _ = timed(cover, "seamline")
    held = [p if need[0][k] else 0 for k, p in enumerate(ptrs)]
    hk, hc, hl = timed(lambda: ctx.MosaicSeamlineDev(held, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "seamline")
    covered = int((count != 0).sum().item())
    layers = float(count.to(torch.int64).sum().item()) / covered
    rec[label] = {"frames": F, "frame": "%dx%d" % (W, H), "canvas": "%dx%d" % (cw, ch), "covered_pixels": covered,
                  "mean_contributing_frames_per_covered_pixel": layers, "max_contributing_frames": int(count.max().item()),
                  "frames_that_own_a_pixel": int(need[0].sum()),
                  "unblended_kernel_ms": uk, "unblended_call_ms_median": uc, "feather_kernel_ms": fk, "feather_call_ms_median": fc,
                  "seamline_kernel_ms": sk, "seamline_call_ms_median": sc,
                  "seamline_with_maps_kernel_ms": mk, "seamline_with_maps_call_ms_median": mc,
                  "seamline_maps_only_kernel_ms": ok, "seamline_maps_only_call_ms_median": oc,
                  "seamline_cover_kernel_ms": ck, "seamline_cover_call_ms_median": cc,
                  "seamline_withheld_kernel_ms": hk, "seamline_withheld_call_ms_median": hc, "seamline_withheld_launches_per_call": hl,
                  "seamline_over_unblended": sk / uk, "seamline_over_feather": sk / fk, "seamline_below_feather": bool(sk < fk)}
    del frames, canvas, owner, count
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
        survey(ctx, A5, 1 + np.random.default_rng(8).uniform(-0.05, 0.05, 2000), 0xC5C5C5, "c5_block_2000", rec, reps=5)
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""Times the weighted (feather) render (csrc/feather.hip) next to the unblended render on the same frames and transforms, and writes a JSON
record (profiles/feather_time.json).

    python scratch/feather_time.py [OUT.json] [--quick] [--c5]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout).  --c5: also 2000 frames on the block layout (72 GB of frames).  Per survey:
kernel time of both renders from the library's profile brackets (classes "warp" and "feather"; one warm-up call, then 5 timed ones), the
wall time of the calls, and the mean number of contributing frames per covered canvas pixel, counted outside the render: the frames' cover
counts on the step-8 lattice (mi355_gain_stats_dev) over the covered lattice points of an unblended canvas of all-255 frames.
--quick: 60 frames (the rocprofv3 run)."""
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
    torch.cuda.synchronize()
    # contributing frames per covered pixel, on the step-8 lattice
    white = torch.full((H * ws,), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.MosaicImagesRefinedDev([white.data_ptr()] * F, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws)
    covered = int((canvas[::8, 0:3 * cw:24] != 0).sum().item())
    _, cover = ctx.GainStatsDev(ptrs, wv, hv, wsv, h9s, [], 8)
    layers = float(cover.sum()) / covered
    del white

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
        return ms / max(n, 1), float(np.median(t))

    uk, uc = timed(lambda: ctx.MosaicImagesRefinedDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "warp")
    fk, fc = timed(lambda: ctx.MosaicFeatheredDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "feather")
    rec[label] = {"frames": F, "frame": "%dx%d" % (W, H), "canvas": "%dx%d" % (cw, ch), "covered_lattice_points": covered,
                  "mean_contributing_frames_per_covered_pixel": layers,
                  "unblended_kernel_ms": uk, "unblended_call_ms_median": uc, "feather_kernel_ms": fk, "feather_call_ms_median": fc,
                  "feather_over_unblended": fk / uk, "bar_1.5_x_layers": 1.5 * layers, "within_bar": bool(fk <= 1.5 * layers * uk)}
    del frames, canvas
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
        survey(ctx, A5, 1 + np.random.default_rng(8).uniform(-0.05, 0.05, 2000), 0xC5C5C5, "c5_block_2000", rec, reps=3)
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

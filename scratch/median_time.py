"""Times the median render (csrc/median.hip) at depth 1, 5 and 9 next to the unblended, the weighted (feather) and the seamline render on the
same frames and transforms in the same process, and writes a JSON record (profiles/median_time.json).

    python scratch/median_time.py [OUT.json] [--quick] [--c5] [--parity]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout).  --c5: also 2000 frames on the block layout (72 GB of frames).  Per survey:
kernel time of the renders from the library's profile brackets (classes "warp", "feather", "seamline" and "median"; one warm-up call, then 5
timed ones), the wall time of the calls, the median render at depth 5 with both maps, as the count map alone and as the cover call, the number
of frames some pixel selects at depth 5, and the mean number of contributing frames per covered canvas pixel from the render's own count map.
--quick: 60 frames.  --parity: one 256 x 256 window of the C3 canvas at depth 5 against tests/median_ref.py (window_ref, on the oracle)."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout, block_layout, affine3  # noqa: E402

W, H = 4000, 3000
DEPTHS = (1, 5, 9)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def survey(ctx, A, gains, seed, label, rec, reps=5, parity=False):
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
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    spread = torch.empty((ch, cw), dtype=torch.uint8, device="cuda")
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

    r = {"frames": F, "frame": "%dx%d" % (W, H), "canvas": "%dx%d" % (cw, ch)}
    uk, r["unblended_call_ms_median"], _ = timed(lambda: ctx.MosaicImagesRefinedDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "warp")
    fk, r["feather_call_ms_median"], _ = timed(lambda: ctx.MosaicFeatheredDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "feather")
    sk, r["seamline_call_ms_median"], _ = timed(lambda: ctx.MosaicSeamlineDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "seamline")
    r["unblended_kernel_ms"], r["feather_kernel_ms"], r["seamline_kernel_ms"] = uk, fk, sk
    note(label, "unblended / feather / seamline kernel ms", uk, fk, sk)
    mk = {}
    for d in DEPTHS:
        mk[d], r["median_depth%d_call_ms_median" % d], _ = timed(
            lambda: ctx.MosaicMedianDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, depth=d), "median")
        r["median_depth%d_kernel_ms" % d] = mk[d]
        note(label, "median depth", d, "kernel ms", mk[d])
    r["median_depth5_with_maps_kernel_ms"], r["median_depth5_with_maps_call_ms_median"], _ = timed(
        lambda: ctx.MosaicMedianDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, d_spread=spread.data_ptr(), d_count=count.data_ptr(), depth=5), "median")
    r["median_depth5_count_only_kernel_ms"], r["median_depth5_count_only_call_ms_median"], _ = timed(
        lambda: ctx.MosaicMedianDev(None, wv, hv, None, h9s, 0, cw, ch, cws, d_count=count.data_ptr(), depth=5), "median")
    r["median_depth9_count_only_kernel_ms"], _, _ = timed(
        lambda: ctx.MosaicMedianDev(None, wv, hv, None, h9s, 0, cw, ch, cws, d_count=count.data_ptr(), depth=9), "median")
    need = [None]

    def cover():
        need[0] = ctx.MedianCover(wv, hv, h9s, depth=5)
    r["median_depth5_cover_kernel_ms"], r["median_depth5_cover_call_ms_median"], _ = timed(cover, "median")
    covered = int((count != 0).sum().item())
    r["covered_pixels"] = covered
    r["mean_contributing_frames_per_covered_pixel"] = float(count.to(torch.int64).sum().item()) / covered
    r["max_contributing_frames"] = int(count.max().item())
    r["frames_selected_somewhere_depth5"] = int(need[0].sum())
    r["pixels_with_nonzero_spread_depth5"] = int((spread != 0).sum().item())
    r["median5_over_seamline"], r["median5_over_feather"] = mk[5] / sk, mk[5] / fk
    r["median5_between_seamline_and_feather"] = bool(sk <= mk[5] <= fk)
    if parity:
        from tests import median_ref as mr
        from tests import oracle_lib as ol
        from tests.synth_survey import host_image
        orc = ol.load_oracle_fast()
        S = 256
        note(label, "parity window")
        rng = np.random.default_rng(31)
        x0, y0 = int(rng.integers(0, cw - S)), int(rng.integers(0, ch - S))
        ref, rspr, rcnt, nsub = mr.window_ref(orc, lambda k: host_image(frames, k, W, H, ws), W, H, h9s, (x0, y0, S, S), 0, 5, threads=8)
        got = canvas[y0:y0 + S, 3 * x0:3 * (x0 + S)].cpu().numpy().reshape(S, S, 3)
        r["parity_window"] = {"x0": x0, "y0": y0, "size": S, "frames_rendered": nsub, "max_frames_per_pixel": int(rcnt.max()),
                              "bytes_differ": int((got != ref).sum()), "spread_differ": int((spread[y0:y0 + S, x0:x0 + S].cpu().numpy() != rspr).sum()),
                              "count_differ": int((count[y0:y0 + S, x0:x0 + S].cpu().numpy().view(np.uint16) != rcnt).sum())}
    rec[label] = r
    del frames, canvas, spread, count
    torch.cuda.empty_cache()


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    ctx = im.Context(0)
    rec = {}
    F = 60 if quick else 500
    A, gains = frame_layout(F, W, H)
    survey(ctx, A, gains, 0xC0FFEE, "c3", rec, parity="--parity" in sys.argv)
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

"""Times the overview pass (csrc/overview.hip) and the striped preview (mi355_mosaic_preview_into) next to the full-size renders on the same
frames in the same process, and writes a JSON record (profiles/overview_time.json).

    python scratch/overview_time.py [OUT.json] [--quick] [--c5]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout).  --c5: also 2000 frames on the block layout (72 GB of frames).  Per survey:
(a) kernel time of mi355_mosaic_overview_dev at levels = 7 on the seamline canvas, with the count map (NODATA_MAP, covers written) and without
    (NODATA_ZERO, no covers), from the library's profile class "overview" (one warm-up call, then 5 timed ones), next to the kernel time of the
    unblended render of the same canvas (class "warp");
(b) the achieved bytes per second from the class's algorithmic bytes (level 0 read once, every level written once) as a fraction of the
    6.3 TB/s a streaming kernel reaches on this part;
(c) wall time of MosaicPreviewInto at level 3 for each render next to the wall time of the matching full-size _into call, both from the same host
    images (both therefore pay the same upload of the frames; the upload alone is timed too).  On the 2000-frame survey (c) is left out: the calls
    take host images or kept frames, and 72 GB of host frames are not built here.
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
HBM_ACHIEVABLE = 6.3e12


def survey(ctx, A, gains, seed, label, rec, reps=5, previews=True):
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
    count = torch.empty((ch, cw), dtype=torch.int16, device="cuda")
    geo = im.overview_layout(cw, ch, 7)
    lv = [torch.empty((oh, ows), dtype=torch.uint8, device="cuda") for ow, oh, ows in geo]
    cv = [torch.empty((oh, ow), dtype=torch.int16, device="cuda") for ow, oh, ows in geo]
    torch.cuda.synchronize()

    def timed(call, cls):
        ctx.profile_enable(True)
        call(); ctx.synchronize()                                           # warm-up
        ctx.profile_reset()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        ms, n, nbytes = ctx.profile_get(cls)
        ctx.profile_enable(False)
        return ms / reps, float(np.median(t)), nbytes / reps

    uk, _, _ = timed(lambda: ctx.MosaicImagesRefinedDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws), "warp")
    sk, _, _ = timed(lambda: ctx.MosaicSeamlineDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, d_count=count.data_ptr()), "seamline")
    lvp, cvp = [t.data_ptr() for t in lv], [t.data_ptr() for t in cv]
    mk, mc, mb = timed(lambda: ctx.MosaicOverviewDev(canvas.data_ptr(), cw, ch, cws, 7, lvp, cvp, d_valid_rows=count.data_ptr(), nodata=2), "overview")
    zk, zc, zb = timed(lambda: ctx.MosaicOverviewDev(canvas.data_ptr(), cw, ch, cws, 7, lvp, None, nodata=1), "overview")
    r = {"frames": F, "frame": "%dx%d" % (W, H), "canvas": "%dx%d" % (cw, ch), "canvas_bytes": int(ch) * int(cws),
         "unblended_kernel_ms": uk, "seamline_with_count_kernel_ms": sk,
         "overview7_with_map_kernel_ms": mk, "overview7_with_map_call_ms_median": mc, "overview7_with_map_bytes": mb,
         "overview7_with_map_TBps": mb / (mk * 1e-3) / 1e12, "overview7_with_map_fraction_of_achievable_hbm": mb / (mk * 1e-3) / HBM_ACHIEVABLE,
         "overview7_no_map_kernel_ms": zk, "overview7_no_map_call_ms_median": zc, "overview7_no_map_bytes": zb,
         "overview7_no_map_TBps": zb / (zk * 1e-3) / 1e12, "overview7_no_map_fraction_of_achievable_hbm": zb / (zk * 1e-3) / HBM_ACHIEVABLE,
         "achievable_hbm_TBps": HBM_ACHIEVABLE / 1e12, "overview_below_unblended_render": bool(mk < uk and zk < uk)}
    del lv, cv, canvas, count
    if previews:
        host = frames.cpu().numpy()
        del frames
        torch.cuda.empty_cache()
        imgs = [host[k].reshape(H, W, 3) for k in range(F)]
        full = np.zeros((ch, cws), np.uint8)
        calls = {0: lambda: ctx.MosaicImagesRefinedInto(imgs, None, h9s, out=full), 1: lambda: ctx.MosaicFeatheredInto(imgs, None, h9s, out=full),
                 2: lambda: ctx.MosaicSeamlineInto(imgs, None, h9s, out=full)}
        up = torch.empty_like(torch.from_numpy(host[0])).cuda()
        t0 = time.perf_counter()
        for k in range(F):
            up.copy_(torch.from_numpy(host[k]))
        torch.cuda.synchronize()
        r["host_frames_upload_ms"] = (time.perf_counter() - t0) * 1e3
        for render, name in ((0, "refined"), (1, "feathered"), (2, "seamline")):
            w = []
            for fn in (calls[render], lambda: ctx.MosaicPreviewInto(imgs, None, h9s, render=render, level=3, nodata=2)):
                fn()                                                        # warm-up: buffers are grown
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    fn()
                    t.append((time.perf_counter() - t0) * 1e3)
                w.append(float(np.median(t)))
            r["%s_into_wall_ms" % name], r["%s_preview3_wall_ms" % name] = w
            r["%s_preview3_below_full_into" % name] = bool(w[1] < w[0])
    else:
        del frames
        r["previews"] = "left out: the preview and _into calls take host images or kept frames"
    rec[label] = r
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
        survey(ctx, A5, 1 + np.random.default_rng(8).uniform(-0.05, 0.05, 2000), 0xC5C5C5, "c5_block_2000", rec, previews=False)
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

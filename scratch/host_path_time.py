"""Times the host caller's sequence (frames in pageable host memory, as the reference's IplImages are) with today's entry
points and with kept frames + a render into a preallocated numpy canvas, in the same run.  The sample is bench.py's `host_frames`: 96
synthetic frames of 4000x3000, pair window 182, second pass of two.  Per phase: extract (host frames handed over, features resolved),
match, align (host), render (+ download).  The render and download of the _into path are split by rendering the same canvas once more
through mi355_mosaic_refined_dev from the kept frames (render only).  Also compares the download variants of mi355_mosaic_refined_into.

    python scratch/host_path_time.py [--frames 96] [--out profiles/host_path_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--window", type=int, default=182)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    n, w, h = a.frames, 4000, 3000
    ctx = im.Context(0)
    fr, _, _, ws = render_frames(ctx, torch, n, w, h)
    imgs = [np.ascontiguousarray(fr[k].cpu().numpy().reshape(h, ws)[:, :3 * w]).reshape(h, w, 3) for k in range(n)]
    del fr
    torch.cuda.empty_cache()
    pairs = im.pair_schedule(n, a.window)
    canvas = {}

    def align(res):
        lab = im.select_connected_results(res, n) if len(res) else np.zeros(n, np.int32)
        lab[0] = 1
        T = im.global_affine_align_results(res, n, fixed=[1 if (k == 0 or lab[k] == 0) else 0 for k in range(n)], label=lab)
        hh = T["m"].copy()
        hh[lab == 0, 8] = 0.0
        return hh

    def one_pass(seed, keep):
        t = {}
        t0 = time.perf_counter()
        for k in range(n):
            ctx.SiftExtractHost(k, imgs[k])
        ctx.synchronize()
        t1 = time.perf_counter(); t["extract"] = t1 - t0
        res = ctx.MatchPairs(pairs, 2.5, seed)
        t2 = time.perf_counter(); t["match"] = t2 - t1
        hh = align(res)
        t3 = time.perf_counter(); t["align"] = t3 - t2
        if keep:
            cw, ch, cws, _ = im.mosaic_layout([w] * n, [h] * n, hh)
            if "out" not in canvas or canvas["out"].shape != (ch, cws):
                canvas["out"] = np.empty((ch, cws), np.uint8)
                canvas["out"].fill(0)                                 # first touch outside the timed pass (a caller's preallocated canvas)
            ctx.MosaicImagesRefinedInto(None, np.arange(n, dtype=np.int32), hh, out=canvas["out"], geom=[(w, h, 3 * w)] * n)
        else:
            _, cw, ch, _ = ctx.MosaicImagesRefined(imgs, hh, want_pixels=False)
        t4 = time.perf_counter(); t["render+download"] = t4 - t3
        t["total"] = t4 - t0
        return t, hh, (cw, ch), int(res["accepted"].sum())

    out = {"frames": n, "size": [w, h], "window": a.window, "pairs": len(pairs)}
    for label, keep in (("today", 0), ("kept_into", 1)):
        ctx.DropFeatures(-1)
        ctx.DropFrames(-1)
        ctx.set_option("keep_frames", keep)
        one_pass(1, keep)
        t, hh, cwh, acc = one_pass(2, keep)
        t = {k: round(v * 1e3, 1) for k, v in t.items()}
        out[label] = {"ms": t, "frames_per_s": round(n / (t["total"] / 1e3), 1), "pairs_per_s": round(len(pairs) / (t["total"] / 1e3), 1),
                      "canvas": list(cwh), "accepted": acc}
        if keep:
            # render alone: the same canvas from the kept frames into HBM, no download
            cw, ch, cws, _ = im.mosaic_layout([w] * n, [h] * n, hh)
            dc = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            fd = [ctx.FrameDev(k) for k in range(n)]
            for rep in range(2):
                t0 = time.perf_counter()
                ctx.MosaicImagesRefinedDev([x[0] for x in fd], [w] * n, [h] * n, [3 * w] * n, hh, dc.data_ptr(), cw, ch, cws)
                ctx.synchronize()
                r_ms = (time.perf_counter() - t0) * 1e3
            out[label]["render_only_ms"] = round(r_ms, 1)
            out[label]["download_ms_est"] = round(t["render+download"] - r_ms, 1)
            del dc
            torch.cuda.empty_cache()
            # download variants of the same call (same bytes; checked against the default)
            ref = canvas["out"].copy()
            var = {}
            for name, opts in (("pinned_x1", {"download_mode": 0, "download_threads": 1}), ("pinned_x4", {"download_mode": 0, "download_threads": 4}),
                               ("pinned_x8", {"download_mode": 0, "download_threads": 8}), ("pinned_x16", {"download_mode": 0, "download_threads": 16}),
                               ("memcpy2d_pageable", {"download_mode": 1}), ("host_register", {"download_mode": 2})):
                for k, v in opts.items():
                    ctx.set_option(k, v)
                best = None
                for rep in range(2):
                    t0 = time.perf_counter()
                    ctx.MosaicImagesRefinedInto(None, np.arange(n, dtype=np.int32), hh, out=canvas["out"], geom=[(w, h, 3 * w)] * n)
                    dt = (time.perf_counter() - t0) * 1e3
                    best = dt if best is None else min(best, dt)
                var[name] = {"render+download_ms": round(best, 1), "download_ms_est": round(best - r_ms, 1),
                             "GB_per_s_est": round(ch * 3 * cw / max(best - r_ms, 1e-3) / 1e6, 2), "same_bytes": bool(np.array_equal(ref, canvas["out"]))}
            ctx.set_option("download_mode", 0)
            ctx.set_option("download_threads", 4)
            out[label]["download_variants"] = var
    out["speedup"] = round(out["today"]["ms"]["total"] / out["kept_into"]["ms"]["total"], 3)
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(s)


if __name__ == "__main__":
    main()

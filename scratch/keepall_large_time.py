"""Keep-all SIFT (nfeatures = 0) on the 4000x3000 survey frames and on the reference's 1000x750 frames, on one MI355X: the keypoint counts
(mi355_last_sift_counters), the per-frame times of the keep-all stages (event brackets: kp_select, orient, topk = the tile-sort ordering, describe), the describe
grid's empty workgroups (the same
2 900-keypoint frame under keepall_max 32768 and 262144) and one 80 000-class pair through the matcher ("match", "select" brackets).

    python scratch/keepall_large_time.py [--frames 4] [--reps 3] [--out profiles/keepall_large_time.json]

Run it under `rocprofv3 --kernel-trace --stats` for the kernel-level view: the 2 900-keypoint frames run with keepall_max = 32768, the
survey frames with 262144, so the two sizes are told apart by the ordering kernels' grid.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ["gauss", "gauss_stream", "downsample", "extrema", "refine", "kp_select", "orient", "topk", "describe", "features"]


def keepall_ctx(im, kmax):
    p = im.default_params()
    p.nfeatures = 0
    ctx = im.Context(0, p)
    if kmax != 32768:
        ctx.set_option("keepall_max", kmax)
    return ctx


def stage_times(ctx, extract, n_frames, reps):
    """ms per frame of every bracketed class, median over reps of one batch of n_frames"""
    extract()                                         # warm-up (work areas)
    ctx.synchronize()
    per = {c: [] for c in CLASSES}
    wall = []
    for _ in range(reps):
        ctx.profile_enable(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        extract()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / n_frames)
        for c in CLASSES:
            ms, n, _ = ctx.profile_get(c)
            per[c].append(ms / n_frames)
        ctx.profile_enable(False)
    out = {c: float(np.median(v)) for c, v in per.items() if max(v) > 0}
    out["wall_ms_per_frame"] = float(np.median(wall))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    from PIL import Image
    out = {"device": torch.cuda.get_device_name(0)}
    w, h = 4000, 3000
    # 1. one survey frame on a default keep-all ctx (ceiling 32768): what trips
    ctx = keepall_ctx(im, 32768)
    fr, _, _, ws = render_frames(ctx, torch, a.frames, w, h)
    try:
        ctx.SiftExtractDev(0, fr[0].data_ptr(), w, h, ws, want_count=True)
        out["default_ctx"] = {"error": None}
    except im.Mi355Error as e:
        out["default_ctx"] = {"error": str(e)}
    out["default_ctx"]["counters"] = ctx.last_sift_counters()
    ctx.close()
    # 2. the survey frames under the largest ceiling: counts, stage times
    ctx = keepall_ctx(im, 262144)
    counts = []
    for k in range(a.frames):
        ctx.SiftExtractDev(k, fr[k].data_ptr(), w, h, ws, want_count=True)
        counts.append(ctx.last_sift_counters())
    out["survey_counters"] = counts
    out["survey_keypoints"] = [c[3] for c in counts]

    def survey():
        for k in range(a.frames):
            ctx.SiftExtractDev(k, fr[k].data_ptr(), w, h, ws)
        ctx.set_option("sift_flush", 1)

    out["survey_stage_ms_sort"] = stage_times(ctx, survey, a.frames, a.reps)
    # 3. one 80 000-class pair (two overlapping survey frames) through the matcher
    ctx.MatchPairs([(0, 1)], 2.5, 3)                  # warm-up
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    r = ctx.MatchPairs([(0, 1)], 2.5, 3)[0]
    wall = (time.perf_counter() - t0) * 1e3
    out["pair_80k"] = {"n_kp": [out["survey_keypoints"][0], out["survey_keypoints"][1]], "wall_ms": wall,
                       "match_ms": ctx.profile_get("match")[0], "select_big_ms": ctx.profile_get("select")[0],
                       "n_selected": int(r["n_selected"]), "n_in": int(r["n_in"]), "accepted": int(r["accepted"])}
    ctx.profile_enable(False)
    ctx.close()
    del fr
    torch.cuda.empty_cache()
    # 4. the reference's frames (about 2 900 keypoints): the describe grid at two ceilings
    gold = os.path.join(ROOT, "tests", "golden")
    names = ["DSC%05d.JPG" % k for k in range(4, 4 + a.frames)]
    imgs = [np.ascontiguousarray(np.array(Image.open(os.path.join(gold, n)).convert("RGB"))[:, :, ::-1]) for n in names]
    dev = [torch.from_numpy(x.copy()).cuda() for x in imgs]
    for kmax in (32768, 262144):
        ctx = keepall_ctx(im, kmax)

        def ref():
            for k, d in enumerate(dev):
                ctx.SiftExtractDev(k, d.data_ptr(), d.shape[1], d.shape[0], d.stride(0))
            ctx.set_option("sift_flush", 1)

        out[f"reference_stage_ms_sort_keepall_max_{kmax}"] = stage_times(ctx, ref, a.frames, a.reps)
        out.setdefault("reference_keypoints", [len(ctx.GetFeatures(k, max_kp=kmax)[0]) for k in range(a.frames)])
        ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)), exist_ok=True)
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""Times the cover-depth statistics (csrc/cover.hip) next to the gain statistics in the same run, and the coverage-checked selection, at survey
size, and writes a JSON record (profiles/cover_time.json).

    python scratch/cover_time.py [OUT.json] [--quick]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout), step 8: cover_depth_kernel next to gain_stats_kernel on the 499 adjacent
pairs (kernel times from the library's profile brackets, call times the wall time of the call; the two stages alternate, medians of 5), then
CoverSelectDev with order=None and no pair list at min_depth 1 and 2: rounds, frames dropped, wall time.  The selection again on the 2000-frame
block survey the seamline timing uses (geometry only: no frames are made for it).  --quick: 60 and 200 frames."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout, block_layout, affine3  # noqa: E402

REPS = 5


def stage(ctx, call, scope):
    ctx.profile_reset()
    t0 = time.perf_counter()
    res = call()
    wall = (time.perf_counter() - t0) * 1e3
    ms, n, _b = ctx.profile_get(scope)
    return res, wall, ms / max(n, 1)


def selection(ctx, wv, hv, h9s, rec):
    cw, ch, _, _ = im.mosaic_layout(wv, hv, h9s)
    rec["canvas"] = "%dx%d" % (cw, ch)
    for depth in (1, 2):
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            status, keep_out, rounds, lost, fs, hist = ctx.CoverSelectDev(wv, hv, h9s, step=8, min_depth=depth, final=True)
            ts.append((time.perf_counter() - t0) * 1e3)
        print("select min_depth %d: %d rounds, %.0f ms" % (depth, rounds, float(np.median(ts))), file=sys.stderr, flush=True)
        rec["select_min_depth_%d" % depth] = {"rounds": rounds, "dropped": int((status == im.COVER_DROPPED).sum()), "kept_for_coverage": int((status == im.COVER_KEPT_COVERAGE).sum()),
                                              "lost": lost, "wall_ms_median": float(np.median(ts)), "wall_ms": ts, "ms_per_round": float(np.median(ts)) / max(rounds, 1),
                                              "hist_after": hist.tolist()}


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    W, H = 4000, 3000
    F = 60 if quick else 500
    ctx = im.Context(0)
    A, gains = frame_layout(F, W, H)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
    ctx.synchronize()
    h9s = np.stack([affine3(a).reshape(9) for a in A]).astype(np.float32)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    pairs = [(k, k + 1) for k in range(F - 1)]
    calls = {"gain": (lambda: ctx.GainStatsDev(ptrs, wv, hv, wsv, h9s, pairs, 8), "gain_stats"),
             "cover": (lambda: ctx.CoverStatsDev(wv, hv, h9s, None, 8), "cover_depth")}
    wall = {k: [] for k in calls}
    kern = {k: [] for k in calls}
    res = {}
    ctx.profile_enable(True)
    for k in calls:
        calls[k][0]()                                                       # warm-up
    for _ in range(REPS):
        for k in calls:                                                     # alternating
            res[k], w_ms, k_ms = stage(ctx, *calls[k])
            wall[k].append(w_ms)
            kern[k].append(k_ms)
    ctx.profile_enable(False)
    print("statistics timed", file=sys.stderr, flush=True)
    fs, hist = res["cover"]
    assert np.array_equal(fs["at_depth"].sum(axis=1), res["gain"][1])      # the frame_cover identity, at survey size
    c3 = {"frames": F, "frame": "%dx%d" % (W, H), "pairs": len(pairs), "step": 8, "lattice_points": int(hist.sum()), "hist": hist.tolist()}
    for k in calls:
        c3[k] = {"kernel_ms_median": float(np.median(kern[k])), "kernel_ms": kern[k], "call_ms_median": float(np.median(wall[k]))}
    c3["kernel_ratio_cover_over_gain"] = c3["cover"]["kernel_ms_median"] / c3["gain"]["kernel_ms_median"]
    del frames
    selection(ctx, wv, hv, h9s, c3)
    rec = {"c3_strip": c3}
    F5 = 200 if quick else 2000
    A5 = block_layout(F5, W, H)
    h5 = np.stack([affine3(a).reshape(9) for a in A5]).astype(np.float32)
    c5 = {"frames": F5, "frame": "%dx%d" % (W, H), "step": 8}
    ts = []
    ctx.CoverStatsDev([W] * F5, [H] * F5, h5, None, 8)
    for _ in range(REPS):
        t0 = time.perf_counter()
        fs5, hist5 = ctx.CoverStatsDev([W] * F5, [H] * F5, h5, None, 8)
        ts.append((time.perf_counter() - t0) * 1e3)
    c5["cover_call_ms_median"] = float(np.median(ts))
    c5["hist"] = hist5.tolist()
    selection(ctx, [W] * F5, [H] * F5, h5, c5)
    rec["c5_block"] = c5
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

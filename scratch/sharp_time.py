"""Times the frame sharpness statistics (csrc/sharp.hip) next to the gain statistics on the same pairs in the same run, at survey size, and
writes a JSON record (profiles/sharp_time.json).

    python scratch/sharp_time.py [OUT.json] [--quick]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout), the 499 adjacent pairs, step 8.  Kernel times come from the library's
profile brackets, call times are the wall time of the call (host work list and copies included); the two stages alternate.  The host
solve and selection are timed on the same records.  --quick: 60 frames."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout, affine3  # noqa: E402


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
    calls = {"gain": lambda: ctx.GainStatsDev(ptrs, wv, hv, wsv, h9s, pairs, 8),
             "sharp_pairs_only": lambda: ctx.SharpStatsDev(ptrs, wv, hv, wsv, h9s, pairs, 8, frames=False),
             "sharp_with_frames": lambda: ctx.SharpStatsDev(ptrs, wv, hv, wsv, h9s, pairs, 8, frames=True)}
    scope = {"gain": "gain_stats", "sharp_pairs_only": "sharp_stats", "sharp_with_frames": "sharp_stats"}
    wall = {k: [] for k in calls}
    kern = {k: [] for k in calls}
    res = {}
    ctx.profile_enable(True)
    for k in calls:
        calls[k]()                                                          # warm-up
    for _ in range(5):
        for k in calls:                                                     # alternating
            ctx.profile_reset()
            t0 = time.perf_counter()
            res[k] = calls[k]()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ms, n, _b = ctx.profile_get(scope[k])
            kern[k].append(ms / max(n, 1))
    ctx.profile_enable(False)
    gst, gcov = res["gain"]
    st, fs = res["sharp_with_frames"]
    assert res["sharp_pairs_only"][0].tobytes() == st.tobytes()
    rec = {"frames": F, "frame": "%dx%d" % (W, H), "pairs": len(pairs), "step": 8,
           "gain_lattice_points_pairs": int(gst["n"].sum()), "gain_lattice_points_frames": int(gcov.sum()),
           "sharp_lattice_points_pairs": int(st["n"].sum()), "sharp_lattice_points_frames": int(fs["n"].sum())}
    for k in calls:
        rec[k] = {"kernel_ms_median": float(np.median(kern[k])), "kernel_ms": kern[k], "call_ms_median": float(np.median(wall[k]))}
    rec["kernel_ratio_pairs_only_over_gain"] = rec["sharp_pairs_only"]["kernel_ms_median"] / rec["gain"]["kernel_ms_median"]
    rec["kernel_ratio_with_frames_over_gain"] = rec["sharp_with_frames"]["kernel_ms_median"] / rec["gain"]["kernel_ms_median"]
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        status, sharp = im.select_sharp_frames(st, F)
        ts.append((time.perf_counter() - t0) * 1e3)
    rec["solve_select_ms_median"] = float(np.median(ts))
    rec["status_counts"] = [int((status == v).sum()) for v in range(4)]
    rec["sharp_min_max"] = [float(sharp.min()), float(sharp.max())]
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    del frames
    ctx.close()


if __name__ == "__main__":
    main()

"""Times exposure gain compensation (csrc/gain.hip) at survey size and writes a JSON record (profiles/gain_time.json).

    python scratch/gain_time.py [OUT.json] [--quick]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout), the 499 adjacent pairs; C4's pair list: the same survey's window-182
schedule restricted to the pairs whose ground footprints overlap (a geometric stand-in for the accepted pairs).  Stats at step 8 (kernel
time from the library's profile brackets and the wall time of the call, which includes the host work list and the copies), the solve
(host), and the in-place apply over all 500 frames.  Solve at C5's 2000 frames on the block layout's overlap graph (window 182).
--quick: 60 frames (the rocprofv3 run)."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout, block_layout, affine3  # noqa: E402


def footprints_overlap(A, w, h, i, j):
    c = np.array([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], np.float64).T
    pi, pj = affine3(A[i]) @ c, affine3(A[j]) @ c
    return not (pi[0].max() < pj[0].min() or pj[0].max() < pi[0].min() or pi[1].max() < pj[1].min() or pj[1].max() < pi[1].min())


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
    rec = {"frames": F, "frame": "%dx%d" % (W, H)}

    def time_stats(pairs, label, reps=5):
        ctx.profile_enable(True)
        ctx.GainStatsDev(ptrs, wv, hv, wsv, h9s, pairs, 8)                 # warm-up
        ctx.profile_reset()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            st, cover = ctx.GainStatsDev(ptrs, wv, hv, wsv, h9s, pairs, 8)
            t.append((time.perf_counter() - t0) * 1e3)
        ms, n, _ = ctx.profile_get("gain_stats")
        ctx.profile_enable(False)
        samples = int(cover.sum() + 2 * st["n"].sum())
        rec[label] = {"pairs": len(pairs), "pairs_with_overlap": int((st["n"] > 0).sum()), "lattice_points_frames": int(cover.sum()),
                      "lattice_points_pairs": int(st["n"].sum()), "frame_samples": samples,
                      "stats_kernel_ms": ms / max(n, 1), "stats_call_ms_median": float(np.median(t))}
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            g = im.solve_gains(st, cover)
            ts.append((time.perf_counter() - t0) * 1e3)
        rec[label]["solve_ms_median"] = float(np.median(ts))
        return st, cover, g

    adj = [(k, k + 1) for k in range(F - 1)]
    st, cover, g = time_stats(adj, "c3_adjacent")
    rec["c3_adjacent"]["corr_g_inv_gain"] = [float(np.corrcoef(g[:, c], 1.0 / gains)[0, 1]) for c in range(3)]
    c4 = [(i, j) for (i, j) in im.pair_schedule(F, 182) if footprints_overlap(A, W, H, int(i), int(j))]
    time_stats(c4, "c4_overlapping_window182")
    # apply: in place over every frame
    ctx.profile_enable(True)
    ctx.ApplyGainsDev(ptrs, ptrs, wv, hv, wsv, g)
    ctx.profile_reset()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        ctx.ApplyGainsDev(ptrs, ptrs, wv, hv, wsv, g)
        t.append((time.perf_counter() - t0) * 1e3)
    ms, n, b = ctx.profile_get("gain_apply")
    ctx.profile_enable(False)
    kms = ms / max(n, 1)
    rec["apply"] = {"frames": F, "bytes": 2 * 3 * W * H * F, "kernel_ms": kms, "call_ms_median": float(np.median(t)),
                    "TB_per_s": 2 * 3 * W * H * F / (kms * 1e-3) / 1e12, "fraction_of_6.3TBps": 2 * 3 * W * H * F / (kms * 1e-3) / 6.3e12}
    # solve at C5's size: 2000 frames, block layout, window-182 pairs whose footprints overlap; statistics synthetic (the solve's cost
    # depends on the pair graph only)
    N5 = 2000
    A5 = block_layout(N5, W, H)
    pairs5 = [(i, j) for (i, j) in im.pair_schedule(N5, 182) if footprints_overlap(A5, W, H, int(i), int(j))]
    rng = np.random.default_rng(1)
    g5 = rng.uniform(0.9, 1.1, N5)
    st5 = np.zeros(len(pairs5), im.GAIN_PAIR_STATS)
    for q, (i, j) in enumerate(pairs5):
        nn = int(rng.integers(1000, 100000)); base = rng.uniform(60, 180, 3)
        st5[q]["a"], st5[q]["b"], st5[q]["n"] = i, j, nn
        st5[q]["sum_a"] = np.round(base * g5[i] * nn); st5[q]["sum_b"] = np.round(base * g5[j] * nn)
    cov5 = np.full(N5, 187500, np.int64)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        im.solve_gains(st5, cov5)
        ts.append((time.perf_counter() - t0) * 1e3)
    rec["solve_c5_block_2000"] = {"frames": N5, "pairs": len(pairs5), "solve_ms_median": float(np.median(ts))}
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    del frames
    ctx.close()


if __name__ == "__main__":
    main()

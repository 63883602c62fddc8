"""Pair stage of the C4 survey (500 frames of 4000x3000, window 182) with and without the descriptor screen (csrc/screen.hip), one process:

  * the screen in window-182 mode and in all-pairs mode (device-synchronised wall time, and the kernels' own time through the profiling
    brackets);
  * the pair stage (mi355_match_pairs_dev) on the window list and on the screened list, alternating, a device synchronise around each;
  * recall: of the window's accepted pairs, how many the screened list contains, by n_in bins; the candidate fraction;
  * a sweep of top_k x partners x min_score: recall / list size / screen time.

    python scratch/pair_screen_time.py [--frames 500] [--reps 5] [--out profiles/pair_screen_time.json] [--no-sweep]
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
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_screen_time.json"))
    ap.add_argument("--no-sweep", action="store_true")
    a = ap.parse_args()
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    ctx = im.Context(0)
    w, h, n = 4000, 3000, a.frames
    t0 = time.time()
    frames, _, _, ws = render_frames(ctx, torch, n, w, h)
    for k in range(n):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), w, h, ws)
    ctx.synchronize()
    del frames
    torch.cuda.empty_cache()
    print("frames + SIFT: %.1f s" % (time.time() - t0), flush=True)
    ids = np.arange(n, dtype=np.int32)
    win = im.pair_schedule(n, 182)
    seed = 17
    d = im.screen_params(window=182)

    def timed(fn):
        ctx.synchronize(); torch.cuda.synchronize()
        t = time.perf_counter(); r = fn(); ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def kernel_ms(fn):
        ctx.profile_enable(True); ctx.profile_reset()
        fn()
        out = {c: ctx.profile_get(c)[0] for c in ("screen_topk", "screen_pairs", "screen_select")}
        ctx.profile_enable(False)
        return out

    res = {"frames": n, "size": [w, h], "window": 182, "window_pairs": int(len(win)), "defaults": {"top_k": d.top_k, "partners": d.partners, "min_score": d.min_score, "ratio_pct": d.ratio_pct}}
    # screen times (defaults), window mode and all-pairs mode
    for mode, wnd in (("window182", 182), ("all_pairs", 0)):
        walls = []
        for _ in range(a.reps):
            ms, scr = timed(lambda: ctx.ScreenPairs(ids, window=wnd))
            walls.append(ms)
        ks = kernel_ms(lambda: ctx.ScreenPairs(ids, window=wnd))
        cand = len(win) if wnd else n * (n - 1) // 2
        ops = cand * 2.0 * 2.0 * d.top_k * d.top_k * 128
        res["screen_" + mode] = {"candidates": cand, "wall_ms": walls, "wall_ms_median": float(np.median(walls)), "kernel_ms": ks,
                                 "pairs_kernel_pops": ops / (ks["screen_pairs"] * 1e-3) / 1e15 if ks["screen_pairs"] > 0 else None,
                                 "list": int(len(scr))}
        print(mode, res["screen_" + mode], flush=True)
    scr = ctx.ScreenPairs(ids, window=182)
    # pair stage, alternating
    dw = torch.empty((len(win), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    ds = torch.empty((max(len(scr), 1), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tw, ts, tss = [], [], []
    for r in range(a.reps + 1):
        mw, _ = timed(lambda: ctx.MatchPairsDev(win, dw.data_ptr(), 2.5, seed))
        ms, _ = timed(lambda: ctx.MatchPairsDev(scr, ds.data_ptr(), 2.5, seed))
        mss, _ = timed(lambda: (ctx.MatchPairsDev(ctx.ScreenPairs(ids, window=182), ds.data_ptr(), 2.5, seed)))
        if r:                                                              # the first round warms the workspaces
            tw.append(mw); ts.append(ms); tss.append(mss)
    rw = dw.cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
    acc = rw["accepted"] == 1
    res["pair_stage"] = {"window_ms": tw, "screened_ms": ts, "screen_plus_screened_ms": tss,
                         "window_ms_median": float(np.median(tw)), "screened_ms_median": float(np.median(ts)),
                         "screen_plus_screened_ms_median": float(np.median(tss)),
                         "speedup_with_screen": float(np.median(tw) / np.median(tss))}
    got = {tuple(p) for p in scr.tolist()}
    inwin = np.array([(int(i), int(j)) in got for i, j in zip(rw["i"], rw["j"])])
    bins = [(31, 40), (40, 60), (60, 100), (100, 200), (200, 401)]
    res["recall"] = {"accepted": int(acc.sum()), "kept": int((acc & inwin).sum()), "recall": float((acc & inwin).sum() / max(1, acc.sum())),
                     "by_n_in": [{"n_in": [lo, hi - 1], "accepted": int((acc & (rw["n_in"] >= lo) & (rw["n_in"] < hi)).sum()),
                                  "kept": int((acc & inwin & (rw["n_in"] >= lo) & (rw["n_in"] < hi)).sum())} for lo, hi in bins],
                     "list": int(len(scr)), "candidate_fraction": len(scr) / len(win)}
    rs = ds.cpu().numpy().reshape(-1).view(im.PAIR_RESULT)[:len(scr)]
    res["recall"]["screened_accepted"] = int((rs["accepted"] == 1).sum())
    res["recall"]["screened_connected"] = int(im.select_connected_results(rs[rs["accepted"] == 1], n).sum())
    print("pair stage", res["pair_stage"], "\nrecall", res["recall"], flush=True)
    # score distribution of the window's pairs (basis of min_score)
    S = torch.empty((n, n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.ScreenScoresDev(ids, S.data_ptr(), window=182)
    Sh = S.cpu().numpy()
    sc = Sh[rw["i"], rw["j"]]
    res["score_quantiles"] = {"accepted": np.percentile(sc[acc], [0, 1, 5, 50]).tolist(), "rejected": np.percentile(sc[~acc], [50, 99, 99.9, 100]).tolist()}
    print("scores", res["score_quantiles"], flush=True)
    if not a.no_sweep:
        sweep = []
        for top_k in (128, 256, 512):
            for partners in (4, 6, 8, 12):
                for min_score in (0, 6, 12):
                    ms, s = timed(lambda: ctx.ScreenPairs(ids, window=182, top_k=top_k, partners=partners, min_score=min_score))
                    g = {tuple(p) for p in s.tolist()}
                    k = np.array([(int(i), int(j)) in g for i, j in zip(rw["i"], rw["j"])])
                    sweep.append({"top_k": top_k, "partners": partners, "min_score": min_score, "list": int(len(s)), "fraction": len(s) / len(win),
                                  "recall": float((acc & k).sum() / max(1, acc.sum())),
                                  "recall_n_in_ge_60": float((acc & k & (rw["n_in"] >= 60)).sum() / max(1, (acc & (rw["n_in"] >= 60)).sum())),
                                  "screen_ms": ms})
                    print(sweep[-1], flush=True)
        res["sweep"] = sweep
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    ctx.close()


if __name__ == "__main__":
    main()

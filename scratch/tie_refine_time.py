"""Times the tie-point refinement (csrc/tie_refine.hip) on the pair records of C3 and of the window-182 C4 survey next to the pair stage that
produced those records and to pair_moments on the same records, all in one process, and writes a JSON record
(profiles/tie_refine_time.json).

    python scratch/tie_refine_time.py [OUT.json] [--quick]

500 synthetic frames of 4000x3000 (tests/synth_survey.py strip layout), SIFT(2000) features, then per survey (C3: the 499 adjacent pairs; C4:
the 74 029 pairs of window 182): the pair stage (match + select + RANSAC, mi355_match_pairs_dev, wall time with a device synchronise, median
of 3 after a warm-up), the accepted records compacted, and on those records tie_refine_kernel at the default parameters (profile class
"tie_refine", median of 5 after a warm-up, out of place) and pair_moments_kernel (between events on the ctx stream); also the refinement
over ALL records of the survey out of place (records that are not accepted are copied) and the status counts.  --quick: 60 frames."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests.synth_survey import frame_layout  # noqa: E402

W, H = 4000, 3000


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    F = 60 if quick else 500
    ctx = im.Context(0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx.set_stream(st.cuda_stream)
    A, gains = frame_layout(F, W, H)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
    for k in range(F):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), W, H, ws)
    ctx.synchronize()
    ptrs = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    rec = {"frames": F, "frame": "%dx%d" % (W, H), "params": {"radius": 7, "search": 3, "min_ncc": 0.7, "drop_mask": 0}}
    for name, window in (("C3", 2), ("C4", 182)):
        pairs = im.pair_schedule(F, window)
        n = len(pairs)
        res = torch.zeros((n, im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
        ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7)
        ctx.synchronize()
        stage = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7)
            ctx.synchronize()
            stage.append((time.perf_counter() - t0) * 1e3)
        acc = torch.zeros_like(res)
        n_acc = ctx.CompactAcceptedDev(res.data_ptr(), n, acc.data_ptr())
        ctx.synchronize()
        ties = int(acc[:n_acc].cpu().numpy().reshape(-1).view(im.PAIR_RESULT)["n_in"].sum())
        dst = torch.zeros_like(res)
        rep = torch.zeros((n, im.TIE_REPORT.itemsize), dtype=torch.uint8, device="cuda")
        mom = torch.zeros((n, im.PAIR_MOMENTS.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def refine(src, cnt):
            ctx.RefineTiesDev(src.data_ptr(), cnt, ptrs, wv, hv, wsv, dst.data_ptr(), d_report=rep.data_ptr())

        kern = {"accepted": [], "all": []}
        ctx.profile_enable(True)
        for key, (src, cnt) in (("accepted", (acc, n_acc)), ("all", (res, n))):
            refine(src, cnt)
            ctx.synchronize()
            for _ in range(5):
                ctx.profile_reset()
                refine(src, cnt)
                ctx.synchronize()
                kern[key].append(ctx.profile_get("tie_refine")[0])
        ctx.profile_enable(False)
        refine(acc, n_acc)
        ctx.synchronize()
        r = rep[:n_acc].cpu().numpy().reshape(-1).view(im.TIE_REPORT)
        moments = []
        for k in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.PairMomentsDev(acc.data_ptr(), n_acc, mom.data_ptr())
            e1.record(st)
            ctx.synchronize()
            if k:
                moments.append(e0.elapsed_time(e1))
        rec[name] = {"window": window, "pairs": n, "accepted": n_acc, "ties": ties,
                     "pair_stage_ms_median": float(np.median(stage)), "pair_stage_ms_all": stage,
                     "tie_refine_accepted_ms_median": float(np.median(kern["accepted"])), "tie_refine_accepted_ms_all": kern["accepted"],
                     "tie_refine_all_records_ms_median": float(np.median(kern["all"])), "tie_refine_all_records_ms_all": kern["all"],
                     "pair_moments_accepted_ms_median": float(np.median(moments)), "pair_moments_accepted_ms_all": moments,
                     "ns_per_tie": float(np.median(kern["accepted"])) * 1e6 / max(ties, 1),
                     "status_counts": [int(v) for v in r["count"].sum(0)[:6]], "mean_ncc2_of_refined": float(r["ncc_q_sum"].sum() / 1048576.0 / max(int(r["count"][:, 1].sum()), 1)),
                     "tie_refine_over_pair_stage": float(np.median(kern["accepted"])) / float(np.median(stage))}
        note(name, json.dumps(rec[name]))
        del res, acc, dst, rep, mom
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

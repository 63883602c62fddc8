"""Times guided matching (csrc/guided.hip) on the bench's resident features and writes a JSON record (profiles/guided_time.json).

    python scratch/guided_time.py [OUT.json] [--quick] [--rocprof]

C4: 500 synthetic frames of 4000 x 3000 in the strip layout, window 182 (--quick: 60 frames).  golden: the reference's 20 frames
(tests/golden/DSC00004 .. 23.JPG), every pair.  Each is a child process under its own time limit; the script stops at the first that fails.
Per configuration: SIFT(2000) features and the pair stage (wall time of mi355_match_pairs_dev, synchronised: the figure guided matching is put
next to), then
  (a) densify: every accepted pair again under its own H ([8] = 1) -- mi355_guided_match_dev as a call (wall time, median of 3 after a warm-up);
  (b) rescue: the pairs mi355_guided_candidates proposes from the affine alignment that no accepted record covers, the same call;
  (c) the split of (a) and (b) between the selection and the RANSAC tail: kernel time of the profile classes "guided_select" and "ransac" from
      the library's brackets, median of 3;
  quality: accepted pairs and the triangles mi355_pair_cycles_dev counts, before and after mi355_merge_pair_results.
--rocprof: one more child, the quick C4 under `rocprofv3 --kernel-trace --stats` (a run of its own: no brackets, no counters), whose rows for
the guided, RANSAC and finalize kernels are kept."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")

W, H = 4000, 3000
LIMIT = {"C4": 420, "golden": 120, "rocprof": 300}
DIST, SEED = 2.5, 7


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def graph_figures(ctx, torch, im, recs, F):
    """accepted pairs and the triangles the cycle kernel counts (every triangle once per edge it closes over)"""
    d = torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1).copy()).cuda()
    e = torch.zeros((len(recs), im.PAIR_EDGE.itemsize), dtype=torch.uint8, device="cuda")
    ctx.PairEdgesDev(d.data_ptr(), len(recs), F, e.data_ptr())
    ctx.synchronize()
    cyc = ctx.PairCyclesDev(e.cpu().numpy().reshape(-1).view(im.PAIR_EDGE), F)
    return {"records": len(recs), "accepted": int((recs["accepted"] != 0).sum()), "ties": int(recs["n_in"][recs["accepted"] != 0].sum()),
            "triangles_counted": int(cyc["n_ok"].sum() + cyc["n_bad"].sum()), "frames_in_a_pair": int(len(np.unique(np.stack([recs["i"], recs["j"]])[:, recs["accepted"] != 0])))}


def timed_guided(ctx, torch, im, pairs, guides):
    """GuidedMatchDev on the pairs: wall time of the call and the kernel time of its two classes, medians of 3 after a warm-up -> (figures, records)"""
    n = len(pairs)
    if n == 0:
        return {"pairs": 0}, np.zeros(0, im.PAIR_RESULT)
    out = torch.zeros((n, im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    ctx.GuidedMatchDev(pairs, guides, out.data_ptr(), DIST, SEED)
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.GuidedMatchDev(pairs, guides, out.data_ptr(), DIST, SEED)
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    kern = {"guided_select": [], "ransac": []}
    for _ in range(3):
        ctx.profile_reset()
        ctx.GuidedMatchDev(pairs, guides, out.data_ptr(), DIST, SEED)
        for cls in kern:
            kern[cls].append(ctx.profile_get(cls)[0])
    ctx.profile_enable(False)
    recs = out.cpu().numpy().reshape(-1).view(im.PAIR_RESULT).copy()
    med = {k: float(np.median(v)) for k, v in kern.items()}
    acc = recs["accepted"] != 0
    return {"pairs": n, "accepted": int(acc.sum()), "ties_of_the_accepted": int(recs["n_in"][acc].sum()), "n_selected_mean": float(recs["n_selected"].mean()),
            "call_ms_median": float(np.median(wall)), "call_ms_all": wall, "kernel_ms_median": med, "kernel_ms_all": kern,
            "select_us_per_pair": med["guided_select"] * 1e3 / n, "ransac_us_per_pair": med["ransac"] * 1e3 / n,
            "selection_exceeds_the_tail": bool(med["guided_select"] > med["ransac"])}, recs


def survey(ctx, torch, im, F, pairs, w, h):
    n = len(pairs)
    res = torch.zeros((n, im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    ctx.MatchPairsDev(pairs, res.data_ptr(), DIST, SEED)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.MatchPairsDev(pairs, res.data_ptr(), DIST, SEED)
    ctx.synchronize()
    pair_stage = (time.perf_counter() - t0) * 1e3
    host = res.cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
    base = host[host["accepted"] != 0].copy()
    del host, res
    note("pairs", n, "accepted", len(base), "pair stage %.1f ms" % pair_stage)
    rec = {"frames": F, "pairs": n, "pair_stage_ms": pair_stage, "pair_stage_us_per_pair": pair_stage * 1e3 / n, "before": graph_figures(ctx, torch, im, base, F)}
    # (a) every accepted pair under its own H
    own = np.ascontiguousarray(base["H"], np.float32).copy()
    own[:, 8] = 1.0
    ij = np.stack([base["i"], base["j"]], 1).astype(np.int32)
    rec["densify"], dense = timed_guided(ctx, torch, im, ij, own)
    rec["densify"]["ties_before"] = int(base["n_in"].sum())
    rec["densify"]["records_improved"] = int((dense["n_in"] > base["n_in"]).sum())
    note("densify", rec["densify"])
    # (b) what the affine alignment says overlaps and no accepted record covers
    label = im.select_connected_results(base, F)
    T = im.global_affine_align_results(base, F, label=label)
    h9s = np.ascontiguousarray(T["m"], np.float32)
    h9s[label == 0] = 0.0                                   # a frame outside the connected set is not placed
    rec["frames_placed"] = int((label != 0).sum())
    t0 = time.perf_counter()
    cand, guides = im.guided_candidates(w, h, h9s, ij)
    rec["candidates_ms"] = (time.perf_counter() - t0) * 1e3
    rec["rescue"], rescued = timed_guided(ctx, torch, im, cand, guides)
    note("rescue", rec["rescue"])
    merged = im.merge_pair_results(im.merge_pair_results(base, dense), rescued[rescued["accepted"] != 0])
    rec["after"] = graph_figures(ctx, torch, im, merged, F)
    note("before", rec["before"], "after", rec["after"])
    return rec


def step(name, F):
    import torch
    import imagemosaicing_amd as im
    ctx = im.Context(0)
    if name == "golden":
        from PIL import Image
        F = 20
        for k in range(F):
            img = np.ascontiguousarray(np.array(Image.open("tests/golden/DSC%05d.JPG" % (4 + k)).convert("RGB"))[:, :, ::-1])
            ctx.SiftExtractHost(k, img)
        h, w = img.shape[:2]
        rec = survey(ctx, torch, im, F, im.pair_schedule(F, 182), w, h)
    else:
        from tests.synth_survey import frame_layout
        A, gains = frame_layout(F, W, H)
        ws = (3 * W + 3) & ~3
        frame = torch.empty(H * ws, dtype=torch.uint8, device="cuda")
        for k in range(F):                                   # one frame at a time: the features are all the pair stage needs
            ctx.SynthFrameDev(frame.data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
            ctx.SiftExtractDev(k, frame.data_ptr(), W, H, ws)
            ctx.synchronize()
        rec = survey(ctx, torch, im, F, im.pair_schedule(F, 182), W, H)
    ctx.close()
    return rec


def rocprof_rows(d):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(p) as f:
            for r in csv.DictReader(f):
                if any(s in r.get("Name", "") for s in ("guided_select", "ransac", "finalize_kernel")):
                    rows.append(r)
    return rows


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--step" in sys.argv:
        name, path = args[0], args[1]
        rec = step(name, 60 if quick else 500)
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
        return 0
    out = args[0] if args else None
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        for name in ("golden", "C4") + (("rocprof",) if "--rocprof" in sys.argv else ()):
            part = os.path.join(d, name + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "C4" if name == "rocprof" else name, part] + (["--quick"] if quick or name == "rocprof" else [])
            if name == "rocprof":
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(d, "prof"), "--output-format", "csv", "--"] + cmd
            rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[name])] + cmd)
            if rc != 0:
                note("step", name, "ended with status", rc, "-- stopping")
                return rc
            if name == "rocprof":
                rec["rocprofv3_quick_C4_kernel_stats"] = rocprof_rows(os.path.join(d, "prof"))
            else:
                with open(part) as f:
                    rec[name] = json.load(f)
            if out:                                                 # what is done is kept even if the next step fails
                with open(out, "w") as f:
                    json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

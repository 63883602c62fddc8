"""Times pair verification (csrc/verify.hip, csrc/verify_loop.cpp) on the bench's record sets and writes a JSON record
(profiles/verify_time.json).

    python scratch/verify_time.py [OUT.json] [--quick] [--c5]

C4: 500 synthetic frames of 4000 x 3000 in the strip layout, window 182.  C5 (--c5): 2000 frames in the block layout, window 182.  Each
configuration is a child process under its own time limit; the script stops at the first that fails.  Per configuration: SIFT(2000)
features and the pair stage (wall time of mi355_match_pairs_dev, synchronised: the figure the stage is put next to), then on its records
  - pair_edges_kernel, pair_residuals_kernel (profile classes "pair_edges", "pair_residuals") and pair_cycles_kernel ("pair_cycles", inside
    mi355_pair_cycles_dev on the downloaded edges), kernel time from the library's brackets, median of 5 after a warm-up;
  - mi355_pair_cycles_dev as a call (adjacency, uploads, launch, download; wall time, median of 5);
  - mi355_verify_pairs_dev as a call (wall time, median of 3 after a warm-up), the rounds it used, the verdict counts, and what is left of
    the call after the launches -- the host loop: the alignments, the adjacency, the copies;
  - mi355_global_affine_align_results on the same records (wall time): the host alignment one round costs.

--quick: 60 frames."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")

W, H = 4000, 3000
LIMIT = {"C4": 420, "C5": 840}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def step(name, F):
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import block_layout, frame_layout
    ctx = im.Context(0)
    A, gains = frame_layout(F, W, H)
    if name == "C5":
        A = block_layout(F, W, H, seed=5)
    ws = (3 * W + 3) & ~3
    frame = torch.empty(H * ws, dtype=torch.uint8, device="cuda")
    for k in range(F):                                   # one frame at a time: the features are all the pair stage needs
        ctx.SynthFrameDev(frame.data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
        ctx.SiftExtractDev(k, frame.data_ptr(), W, H, ws)
        ctx.synchronize()
    pairs = im.pair_schedule(F, 182)
    n = len(pairs)
    res = torch.zeros((n, im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7)
    ctx.synchronize()
    pair_stage = (time.perf_counter() - t0) * 1e3
    note(name, "pairs", n, "pair stage %.1f ms" % pair_stage)
    edges = torch.zeros((n, im.PAIR_EDGE.itemsize), dtype=torch.uint8, device="cuda")
    resid = torch.zeros((n, im.PAIR_RESIDUAL.itemsize), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(res)
    host = res.cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
    n_acc = int((host["accepted"] != 0).sum())
    t0 = time.perf_counter()
    T = im.global_affine_align_results(host, F, label=im.select_connected_results(host, F))
    align_ms = (time.perf_counter() - t0) * 1e3
    h9s = np.ascontiguousarray(T["m"], np.float32)
    torch.cuda.synchronize()

    calls = {"pair_edges": lambda: ctx.PairEdgesDev(res.data_ptr(), n, F, edges.data_ptr()),
             "pair_residuals": lambda: ctx.PairResidualsDev(res.data_ptr(), n, h9s, None, resid.data_ptr())}
    ctx.profile_enable(True)
    kern = {}
    for cls, call in calls.items():
        call()
        ctx.synchronize()
        v = []
        for _ in range(5):
            ctx.profile_reset()
            call()
            ctx.synchronize()
            v.append(ctx.profile_get(cls)[0])
        kern[cls] = v
    h_edges = edges.cpu().numpy().reshape(-1).view(im.PAIR_EDGE)
    ctx.PairCyclesDev(h_edges, F)
    v, wall = [], []
    for _ in range(5):
        ctx.profile_reset()
        t0 = time.perf_counter()
        cyc = ctx.PairCyclesDev(h_edges, F)
        wall.append((time.perf_counter() - t0) * 1e3)
        v.append(ctx.profile_get("pair_cycles")[0])
    kern["pair_cycles"] = v
    ctx.profile_enable(False)
    triangles = int(cyc["n_ok"].sum() + cyc["n_bad"].sum())
    label, tr, rep, summ = ctx.VerifyPairsDev(res.data_ptr(), n, F, out.data_ptr())
    whole = []
    for _ in range(3):
        t0 = time.perf_counter()
        label, tr, rep, summ = ctx.VerifyPairsDev(res.data_ptr(), n, F, out.data_ptr())
        whole.append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(x)) for k, x in kern.items()}
    rounds = int(summ["rounds"])
    launches = med["pair_edges"] + med["pair_cycles"] + med["pair_residuals"] * rounds
    rec = {"frames": F, "pairs": n, "accepted": n_acc, "ties": int(host["n_in"][host["accepted"] != 0].sum()), "triangles_counted": triangles,
           "pair_stage_ms": pair_stage, "kernel_ms_median": med, "kernel_ms_all": kern,
           "pair_cycles_call_ms_median": float(np.median(wall)), "pair_cycles_call_ms_all": wall,
           "verify_pairs_dev_ms_median": float(np.median(whole)), "verify_pairs_dev_ms_all": whole, "rounds": rounds,
           "verdict_counts": [int(c) for c in summ["count"][:6]], "frames_labelled": int(summ["n_labelled"]), "s": float(summ["s"]), "gate": float(summ["gate"]),
           "host_alignment_ms": align_ms, "kernels_of_one_call_ms": launches, "rest_of_the_call_ms": float(np.median(whole)) - launches,
           "verify_over_pair_stage": float(np.median(whole)) / pair_stage}
    ctx.close()
    return rec


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--step" in sys.argv:
        name, path = args[0], args[1]
        rec = step(name, 60 if quick else (2000 if name == "C5" else 500))
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
        return 0
    out = args[0] if args else None
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        for name in ("C4", "C5") if "--c5" in sys.argv else ("C4",):
            part = os.path.join(d, name + ".json")
            cmd = ["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "--step", name, part] + (["--quick"] if quick else [])
            rc = subprocess.call(cmd)
            if rc != 0:
                note("step", name, "ended with status", rc, "-- stopping")
                return rc
            with open(part) as f:
                rec[name] = json.load(f)
            if out:                                                 # what is done is kept even if the next step fails
                with open(out, "w") as f:
                    json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

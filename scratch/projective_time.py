"""Times one trial of the projective refinement (csrc/projective.hip, csrc/projective_solve.cpp) piece by piece in one process and writes a
JSON record (profiles/projective_time.json).

    python scratch/projective_time.py [OUT.json] [--quick]

Synthetic records: 500 images of 640 x 480 in a strip 25 px apart, every image tied to the 20 after it, 100 inliers per pair with 0.3 px of
noise (9790 accepted pairs, 979 000 points).  Reported per trial: the block kernel (with the upload of the parameters, between two events on
the ctx stream), the device-to-host copy of the blocks into pinned memory, assembly + scaling + factorisation + solve on the host (the wall
time of a refinement of one trial minus one of no trial, minus one kernel and one copy), mi355_pair_moments_dev on the same records, and the
host twin's blocks (mi355_pair_normal_blocks_host, one thread).  --quick: 60 images."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402

W, H, STEP, WIN, PER = 640, 480, 25.0, 20, 100


def records(n):
    rng = np.random.default_rng(12)
    pairs = [(k, k + d) for k in range(n) for d in range(1, WIN + 1) if k + d < n]
    r = np.zeros(len(pairs), im.PAIR_RESULT)
    for p, (i, j) in enumerate(pairs):
        cx = rng.uniform(STEP * j, STEP * i + W - 1, PER)
        cy = rng.uniform(0, H - 1, PER)
        r["i"][p], r["j"][p], r["n_in"][p], r["n_selected"][p], r["ok"][p], r["accepted"][p] = i, j, PER, PER, 1, 1
        r["a"]["x"][p, :PER], r["a"]["y"][p, :PER] = cx - STEP * i + rng.normal(0, 0.3, PER), cy + rng.normal(0, 0.3, PER)
        r["b"]["x"][p, :PER], r["b"]["y"][p, :PER] = cx - STEP * j + rng.normal(0, 0.3, PER), cy + rng.normal(0, 0.3, PER)
    return r


def median_ms(f, reps=7):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = 60 if "--quick" in sys.argv else 500
    r = records(n)
    ctx = im.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    d_r = torch.from_numpy(r.view(np.uint8).reshape(len(r), -1).copy()).cuda()
    d_b = torch.empty((len(r), im.PAIR_NORMAL_BLOCK.itemsize), dtype=torch.uint8, device="cuda")
    d_m = torch.empty((len(r), im.PAIR_MOMENTS.itemsize), dtype=torch.uint8, device="cuda")
    h_b = torch.empty((len(r), im.PAIR_NORMAL_BLOCK.itemsize), dtype=torch.uint8).pin_memory()
    start = im.global_affine_align_results(r, n)
    w, h = np.full(n, W, np.int32), np.full(n, H, np.int32)
    part = np.ones(n, np.uint8)
    part[0] = 2
    h8 = start["m"][:, :8].astype(np.float64)

    def events(call, reps=10):
        call()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return float(np.median(t))

    rec = {"images": n, "pairs": int(len(r)), "points": int(r["n_in"].sum()), "block_bytes": int(len(r)) * im.PAIR_NORMAL_BLOCK.itemsize,
           "record_bytes": int(len(r)) * im.PAIR_RESULT.itemsize}
    rec["block_kernel_ms"] = events(lambda: ctx.PairNormalBlocksDev(d_r.data_ptr(), len(r), h8, part, d_b.data_ptr()))
    rec["block_copy_d2h_ms"] = events(lambda: h_b.copy_(d_b, non_blocking=True))
    rec["pair_moments_kernel_ms"] = events(lambda: ctx.PairMomentsDev(d_r.data_ptr(), len(r), d_m.data_ptr()))
    rec["host_twin_blocks_ms"] = median_ms(lambda: im.pair_normal_blocks_host(r, h8, part), reps=3)
    t0 = median_ms(lambda: ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(r), w, h, start, params=im.projective_params(max_iters=0)))
    t1 = median_ms(lambda: ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(r), w, h, start, params=im.projective_params(max_iters=1)))
    rec["refine_dev_no_trial_ms"], rec["refine_dev_one_trial_ms"] = t0, t1
    rec["trial_ms"] = t1 - t0
    rec["assembly_factorisation_solve_ms"] = t1 - t0 - rec["block_kernel_ms"] - rec["block_copy_d2h_ms"]
    out, rep = ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(r), w, h, start)
    rec["default_run"] = dict(rep, rms0=float(np.sqrt(rep["cost0"] / rep["n_points"])), rms=float(np.sqrt(rep["cost_data"] / rep["n_points"])),
                              wall_ms=median_ms(lambda: ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(r), w, h, start), reps=3))
    rec["default_run_host_ms"] = median_ms(lambda: im.global_projective_refine_results(r, w, h, start), reps=3)
    ctx.set_stream(None)
    print(json.dumps(rec, indent=1))
    if args:
        with open(args[0], "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

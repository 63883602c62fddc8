"""Times the local registration (csrc/local_warp.hip) and writes a JSON record (profiles/local_warp_time.json).

    python scratch/local_warp_time.py [OUT.json] [--quick]

500 synthetic frames of 4000x3000 (C3; tests/synth_survey.py strip layout).  Two steps, each a child process under its own time limit; the
script stops at the first step that fails:

  apply   local_warp_kernel (profile class "local_warp", random grids of +-2 px at 8 x 6) out of place and in place, next to undistort_kernel
          (the tests' barrel camera with the fitted output camera) and the gain LUT pass (mi355_apply_gains_dev) in the same process: the
          three move the same 6 w h bytes per frame.  Kernel time from the library's profile brackets, one warm-up call, then 5 timed ones, the
          passes alternating; the apply also as a fraction of the 6.3 TB/s a streaming kernel reaches on this part.
  stats   SIFT(2000) features, the window-182 pair stage (C4), the accepted records compacted, and on those records tie_residual_kernel
          (class "tie_residuals", median of 5 after a warm-up), and mi355_tie_residual_stats_dev next to mi355_pair_moments_dev timed the
          same way (between events on the ctx stream around the call, alternating, median of 5 after a warm-up); then the host
          solve on the sums (wall time, median of 5) and the whole step mi355_local_register_dev on copies of the frames (wall time, once).

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
HBM_ACHIEVABLE = 6.3e12
LIMIT = {"apply": 420, "stats": 840}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def make_frames(ctx, torch, F):
    from tests.synth_survey import frame_layout
    A, gains = frame_layout(F, W, H)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
    ctx.synchronize()
    return frames, A, ws


def step_apply(F):
    import torch
    import imagemosaicing_amd as im
    from tests import undistort_ref as ur
    ctx = im.Context(0)
    frames, _, ws = make_frames(ctx, torch, F)
    dst = torch.empty_like(frames)
    sp = [frames[k].data_ptr() for k in range(F)]
    dp = [dst[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    barrel = im.Camera(**ur.cameras_for(W, H)["barrel"])
    fitted = im.undistort_fit(barrel, W, H)
    gains = np.random.default_rng(2).uniform(0.9, 1.1, (F, 3)).astype(np.float32)
    grids = np.random.default_rng(3).uniform(-2.0, 2.0, (F, 7, 9, 2)).astype(np.float32)
    clamped = {}

    def lw(d, key):
        clamped[key] = ctx.ApplyLocalWarpsDev(sp, d, wv, hv, wsv, wsv, grids)

    passes = {
        "local_warp_out_of_place": (lambda: lw(dp, "out_of_place"), "local_warp"),
        "undistort_out_of_place": (lambda: ctx.UndistortFramesDev(sp, dp, wv, hv, wsv, wsv, barrel, fitted), "undistort"),
        "apply_gains_out_of_place": (lambda: ctx.ApplyGainsDev(sp, dp, wv, hv, wsv, gains), "gain_apply"),
        "local_warp_in_place": (lambda: lw(sp, "in_place"), "local_warp"),
    }
    reps = 5
    ctx.profile_enable(True)
    for name, (call, _) in passes.items():
        call()
    ctx.synchronize()
    kern = {k: [] for k in passes}
    wall = {k: [] for k in passes}
    for rep in range(reps):
        for name, (call, cls) in passes.items():
            ctx.profile_reset()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            kern[name].append(ctx.profile_get(cls)[0])
        note("rep", rep, {k: round(v[-1], 3) for k, v in kern.items()})
    ctx.profile_enable(False)
    need = 6.0 * W * H * F
    rec = {"frames": F, "frame": "%dx%d" % (W, H), "pitch": ws, "bytes_needed": need, "reps": reps, "grid": "8x6, uniform +-2 px",
           "n_clamped_per_frame_mean": {k: float(v.mean()) for k, v in clamped.items()}}
    for name in passes:
        k = float(np.median(kern[name]))
        rec[name] = {"kernel_ms_median": k, "kernel_ms_all": kern[name], "call_ms_median": float(np.median(wall[name])), "kernel_TB_per_s": need / (k * 1e-3) / 1e12}
    t = rec["local_warp_out_of_place"]["kernel_ms_median"]
    rec["local_warp_fraction_of_achievable_hbm"] = need / (t * 1e-3) / HBM_ACHIEVABLE
    rec["local_warp_over_undistort"] = t / rec["undistort_out_of_place"]["kernel_ms_median"]
    rec["local_warp_over_apply_gains"] = t / rec["apply_gains_out_of_place"]["kernel_ms_median"]
    ctx.close()
    return rec


def step_stats(F):
    import torch
    import imagemosaicing_amd as im
    ctx = im.Context(0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx.set_stream(st.cuda_stream)
    frames, A, ws = make_frames(ctx, torch, F)
    for k in range(F):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), W, H, ws)
    ctx.synchronize()
    pairs = im.pair_schedule(F, 182)
    n = len(pairs)
    res = torch.zeros((n, im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7)
    ctx.synchronize()
    acc = torch.zeros_like(res)
    n_acc = ctx.CompactAcceptedDev(res.data_ptr(), n, acc.data_ptr())
    ctx.synchronize()
    host = acc[:n_acc].cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
    ties = int(host["n_in"].sum())
    # the alignment the residuals are taken against: the global affine alignment of the accepted records
    T = im.global_affine_align_results(host, F)
    h9s = np.ascontiguousarray(T["m"], np.float32)
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    stats = torch.zeros(im.local_warp_stats_len(F, 8, 6), dtype=torch.int64, device="cuda")
    mom = torch.zeros((n, im.PAIR_MOMENTS.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    ctx.TieResidualStatsDev(acc.data_ptr(), n_acc, wv, hv, h9s, stats.data_ptr())
    ctx.synchronize()
    k_stats = []
    for _ in range(5):
        ctx.profile_reset()
        ctx.TieResidualStatsDev(acc.data_ptr(), n_acc, wv, hv, h9s, stats.data_ptr())
        ctx.synchronize()
        k_stats.append(ctx.profile_get("tie_residuals")[0])
    ctx.profile_enable(False)

    def between_events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the two entry points timed the same way: between events on the ctx stream around the call (host enqueue and, for the statistics, the
    # clear and the table upload included), alternating
    calls = {"stats": lambda: ctx.TieResidualStatsDev(acc.data_ptr(), n_acc, wv, hv, h9s, stats.data_ptr()),
             "moments": lambda: ctx.PairMomentsDev(acc.data_ptr(), n_acc, mom.data_ptr())}
    ev = {k: [] for k in calls}
    for name, call in calls.items():
        between_events(call)
    for _ in range(5):
        for name, call in calls.items():
            ev[name].append(between_events(call))
    hs = stats.cpu().numpy()
    solve = []
    for _ in range(6):
        t0 = time.perf_counter()
        grids, rep = im.solve_local_warps(hs, F)
        solve.append((time.perf_counter() - t0) * 1e3)
    work = frames.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g2, rep2 = ctx.LocalRegisterDev(acc.data_ptr(), n_acc, [work[k].data_ptr() for k in range(F)], wv, hv, wsv, h9s)
    ctx.synchronize()
    whole = (time.perf_counter() - t0) * 1e3
    rec = {"frames": F, "pairs": n, "accepted": int(n_acc), "ties": ties, "grid": "8x6",
           "tie_residual_kernel_ms_median": float(np.median(k_stats)), "tie_residual_kernel_ms_all": k_stats,
           "tie_residual_call_between_events_ms_median": float(np.median(ev["stats"])), "tie_residual_call_between_events_ms_all": ev["stats"],
           "pair_moments_call_between_events_ms_median": float(np.median(ev["moments"])), "pair_moments_call_between_events_ms_all": ev["moments"],
           "solve_ms_median": float(np.median(solve[1:])), "solve_ms_all": solve[1:], "local_register_call_ms": whole,
           "kept_sides": int(rep["n_ties"].sum()), "rej_residual": int(rep["rej_residual"].sum()), "rej_side": int(rep["rej_side"].sum()),
           "frames_solved": int(rep["solved"].sum()), "rms_before_mean_px": float(rep["rms_before"].mean()), "rms_after_mean_px": float(rep["rms_after"].mean()),
           "largest_shift_px": float(rep["max_shift"].max()), "grids_equal_to_one_call": bool(np.array_equal(grids, g2))}
    rec["tie_residual_over_pair_moments_between_events"] = rec["tie_residual_call_between_events_ms_median"] / rec["pair_moments_call_between_events_ms_median"]
    ctx.close()
    return rec


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    F = 60 if quick else 500
    if "--step" in sys.argv:
        name, path = args[0], args[1]
        rec = step_apply(F) if name == "apply" else step_stats(F)
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
        return 0
    out = args[0] if args else None
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        for name in ("apply", "stats"):
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

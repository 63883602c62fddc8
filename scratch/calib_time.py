"""Times the lens self-calibration (csrc/calib.hip, csrc/calib_solve.cpp) and writes a JSON record (profiles/calib_time.json).

    python scratch/calib_time.py [OUT.json] [--quick]

500 synthetic frames of 4000x3000 (tests/synth_survey.py strip layout), SIFT(2000) features, the window-182 pair stage (C4), the accepted
records compacted; C3's records are the adjacent pairs (j = i + 1) among them.  One child process under its own time limit.  On each set:

  pair_calib_blocks_kernel    the library's profile brackets (class "calibrate"), median of 5 after a warm-up, at the start camera and states
  both block entry points     mi355_pair_calib_blocks_dev and mi355_pair_normal_blocks_dev between events on the ctx stream around the call (the
                              upload of the states included), alternating, median of 5 after a warm-up: the projective kernel is the yardstick
  the copy of the blocks      device to pinned host memory between events, median of 5
  mi355_calibrate_lens_dev    wall time (median of 5 after a warm-up) of the default run and of a run with max_iters = 0; per trial: the
                              kernel from the profile brackets, the copy as above, and the host solve as what is left of the wall time

The frames are pinhole renders, so the estimate is close to zero: the run measures time, not accuracy.  --quick: 60 frames."""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

W, H = 4000, 3000
LIMIT = 840


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def measure(ctx, torch, im, st, acc_host, F, name):
    from tests import calib_ref as cr
    n = len(acc_host)
    d_r = torch.from_numpy(acc_host.view(np.uint8).reshape(n, -1).copy()).cuda()
    start = im.Camera(3250.0, 3250.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    h8c = np.array([cr.start_state(r["H"], cr.cam_tuple(start)) for r in acc_host])
    label = im.select_connected_results(acc_host, F)           # the projective kernel's parameters: the affine alignment of the largest component
    fixed = [1 if (k == 0 or label[k] == 0) else 0 for k in range(F)]
    T = im.global_affine_align_results(acc_host, F, fixed=fixed, label=label)
    h8p = T["m"][:, :8].astype(np.float64)
    part = np.where(label != 0, 1, 0).astype(np.uint8)
    part[0] = 2
    d_cb = torch.empty((n, im.PAIR_CALIB_BLOCK.itemsize), dtype=torch.uint8, device="cuda")
    d_nb = torch.empty((n, im.PAIR_NORMAL_BLOCK.itemsize), dtype=torch.uint8, device="cuda")
    h_cb = torch.empty((n, im.PAIR_CALIB_BLOCK.itemsize), dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()

    def between_events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    calib = lambda: ctx.PairCalibBlocksDev(d_r.data_ptr(), n, h8c, start, d_cb.data_ptr())
    calls = {"calib": calib, "normal": lambda: ctx.PairNormalBlocksDev(d_r.data_ptr(), n, h8p, part, d_nb.data_ptr()),
             "copy": lambda: h_cb.copy_(d_cb, non_blocking=True)}
    ctx.profile_enable(True)
    calib()
    ctx.synchronize()
    kern = []
    for _ in range(5):
        ctx.profile_reset()
        calib()
        ctx.synchronize()
        kern.append(ctx.profile_get("calibrate")[0])
    ctx.profile_enable(False)
    ev = {k: [] for k in calls}
    for call in calls.values():
        between_events(call)
    for _ in range(5):
        for k, call in calls.items():
            ev[k].append(between_events(call))
    blk = h_cb.numpy().reshape(-1).view(im.PAIR_CALIB_BLOCK)
    nblk = d_nb.cpu().numpy().reshape(-1).view(im.PAIR_NORMAL_BLOCK)

    def wall(**kw):
        t = []
        for _ in range(6):
            t0 = time.perf_counter()
            out = ctx.CalibrateLensDev(d_r.data_ptr(), n, start, **kw)
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t[1:])), out

    w0, _ = wall(max_iters=0)
    w1, (cam, rep) = wall()
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.CalibrateLensDev(d_r.data_ptr(), n, start)
    k_ms, k_n, _ = ctx.profile_get("calibrate")
    ctx.profile_enable(False)
    trials = max(rep["trials"], 1)
    k_med, c_med = float(np.median(kern)), float(np.median(ev["copy"]))
    rec = {"set": name, "records": n, "used": int((blk["n_in"] > 0).sum()), "used_by_the_projective_kernel": int((nblk["n_in"] > 0).sum()), "ties": int(acc_host["n_in"].sum()), "bad_ties": int(blk["n_bad"].sum()),
           "calib_kernel_ms_median": k_med, "calib_kernel_ms_all": kern,
           "calib_call_between_events_ms_median": float(np.median(ev["calib"])), "calib_call_between_events_ms_all": ev["calib"],
           "normal_call_between_events_ms_median": float(np.median(ev["normal"])), "normal_call_between_events_ms_all": ev["normal"],
           "block_copy_d2h_ms_median": c_med, "block_bytes": n * im.PAIR_CALIB_BLOCK.itemsize,
           "calibrate_dev_no_trial_ms": w0, "calibrate_dev_default_ms": w1, "report": rep, "estimate": [getattr(cam, f) for f in cr.CAM_FIELDS[4:]],
           "calibrate_kernel_launches": int(k_n), "calibrate_kernel_ms_per_launch": k_ms / max(k_n, 1),
           "per_trial_ms": {"kernel": k_ms / max(k_n, 1), "copy": c_med, "whole": (w1 - w0) / trials,
                            "host_solve_and_rest": (w1 - w0) / trials - k_ms / max(k_n, 1) - c_med}}
    rec["calib_over_normal_between_events"] = rec["calib_call_between_events_ms_median"] / rec["normal_call_between_events_ms_median"]
    return rec


def step(F):
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import frame_layout
    ctx = im.Context(0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx.set_stream(st.cuda_stream)
    A, gains = frame_layout(F, W, H)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")      # all of them: the extraction reads a frame when its batch runs
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
    ctx.synchronize()
    for k in range(F):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), W, H, ws)
    ctx.synchronize()
    note("features done")
    pairs = im.pair_schedule(F, 182)
    n = len(pairs)
    res = torch.zeros((n, im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7)
    ctx.synchronize()
    acc = torch.zeros_like(res)
    n_acc = ctx.CompactAcceptedDev(res.data_ptr(), n, acc.data_ptr())
    ctx.synchronize()
    host = acc[:n_acc].cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
    del res, acc, frames
    note("pair stage done:", n, "pairs,", n_acc, "accepted")
    rec = {"frames": F, "pairs": n, "accepted": int(n_acc)}
    rec["C4"] = measure(ctx, torch, im, st, host, F, "window 182")
    note("C4", json.dumps(rec["C4"]["per_trial_ms"]))
    rec["C3"] = measure(ctx, torch, im, st, host[host["j"] == host["i"] + 1], F, "adjacent pairs (j = i + 1) of the same records")
    ctx.set_stream(None)
    ctx.close()
    return rec


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    F = 60 if quick else 500
    if "--step" in sys.argv:
        rec = step(F)
        with open(args[0], "w") as f:
            json.dump(rec, f, indent=1)
        return 0
    out = args[0] if args else "profiles/calib_time.json"
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", out] + (["--quick"] if quick else [])
    rc = subprocess.call(cmd)
    if rc != 0:
        note("the step ended with status", rc)
        return rc
    with open(out) as f:
        print(f.read())
    return 0


if __name__ == "__main__":
    sys.exit(main())

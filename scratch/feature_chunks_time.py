"""Times the chunk-record feature exchange on one MI355X for an 8-rank C3 / C4 share (63 frames of 4000x3000): the keep-all keypoint counts
of real extractions of bench.py's synthetic survey frames (the payload a keep-all multi-GPU run moves), the pack and install kernels (event
brackets, GB/s over the carried bytes: one record read or written plus one written or read per record), and the world-1 collective
mi355_allgather_feature_chunks with the own frames re-installed (wall clock, median of the repetitions).  The same for 63 frames of 2 900
keypoints (the reference's frames) set through mi355_set_features.

    python scratch/feature_chunks_time.py [--frames 63] [--reps 10] [--keepall-max 131072] [--out profiles/feature_chunks_time.json]

--keepall-max sets the ctx's ceiling of keypoints per keep-all frame (option "keepall_max"); the survey frames keep about 83 000 each.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_share(ctx, ids, reps, torch, im, kmax=32768):
    n_rec = ctx.FeatureChunkCount(ids)
    n_kp = [len(ctx.GetFeatures(k, max_kp=kmax)[0]) for k in ids]
    pay = torch.empty((n_rec, im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    carried = n_rec * im.FEATURE_RECORD_BYTES
    useful = sum(n * (28 + 128) for n in n_kp)
    hdr = ctx.PackFeatureChunksDev(ids, pay.data_ptr(), n_rec)            # warm-up (workspaces)
    ctx.InstallFeatureChunksDev(hdr, pay.data_ptr())
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        hdr = ctx.PackFeatureChunksDev(ids, pay.data_ptr(), n_rec)
        ctx.InstallFeatureChunksDev(hdr, pay.data_ptr())
    pk_ms, pk_n, _ = ctx.profile_get("feature_pack")
    in_ms, in_n, _ = ctx.profile_get("feature_install")
    ctx.profile_enable(False)
    pk, ins = pk_ms / max(pk_n, 1), in_ms / max(in_n, 1)
    wall = []
    ctx.AllGatherFeatureChunks(ids, install_own=True)                     # warm-up
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.AllGatherFeatureChunks(ids, install_own=True)
        wall.append((time.perf_counter() - t0) * 1e3)
    return {"frames": len(ids), "keypoints_min_median_max": [int(min(n_kp)), int(np.median(n_kp)), int(max(n_kp))],
            "records": n_rec, "carried_MB": carried / 1e6, "useful_MB": useful / 1e6, "carried_over_useful": carried / max(useful, 1),
            "pack_kernel_ms": pk, "pack_GBps": 2 * carried / pk / 1e6 if pk > 0 else None,
            "install_kernel_ms": ins, "install_GBps": 2 * carried / ins / 1e6 if ins > 0 else None,
            "allgather_world1_install_own_ms_median": float(np.median(wall)), "allgather_world1_ms_min": float(min(wall)),
            "received_per_rank_at_8_ranks_MB": 8 * carried / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=63)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keepall-max", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import imagemosaicing_amd as im
    from imagemosaicing_amd import dist as md
    from tests.synth_survey import render_frames
    out = {"device": torch.cuda.get_device_name(0)}
    prm = im.default_params()
    prm.nfeatures = 0
    ctx = im.Context(0, prm)
    if a.keepall_max != 32768:
        ctx.set_option("keepall_max", a.keepall_max)
    out["keepall_max"] = a.keepall_max
    md.init_comm(ctx)                                  # a communicator of one rank
    # 1. keep-all extractions of the survey's 4000x3000 frames
    w, h = 4000, 3000
    fr, _, _, ws = render_frames(ctx, torch, a.frames, w, h)
    survey = {"ok": [], "failed": {}}
    t0 = time.perf_counter()
    for k in range(a.frames):
        try:
            ctx.SiftExtractDev(k, fr[k].data_ptr(), w, h, ws, want_count=True)
            survey["ok"].append(k)
        except im.Mi355Error as e:
            survey["failed"][k] = str(e)
            ctx.DropFeatures(k)
    del fr
    torch.cuda.empty_cache()
    out["survey_4000x3000_extract_ms_per_frame_one_at_a_time"] = (time.perf_counter() - t0) * 1e3 / a.frames
    out["survey_4000x3000_failed_frames"] = survey["failed"]
    if survey["ok"]:
        out["survey_4000x3000_keepall"] = time_share(ctx, survey["ok"], a.reps, torch, im, a.keepall_max)
    ctx.DropFeatures(-1)
    # 2. frames of 2 900 keypoints (the reference's 1000x750 frames kept about that many)
    rng = np.random.default_rng(1)
    for k in range(a.frames):
        n = 2900
        kp = np.zeros(n, im.KEYPOINT)
        kp["x"] = rng.uniform(0, 1000, n); kp["y"] = rng.uniform(0, 750, n)
        ctx.SetFeatures(k, kp, rng.integers(0, 256, (n, 128)).astype(np.float32), 1000, 750)
    out["reference_like_2900"] = time_share(ctx, list(range(a.frames)), a.reps, torch, im, a.keepall_max)
    ctx.CommDestroy()
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)), exist_ok=True)
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

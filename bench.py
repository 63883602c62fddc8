#!/usr/bin/env python3
"""bench.py -- image-pairs/sec of the pairwise hot path (detect+describe, match+select, RANSAC-H, warp)
on MI355X, the metric and workload of BASELINE.json.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over the whole batch of synthetic frames resident in HBM:
  SIFT detect+describe of every frame once  ->  match + grid select + Ransac2D of every scheduled pair  ->
  [N>1: RCCL all-gather of the fixed-size pair records]  ->  global affine alignment of the records on the host
  (the reference's driver step between match and warp)  ->  inverse-warp of every frame once into the canvas.
Workload at N=1: BASELINE configs[2] "500-frame 4000x3000 UAV set, all adjacent pairs" (C3), the configuration
the metric is quoted on (4000x3000 frames).  With N ranks (default --scaling strong) the SAME survey is sharded the way the
reference's threads shard it (MosaicWithoutPos.cpp:4861 / :5066): rank r extracts the frames k mod N == r, matches the
pairs whose i it owns and renders canvas stripe r.  Two RCCL all-gathers inside the C ABI cross ranks: the feature records
after detect+describe and the accepted pair records (H + inliers) that feed global alignment.  value = the survey's
pairs / max-over-ranks time.  --scaling weak keeps an independent strip per rank (the result all-gather only).

`python bench.py --gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset) re-executes itself under
`python -m torch.distributed.run --nproc-per-node N` on 127.0.0.1, so the plain command form measures N ranks too.
The line carries `transport` and `rccl_ranks` (ncclCommCount of the C ABI's communicator); with the default transport a
rank that cannot create that communicator fails the run instead of falling back.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times --steps steps and prints the headline line (metric, value, unit, higher_is_better, dtype,
ms_per_step, the configuration).  --full adds everything else the line has carried: kernel events in the timed region, the
untimed phase step, the exclusive passes and rooflines, quality against the ground truth, the CPU baseline with its parity
sample and the host-frame sample.  --dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy
(dump_outputs); the inputs are synthetic and seeded, the same on every run with the same arguments.
"""
import argparse
import ctypes
import gc
import json
import math
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DOM = "gauss_stream"       # profile class of the dominant kernel (blur16_stream): the only launches bracketed with events in the timed region
SLOTS = int(os.environ.get("MI355_BENCH_SLOTS", "3"))   # batch work areas in flight (library default 3)
BATCH = int(os.environ.get("MI355_BENCH_BATCH", "0"))   # frames per batch; 0 = chosen in main(): 32 (library default 16) unless the survey needs the HBM (C5, --blend)
PMC_JSON = "r06_pmc_blur16_stream.json"   # committed rocprofv3 --pmc passes of this command (profiles/pmc_traffic.py)
HBM_PEAK_GBS = 8000.0      # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md (6.29 TB/s measured copy)
VALU_PEAK_TOPS = 78.65     # f32 vector multiplies OR adds per second (T lane-operations/s): the 157.3 TFLOP/s vector peak counts an fma as two


def streamed_lane_ops(w, h):
    """f32 lane-operations (separately rounded products and sums, oracle_sift.c gauss_blur16) of the levels of ONE w x h frame that go
    through blur16_stream: per output pixel of a level with radius R the row pass is 2R+1 products + 2R sums, the column pass R+1
    products + 2R sums (pairs) = 7R + 2.  Same level selection as sift.hip blur_streams(): >= 512 columns, width a multiple of 4."""
    radii = {0: 6, 1: 5, 2: 6, 3: 8, 4: 10, 5: 13}          # base level sigma sqrt(1.6^2 - 0.5^2), then the five incremental blurs
    total, o = 0.0, 0
    while (w >> o) >= 12 and (h >> o) >= 12:
        ow, oh = w >> o, h >> o
        if ow >= 512 and oh >= 64 and ow % 4 == 0 and ((ow & 255) == 0 or (ow & 255) > 16):
            for lv, R in radii.items():
                if lv == 0 and o > 0:
                    continue
                total += float(ow) * oh * (7 * R + 2)
        o += 1
    return total


# Separately rounded f32 operations (one lane-operation each: a multiply, an add / subtract, a division, a square root, a compare) that
# Ransac2D's definition requires for ONE draw, counted from the operation plan of csrc/hmath.h (the structural zeros of the 4-point systems
# are not operated on, exactly like the reference's InverseMatrix skips them):
#   J^T J of the 8 x 8 pattern matrix        120 products + 93 sums (27 distinct entries)                                   = 213
#   its inverse (Gauss-Jordan, planned)      46 divisions + 176 multiply-adds (2 each) + 56 first values                   = 454
#   (J^T J)^-1 J^T                           320 products + 256 sums                                                       = 576
#   times the right-hand side                64 products + 56 sums                                                         = 120
#   4-point solve  = 16 (design matrix) + 213 + 454 + 576 + 120 + 84 (residual of the 4 points: apply 15 + distance 6 each) = 1463
#   Gauss-Newton step (LeastSquare.h:353-531 on 4 points) = 112 (Jacobian + residuals: 9 divisions, 11 products, 8 sums per point)
#                                                   + 213 + 454 + 576 + 120 + 16 (update, stop test)                        = 1491
#   support of a hypothesis, per correspondence: ApplyProjectMat (4 + 4 + 4 ops, 1 reciprocal, 2 products), 2 differences, 2 squares, sum, compare = 21
RANSAC_SOLVE_OPS, RANSAC_GN_STEP_OPS, RANSAC_SUPPORT_OPS = 1463, 1491, 21


def ransac_lane_ops(n, sample_times=1000, polished_fraction=0.98, gn_steps=15, classified_per_listed=1.1):
    """lane-operations of ONE pair with n correspondences (n >= 4): the classification pass (4-point solve of the draws looked at until
    `sample_times` hold a hypothesis slot, ~1.1 per listed draw), then per listed draw the solve again, the polish of the draws whose first
    residual lies in (0.01, 5) (98 % on survey data: profiles/r05_ransac_time.txt, 979.7 of 1000; always all 15 steps -- the 1e-10 stop rule is
    never met in f32) and the support count over the n correspondences.  The closing refinement on the inliers (accepted pairs only, 3 % at C4) is left out."""
    if n < 4:
        return 0.0
    return sample_times * (classified_per_listed * RANSAC_SOLVE_OPS + RANSAC_SOLVE_OPS + polished_fraction * gn_steps * RANSAC_GN_STEP_OPS + n * RANSAC_SUPPORT_OPS)


def batch_for(frames_of_rank, big):
    """frames per SIFT batch: 32 when the rank's frames fill three batches of 32 (the latency-bound launches of the small octaves and the
    per-frame selections are then paid once per 32 frames; 3 x 32 frames in flight = 86 GB of work areas at 12 MP), otherwise a third of
    the rank's frames so that all three batch work areas are in flight (a rank of an 8-rank C3 / C4 run owns 62-63 frames: two batches
    of 32 leave a slot idle -- 21.0 instead of 21.9 ms per step for the rank's share); surveys that need the HBM themselves keep 16."""
    if big:
        return 16
    if frames_of_rank >= 3 * 32:
        return 32
    return max(8, min(32, -(-frames_of_rank // SLOTS)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=500, help="frames per rank (C3: 500)")
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--window", type=int, default=2, help="pair window: j in (i, i+window); 2 = adjacent pairs (C3), 182 = reference window (C4)")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="N>1: strong = ONE survey of --frames frames, detect+describe / pairs / canvas stripes sharded over the ranks with the two RCCL "
                         "all-gathers (features, pair records); weak = an independent --frames strip per rank")
    ap.add_argument("--transport", choices=["rccl", "torch"], default=None,
                    help="exchange transport: rccl = the C ABI's own ncclAllGather calls (default with backend nccl), torch = torch.distributed (gloo dry runs)")
    ap.add_argument("--layout", choices=["strip", "block"], default="strip",
                    help="strip = serpentine survey, 60 %% forward / 30 %% side overlap (SURVEY 8d; C3 / C4); block = the frames piled onto a ~20000 x 20000 canvas (C5's canvas)")
    ap.add_argument("--blend", action="store_true",
                    help="after the timed steps also render the survey with LaplacianPyramidBlending (mi355_mosaic_blended_dev: frames, chips, masks and the blender's "
                         "pyramids co-resident in HBM) and report its time and the resident memory; not part of `value` (the metric's warp is the last-write-wins canvas)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--profile-all", action="store_true", help="bracket every kernel class with events (extra JSON field)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for single-GPU dry runs of the N>1 path)")
    ap.add_argument("--all-ranks-on-device0", action="store_true", help="dry run of the N>1 path on a 1-GPU box (use with --backend gloo)")
    ap.add_argument("--frames-resident", default="owned", choices=["owned", "replicas"],
                    help="strong scaling with N > 1: owned = a rank synthesises and holds only the frames it extracts (k mod N) and receives the frames its canvas stripe reads "
                         "from their owners inside the timed step (mi355_exchange_frames: SURVEY 8e's primary form); replicas = every rank holds all frames (no exchange)")
    ap.add_argument("--frame-owner", default="blocks", choices=["blocks", "mod"],
                    help="which rank extracts and holds frame k (strong scaling): blocks = contiguous runs of ceil(F/N) frames (a rank's frames lie in one band of the canvas, its stripe is dealt "
                         "out to match: the frame exchange moves the bands' edges only); mod = k mod N, the reference's thread rule (MosaicWithoutPos.cpp:4861). Pairs stay i mod N either way")
    ap.add_argument("--no-host-frames", action="store_true", help="skip the untimed host-frame sample (frames in pageable host memory through mi355_sift_extract / mi355_mosaic_refined)")
    ap.add_argument("--align-input", default="auto", choices=["auto", "records", "moments"], help="auto = records on one GPU, and with N > 1 (strong) the moments on every rank + the records to rank 0's host only (mi355_allgather_results root = 0, the rank that would run the unchanged driver). What the host alignment starts from: the accepted pair records (9664 B each) or their second moments formed on the device (mi355_allgather_moments / mi355_pair_moments_dev, 184 B each; same transforms bit for bit)")
    ap.add_argument("--as-rank", default=None, help="ONE-GPU PROXY of a rank's share of an --of G rank run (no launcher, no other rank): comma list of ranks, e.g. 0,7")
    ap.add_argument("--of", type=int, default=8, help="rank count the --as-rank proxy pretends to be part of")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: kernel events in the timed region, the untimed phase step, the exclusive passes and "
                         "rooflines, quality against the ground truth, the CPU baseline with its parity sample and the host-frame sample. "
                         "Without it a run sets up, warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step computed (rank 0) as DIR/<name>.npy, float32 / float64, < 64 MB in all")
    return ap.parse_args()


from tests.synth_survey import frame_layout, block_layout, affine3  # noqa: E402  (ground-truth geometry shared with tests/test_gpu_configs.py)


def cpu_has_v3():
    try:
        flags = open("/proc/cpuinfo").read()
        return all(f in flags for f in (" avx2", " fma", " bmi2"))
    except OSError:
        return False


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_run(frames_host, A, w, h, ws, T, lib):
    """One pass of the oracle pipeline over the sample on T host threads, image-strided in two barrier phases like the
    reference (MosaicWithoutPos.cpp:5246-5247 T = min(8, ncpu-1); :4861 / :5066 thread k takes images k mod T):
    phase A SIFT of every frame, phase B per frame i: match + select + Ransac2D of pair (i, i+1) and the warp of frame i."""
    from tests import oracle_lib as ol
    n = len(frames_host)
    orcs = [ol.Oracle(os.path.join(ROOT, "oracle", lib)) for _ in range(T)]
    feats = [None] * n
    done = [None] * n

    def phase_a(t):
        for k in range(t, n, T):
            img = frames_host[k].reshape(h, ws)[:, :3 * w].reshape(h, w, 3)
            feats[k] = orcs[t].sift(np.ascontiguousarray(img))

    def phase_b(t):
        for k in range(t, n, T):
            if k + 1 < n:
                (k0, d0), (k1, d1) = feats[k], feats[k + 1]
                done[k] = orcs[t].match_pair(np.stack([k0["x"], k0["y"]], 1), d0, np.stack([k1["x"], k1["y"]], 1), d1, w, h, 2.5, 1)
            img = np.ascontiguousarray(frames_host[k].reshape(h, ws)[:, :3 * w].reshape(h, w, 3))
            Hk = np.linalg.inv(affine3(A[0])) @ affine3(A[k])
            orcs[t].image_projection_transform(img, Hk.reshape(9).astype(np.float32))

    t0 = time.perf_counter()
    for fn in (phase_a, phase_b):
        th = [threading.Thread(target=fn, args=(t,)) for t in range(T)]
        [t.start() for t in th]
        [t.join() for t in th]
    return time.perf_counter() - t0, [d for d in done if d is not None]


def cpu_baseline(frames_host, A, w, h, ws):
    """The oracle (CPU port of the same pipeline) on the GPU box's host cores: (i) T = min(8, nproc-1)
    threads over the 20-frame / 19-adjacent-pair subset, (ii) 1 thread over its first 4 frames / 3 pairs (a 1-thread pass
    over all 20 would take ~2 min).  `value` is (i), the reference's own threading rule."""
    from tests import oracle_lib as ol
    ol.build_oracle()
    lib = "liboracle_v3.so" if cpu_has_v3() and os.path.exists(os.path.join(ROOT, "oracle", "liboracle_v3.so")) else "liboracle.so"
    nproc = os.cpu_count() or 2
    T = max(1, min(8, nproc - 1))
    n = len(frames_host)
    dt, done = cpu_run(frames_host, A, w, h, ws, T, lib)
    pairs = max(n - 1, 1)
    n1 = min(4, n)
    dt1, _ = cpu_run(frames_host[:n1], A, w, h, ws, 1, lib)
    out = {"value": pairs / dt, "unit": "image-pairs/s", "cores": T, "kind": "port", "nproc": nproc, "cpu_model": cpu_model(),
           "sample": "%d frames %dx%d / %d adjacent pairs of the same synthetic workload (BASELINE.md section 2 subset), %d threads image-strided in two phases like the reference, oracle/%s, %.1f s"
                     % (n, w, h, pairs, T, lib, dt),
           "one_thread": {"value": max(n1 - 1, 1) / dt1, "unit": "image-pairs/s", "cores": 1,
                          "sample": "first %d frames / %d pairs of the same subset, 1 thread, %.1f s" % (n1, max(n1 - 1, 1), dt1)},
           "inliers": [int(d[0]) for d in done]}
    return out, done


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run ... bench.py <same args>`"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush(); sys.stderr.flush()
    os.execv(sys.executable, cmd)


def rank_share_proxy(args):
    """`python bench.py --as-rank 0,7 --of 8 [--window 182]`: what ONE rank of a G-rank strong-scaling run does, measured on one GPU.

    A PROXY, not a scaling curve (no multi-GPU box was available to this build).  Rank r of G extracts the frames k mod G == r, passes the feature
    exchange (world-1 RCCL: the same pack / ncclAllGather / install calls with its share as payload), matches the pairs i mod G == r, takes part
    in the result exchange, runs the replicated host alignment on the WHOLE survey's moments (or records), obtains the frames its canvas stripe
    reads and renders stripe r.  The other ranks' features / records / moments come from one untimed single-GPU pass over the whole survey.

    Accounting (VERDICT r05 weak #5, next #2b / #3):
      * the one-GPU denominator is the PLAIN single-GPU step (device compaction, pinned copy of the accepted records, alignment from them):
        bench.py's own world-1 path, not a path through the exchange;
      * every byte a rank's host RECEIVES is copied in the timed share: all ranks' moments; on the root (rank 0) also ALL ranks' records,
        enqueued like the N-rank step does (the copy runs beside the host alignment); with --align-input records every rank copies all
        ranks' records (the round-5 default, kept for comparison);
      * what one GPU cannot measure is wire time: the xGMI time of the other ranks' feature records, moments, records (to the root) and of the
        frames the stripe reads from their owners.  It is added from the link model of SURVEY section 5 and printed apart, bytes stated."""
    import imagemosaicing_amd as im
    from imagemosaicing_amd import dist as md
    G = args.of
    ranks = [int(x) for x in str(args.as_rank).split(",")]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    global BATCH
    batch_one = BATCH if BATCH > 0 else batch_for(args.frames, args.frames * args.width * args.height > 1000 * 4000 * 3000)
    if BATCH <= 0:
        BATCH = batch_for(-(-args.frames // G), args.frames * args.width * args.height > 1000 * 4000 * 3000)
    ctx = im.Context(0)
    ctx.set_option("sift_slots", SLOTS)
    ctx.set_option("sift_batch", batch_one)                       # the one-GPU reference pass runs with the one-GPU batch size
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    w, h, F = args.width, args.height, args.frames
    ws = (3 * w + 3) & ~3
    A, gains = frame_layout(F, w, h, 0)
    if args.layout == "block":
        A = block_layout(F, w, h, seed=5)
    frames = torch.empty((F, h * ws), dtype=torch.uint8, device=dev)
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), w, h, ws, A[k], 0xC0FFEE, k & 0xffffffff, gains[k], 2.0)
    ctx.synchronize()
    fptr = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [w] * F, [h] * F, [ws] * F
    all_pairs = im.pair_schedule(F, args.window)
    survey_pairs = len(all_pairs)
    REC, MOM = im.PAIR_RESULT.itemsize, im.PAIR_MOMENTS.itemsize
    results = torch.zeros((survey_pairs, REC), dtype=torch.uint8, device=dev)
    compact = torch.zeros((survey_pairs, REC), dtype=torch.uint8, device=dev)
    res_host = torch.empty((survey_pairs, REC), dtype=torch.uint8).pin_memory()
    Hgt = np.stack([(np.linalg.inv(affine3(A[0])) @ affine3(A[k])).reshape(9) for k in range(F)]).astype(np.float32)
    gw, gh, gws, _ = im.mosaic_layout(wv, hv, Hgt)
    canvas_cap = int(1.2 * gws * gh) + (64 << 20)
    canvas = torch.empty(canvas_cap, dtype=torch.uint8, device=dev)
    ex = md.Exchange(ctx, "rccl", strict=True)                    # a communicator of one rank: the same calls as in the N-rank run

    mode = args.align_input
    if mode == "auto":
        mode = "moments"                                          # the N > 1 default of bench.py: moments everywhere + records to rank 0
    use_mom = mode == "moments"

    def align_and_layout(r, mom):
        if mom:
            label = im.select_connected_moments(r, F) if len(r) else np.zeros(F, np.int32)
        else:
            label = im.select_connected_results(r, F) if len(r) else np.zeros(F, np.int32)
        label[0] = 1
        fixed_k = [1 if (k == 0 or label[k] == 0) else 0 for k in range(F)]
        T = im.global_affine_align_moments(r, F, fixed=fixed_k, label=label) if mom else im.global_affine_align_results(r, F, fixed=fixed_k, label=label)
        h9 = T["m"].copy()
        h9[label == 0, 8] = 0.0
        cw, ch, cws, _ = im.mosaic_layout(wv, hv, h9)
        return h9, cw, ch, cws

    def full_step(seed):
        """bench.py's single-GPU step (main(): world == 1, --align-input records): the denominator"""
        for k in range(F):
            ctx.SiftExtractDev(k, fptr[k], w, h, ws)
        ctx.MatchPairsDev(all_pairs, results.data_ptr(), 2.5, seed)
        k_acc = ctx.CompactAcceptedDev(results.data_ptr(), survey_pairs, compact.data_ptr())
        if k_acc:
            res_host[:k_acc].copy_(compact[:k_acc], non_blocking=True)
        stream.synchronize()
        r = res_host.numpy().view(im.PAIR_RESULT).reshape(-1)[:k_acc]
        h9, cw, ch, cws = align_and_layout(r, False)
        ctx.MosaicImagesRefinedDev(fptr, wv, hv, wsv, h9, canvas.data_ptr(), cw, ch, cws)
        return r

    def timed(fn, n):
        gc.collect(); gc.disable()  # (a generation-2 collection of the interpreter paused one step of the second rank measured for ~60 ms, whichever rank that was)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        marks = []
        for i in range(n):
            fn(100 + i)
            marks.append(time.perf_counter())
        ctx.synchronize(); torch.cuda.synchronize()
        t1 = time.perf_counter()
        gc.enable()
        if (os.environ.get("MI355_PROXY_STEPS") or os.environ.get("MI355_PROXY_MARKS")) and n > 1:
            print("[proxy] host returns from the steps at (ms): %s, all done at %.2f" % ([round((m - t0) * 1e3, 2) for m in marks], (t1 - t0) * 1e3), file=sys.stderr, flush=True)
        return (t1 - t0) / n * 1e3

    for i in range(max(args.warmup, 1)):
        full_step(1 + i)
    t_one = timed(full_step, max(args.steps, 1))
    r_all = full_step(7).copy()                                   # every frame's features + the survey's accepted records now resident
    ctx.synchronize()
    acc = int(len(r_all))
    # the whole survey's accepted records and moments, resident: what the other ranks would have sent (their device-to-host leg is timed below)
    all_acc_dev = compact[:max(acc, 1)]
    mom_all_dev = torch.zeros((max(acc, 1), MOM), dtype=torch.uint8, device=dev)
    if acc:
        ctx.PairMomentsDev(all_acc_dev.data_ptr(), acc, mom_all_dev.data_ptr())
    ctx.synchronize()
    mom_all = mom_all_dev[:acc].cpu().numpy().reshape(-1).view(im.PAIR_MOMENTS)
    mom_all = mom_all[np.lexsort((mom_all["j"], mom_all["i"]))]
    mom_host = torch.empty((max(acc, 1), MOM), dtype=torch.uint8).pin_memory()
    ctx.set_option("sift_batch", BATCH)                           # a rank's own batch size (batch_for)
    shares = {}
    owner = md.frame_owner(F, G, args.frame_owner)
    for rk in ranks:
        own = md.owned_frames(F, rk, G, args.frame_owner)
        pairs = im.pair_schedule(F, args.window, rk, G)
        res_r = torch.zeros((max(len(pairs), 1), REC), dtype=torch.uint8, device=dev)
        comp_r = torch.zeros((max(len(pairs), 1), REC), dtype=torch.uint8, device=dev)
        ph, xinfo = {}, {}

        def share_step(seed, sync=False):
            t = [time.perf_counter()]

            def mark():
                if sync:
                    ctx.synchronize(); t.append(time.perf_counter())
            for k in own:
                ctx.SiftExtractDev(k, fptr[k], w, h, ws)
            mark()
            ex.allgather_features(own, len(own), dev)             # pack + ncclAllGather + install of this rank's records
            mark()
            ctx.MatchPairsDev(pairs, res_r.data_ptr(), 2.5, seed)
            mark()
            if use_mom:
                # this rank's share through the real call (compaction, moments, count + payload all-gathers, copy of ITS moments to the pinned buffer) ...
                m_own = ex.allgather_moments(res_r, len(pairs), copy=False)
                # ... and the copy of the OTHER ranks' moments a real run receives
                n_other = max(acc - len(m_own), 0)
                if n_other:
                    mom_host[:n_other].copy_(mom_all_dev[:n_other], non_blocking=True)
                    stream.synchronize()
                if rk == 0:
                    # the root: ALL ranks' records to its pinned host buffer (1.1 GB at C5), enqueued -- the copy runs beside the alignment below
                    ex.allgather_results(all_acc_dev, acc, accepted_only=False, root=0, copy=False, wait=False)
                else:
                    ctx.CompactAcceptedDev(res_r.data_ptr(), len(pairs), comp_r.data_ptr())      # a non-root rank compacts and ncclSends (wire: modelled)
            else:
                # round-5 form: ALL ranks' records to EVERY rank's host (the pinned buffer of the library), waited for
                ex.allgather_results(all_acc_dev, acc, accepted_only=False, root=-1, copy=False)
            mark()
            h9, cw, ch, cws = align_and_layout(mom_all if use_mom else r_all, use_mom)      # replicated on every rank: the whole survey
            mark()
            stripes = [((ch * q) // G, (ch * (q + 1)) // G - (ch * q) // G) for q in range(G)]
            sidx = md.stripe_of_ranks(wv, hv, h9, owner, G)
            row0, rows = stripes[int(sidx[rk])]
            if args.frames_resident == "replicas":
                ptrs = fptr                                        # round 5's form: every rank holds every frame, nothing to obtain
            else:
                # the rank's own cover row: the frames that give its stripe a pixel (the tile kernel's walk without loads) ...
                exact = md.exact_cover_pays(wv, hv, h9, cw, ch)
                need_mine = ctx.StripeCover(wv, hv, h9, row0, rows, exact=exact)
                # ... and the exchange call on the one-rank communicator: the all-gather of the cover rows and the table walk are real, the
                # transfers themselves are wire (modelled from the bytes below)
                ptrs, _, _ = ex.exchange_frames(fptr, hv, wsv, need_mine)
            mark()
            ctx.MosaicImagesRefinedDev(ptrs, wv, hv, wsv, h9, canvas.data_ptr(), cw, ch, cws, row0, rows)
            mark()
            if sync:
                names = ["detect_describe", "feature_allgather_local", "match_select_ransac", "result_exchange_local_and_d2h", "host_alignment_replicated", "stripe_cover_and_exchange_call", "warp_stripe"]
                ph.update({n: (t[i + 1] - t[i]) * 1e3 for i, n in enumerate(names)})
                fb = float(h * ws)
                exact = md.exact_cover_pays(wv, hv, h9, cw, ch)
                need = np.stack([ctx.StripeCover(wv, hv, h9, stripes[int(sidx[q])][0], stripes[int(sidx[q])][1], exact=exact) for q in range(G)])      # every rank's row (untimed: a rank forms its own)
                box = ctx.StripeCover(wv, hv, h9, row0, rows)
                if args.frames_resident == "replicas":
                    need = need * 0                                # nothing crosses ranks: the bytes below are zero
                xinfo.update({"stripe": int(sidx[rk]), "frames_read_by_the_stripe": int(need[rk].sum()), "frames_whose_box_meets_the_stripe": int(box.sum()),
                              "frames_received": int(sum(1 for k in range(F) if need[rk, k] and owner[k] != rk)),
                              "bytes_received": fb * sum(1 for k in range(F) if need[rk, k] and owner[k] != rk),
                              "bytes_sent": fb * sum(int(need[q, k]) for q in range(G) for k in own if q != rk), "owner_rule": args.frame_owner,
                              "cover": "exact (device pass)" if exact else "by box (host geometry: the survey is thin, an exact list would cost more than the few frames it saves)"})

        for i in range(max(args.warmup, 1)):
            share_step(1 + i)
        t_r = timed(share_step, max(args.steps, 1))
        step_ms = []
        if os.environ.get("MI355_PROXY_STEPS"):                 # diagnostic: every step on its own, synchronised at its end
            for i in range(max(args.steps, 1)):
                step_ms.append(round(timed(share_step, 1), 2))
            print("[proxy] rank %d steps one by one: %s" % (rk, step_ms), file=sys.stderr, flush=True)
        share_step(999, sync=True)
        shares[str(rk)] = {"ms_per_step": t_r, "frames": len(own), "pairs": int(len(pairs)), "batches": -(-len(own) // BATCH), "phase_ms_synchronised": dict(ph), "frame_exchange": dict(xinfo)}
    blend = None
    if args.blend:
        # the default compositing path (LaplacianPyramidBlending) as the ranks would share it: the whole canvas on one GPU against a rank's stripe
        h9b, _, _, _ = align_and_layout(mom_all if use_mom else r_all, use_mom)
        keep = im.resample_by_overlap(wv, hv, h9b, 0.7)
        bw_, bh_, _ = im.blend_layout(wv, hv, h9b, keep)

        def blend_ms(row0, rows):
            ts = []
            for rep in range(3):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                o, _, _, _ = ctx.MosaicBlendedDev(fptr, wv, hv, wsv, h9b, keep=keep, band=5, row0=row0, rows=rows)
                ctx.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
                del o
            return min(ts[1:])
        whole = blend_ms(0, -1)
        bstripes = [((bh_ * q) // G, (bh_ * (q + 1)) // G - (bh_ * q) // G) for q in range(G)]
        bsidx = md.stripe_of_ranks(wv, hv, h9b, owner, G)
        stripes_ms, bx = {}, {}
        for rk in ranks:
            b0, bn = bstripes[int(bsidx[rk])]
            bneed = ctx.StripeCover(wv, hv, h9b, b0, bn, blended=True, keep=keep, band=5)
            stripes_ms[str(rk)] = blend_ms(b0, bn)
            bx[str(rk)] = {"frames_read_by_the_stripe": int(bneed.sum()), "bytes_received": float(h * ws) * sum(1 for k in range(F) if bneed[k] and owner[k] != rk)}
        blend = {"canvas": [bw_, bh_], "chips": int(keep.sum()), "bands": 5, "whole_canvas_ms_one_gpu": whole, "stripe_ms": stripes_ms, "frame_exchange": bx,
                 "wire_ms_frames_direct_7_links": {q: v["bytes_received"] / (7 * 153e9) * 1e3 for q, v in bx.items()},
                 "speedup_of_the_slowest_stripe": whole / max(stripes_ms.values()),
                 "speedup_with_the_frames_wire_time": whole / max(stripes_ms[q] + bx[q]["bytes_received"] / (7 * 153e9) * 1e3 for q in stripes_ms),
                 "note": "mi355_mosaic_blended_rows_dev: a rank forms the chips that reach its rows (+ the pyramids' reach), their ownership there and the rows of every blender level its output depends on; "
                         "the frames of those chips it does not hold come from their owners (mi355_exchange_frames; bytes stated, wire time modelled)"}
    feat_bytes = F * 319488 * (G - 1) / G                          # feature records a rank RECEIVES (2048 x (28 + 128) B per frame)
    mom_bytes = acc * MOM * (G - 1) / G if use_mom else 0.0
    rec_bytes_root = acc * REC * (G - 1) / G                       # records the ROOT receives (moments mode), or every rank (records mode)
    link = 153e9
    per_rank = {}
    for q, v in shares.items():
        fx = v["frame_exchange"]
        recs = rec_bytes_root if (not use_mom or int(q) == 0) else 0.0
        ring = (feat_bytes + mom_bytes + (recs if not use_mom else 0.0)) / link * 1e3            # all-gathers: ring, bound by one link
        direct = ((recs if use_mom else 0.0) + fx["bytes_received"]) / (7 * link) * 1e3           # ncclSend / ncclRecv from 7 different peers: the 7 links side by side
        per_rank[q] = {"allgather_ring_one_link_ms": ring, "send_recv_direct_7_links_ms": direct,
                       "bytes_received": {"features": feat_bytes, "moments": mom_bytes, "records": recs, "frames": fx["bytes_received"]},
                       "bytes_sent_frames": fx["bytes_sent"], "predicted_ms_per_step": v["ms_per_step"] + ring + direct}
    t_pred = max(v["predicted_ms_per_step"] for v in per_rank.values())
    out = {"kind": "rank_share_proxy (ONE GPU; a proxy of a rank's share, NOT a measured scaling curve)",
           "metric": "image-pairs/sec (detect+match+H+warp), 4000x3000 UAV frames", "of_ranks": G, "ranks_run": ranks,
           "workload": "%d frames %dx%d, pair window %d (%d pairs), strong scaling: frames %s, pairs i mod %d, canvas stripes; %s" % (F, w, h, args.window, survey_pairs, ("in %d blocks" % G) if args.frame_owner == "blocks" else ("k mod %d" % G), G, "every frame on every rank (replicas)" if args.frames_resident == "replicas" else "frames held by their owners only"),
           "one_gpu_ms_per_step": t_one, "one_gpu_pairs_per_s": survey_pairs / t_one * 1e3,
           "one_gpu_path": "bench.py's plain single-GPU step (device compaction, pinned copy of the accepted records, alignment from the records): not a path through the exchange",
           "frames_per_batch": {"one_gpu": batch_one, "rank": BATCH},
           "share": shares, "accepted_records": acc, "align_input": mode,
           "result_exchange": ("moments to every rank (all ranks' %d x %d B copied to the host in the share) + records to rank 0 only (all ranks' %d x %d B = %.2f GB copied to rank 0's pinned buffer in its share, enqueued beside the alignment)" % (acc, MOM, acc, REC, acc * REC / 1e9))
                              if use_mom else ("records of ALL ranks to EVERY rank's pinned host buffer (%d x %d B = %.2f GB copied in the share, waited for)" % (acc, REC, acc * REC / 1e9)),
           "wire_model": {"link_GBs": 153.0, "per_rank": per_rank,
                          "note": "not measurable on one GPU: xGMI time of what the OTHER ranks send; all-gathers as a ring bound by one 153 GB/s link, ncclSend / ncclRecv from distinct peers over the 7 links side by side (SURVEY section 5)"},
           "predicted_ms_per_step": t_pred,
           "predicted_pairs_per_s": survey_pairs / t_pred * 1e3,
           "predicted_speedup_over_one_gpu": t_one / t_pred,
           "blend": blend,
           "note": "max over the ranks run of (measured share + wire model); assumes the slowest of the ranks run is the slowest rank (rank 0 owns ceil(F/G) frames, is the records' root "
                   "and renders the first stripe; rank G-1 the last)"}
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(out), flush=True)
    ex.close()
    ctx.set_stream(None)
    ctx.close()


DUMP_SEED = 20240607       # fixed samples of --dump-outputs: the same positions on every run with the same arguments
DUMP_PAIRS = 1 << 17       # pair records written whole up to this many scheduled pairs, a fixed sample of as many beyond
DUMP_INLIER_PAIRS = 1024   # pairs whose inlier lists are written (all of them up to this many, a fixed sample beyond)
DUMP_PIXELS = 1 << 20      # canvas pixels sampled for canvas_sample.npy
DUMP_CAP = 64 << 20        # bytes of all dumped arrays together


def dump_outputs(d, results, n_pairs, h9, canvas, cw, ch, cws, rows):
    """--dump-outputs: what the last timed step handed its caller, as float32 / float64 .npy files in d.
      pairs.npy           (P, 6) i, j, ok, accepted, n_selected, n_in of every scheduled pair (or of a fixed sample of DUMP_PAIRS)
      pairs_H.npy         (P, 9) the homography of the same pairs where accepted, 0 elsewhere
      pairs_inliers.npy   (Q, 2, 400, 3) x, y, keypoint id of the inlier lists a / b of up to DUMP_INLIER_PAIRS of those pairs, 0 past n_in
      transforms.npy      (F, 9) what the warp used (m8 = 0: image left out)
      canvas_size.npy     cw, ch, first row, rows rendered by this rank
      canvas_row_sums.npy / canvas_col_sums.npy   byte sums of every rendered canvas row / of every byte column over those rows
      canvas_sample.npy   (N, 3) B, G, R of a fixed sample of DUMP_PIXELS rendered canvas pixels"""
    import imagemosaicing_amd as im
    rng = np.random.default_rng(DUMP_SEED)
    dev = results.device
    pick = np.arange(n_pairs) if n_pairs <= DUMP_PAIRS else np.sort(rng.choice(n_pairs, DUMP_PAIRS, replace=False))
    res = results[torch.from_numpy(pick).to(dev)].cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
    acc = res["accepted"] != 0
    out = {"pairs": np.stack([res[f].astype(np.float32) for f in ("i", "j", "ok", "accepted", "n_selected", "n_in")], 1),
           "pairs_H": np.where(acc[:, None], res["H"], np.float32(0)).astype(np.float32)}
    q = np.arange(len(res)) if len(res) <= DUMP_INLIER_PAIRS else np.sort(rng.choice(len(res), DUMP_INLIER_PAIRS, replace=False))
    inl = np.zeros((len(q), 2, 400, 3), np.float32)
    for s, side in enumerate(("a", "b")):
        pts = res[side][q]
        inl[:, s] = np.stack([pts["x"], pts["y"], pts["id"].astype(np.float32)], 2)
    live = acc[q, None] & (np.arange(400)[None, :] < res["n_in"][q, None])
    out["pairs_inliers"] = np.where(live[:, None, :, None], inl, np.float32(0))
    out["transforms"] = np.ascontiguousarray(h9, np.float32)
    row0, nrows = rows
    out["canvas_size"] = np.array([cw, ch, row0, nrows], np.float64)
    region = canvas[row0 * cws:(row0 + nrows) * cws].view(nrows, cws)[:, :3 * cw]
    row_sums, col_sums = [], torch.zeros(3 * cw, dtype=torch.float64, device=dev)
    for r in range(0, nrows, 256):
        chunk = region[r:r + 256].to(torch.float64)
        row_sums.append(chunk.sum(1))
        col_sums += chunk.sum(0)
    out["canvas_row_sums"] = torch.cat(row_sums).cpu().numpy() if row_sums else np.zeros(0)
    out["canvas_col_sums"] = col_sums.cpu().numpy()
    npix = nrows * cw
    px = np.arange(npix) if npix <= DUMP_PIXELS else np.sort(rng.integers(0, npix, DUMP_PIXELS))
    offs = torch.from_numpy((px // cw) * cws + 3 * (px % cw)).to(dev)
    flat = canvas[row0 * cws:(row0 + nrows) * cws]
    out["canvas_sample"] = torch.stack([flat[offs + c] for c in range(3)], 1).to(torch.float32).cpu().numpy()
    total = sum(a.nbytes for a in out.values())
    assert total <= DUMP_CAP, "outputs of %d bytes exceed the dump's cap" % total
    os.makedirs(d, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(d, name + ".npy"), a)


def main():
    args = parse()
    if args.as_rank is not None:
        if args.dump_outputs:
            raise SystemExit("--dump-outputs writes the outputs of the main path, not of the --as-rank proxy")
        return rank_share_proxy(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(args.gpus, 1):
        raise SystemExit("WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus))
    if args.all_ranks_on_device0:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    global BATCH
    if BATCH <= 0:
        # 32 frames per batch: the latency-bound launches of the small octaves and the per-frame selections are paid once per 32 frames
        # (3 x 32 frames in flight = 86 GB of work areas at 12 MP); surveys that need the HBM themselves keep the library's 16
        per_rank = -(-args.frames // world) if (world > 1 and args.scaling == "strong") else args.frames
        BATCH = batch_for(per_rank, args.blend or args.frames * args.width * args.height > 1000 * 4000 * 3000)
    import imagemosaicing_amd as im
    from imagemosaicing_amd import dist as md
    ctx = im.Context(local_rank)
    ctx.set_option("sift_slots", SLOTS)
    ctx.set_option("sift_batch", BATCH)
    # One explicit stream for everything (HIP kernels of the library, torch copies, RCCL): torch's default stream
    # is the NULL stream, which the library's set_stream treats as "use the ctx-owned stream".
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0
    ctx.set_stream(stream.cuda_stream)

    w, h, F = args.width, args.height, args.frames
    ws = (3 * w + 3) & ~3
    strong = args.scaling == "strong"
    exchange = world > 1 or bool(os.environ.get("MI355_BENCH_FORCE_EXCHANGE"))      # the env switch runs the collectives on one rank (dry run of the calls)
    transport = args.transport or ("rccl" if (args.backend == "nccl" or world == 1) else "torch")
    ex = md.Exchange(ctx, transport, strict=True) if exchange else None      # no silent fallback: rccl means the C ABI's communicator or an error
    rccl_ranks = ex.rccl_ranks if ex is not None else None
    # strong: ONE survey, the same F frames on every rank (replicated in HBM: a rank renders every frame that crosses its canvas
    # stripe, SURVEY 8e "replicas of frames + stripes"), detect+describe and pairs sharded; weak: an independent strip per rank
    lay_rank = 0 if strong else rank
    A, gains = frame_layout(F, w, h, lay_rank)
    if args.layout == "block":
        A = block_layout(F, w, h, seed=5 + lay_rank)
    # ---- synthetic frames, generated straight into HBM (never timed) ----
    # strong scaling, N > 1: a rank synthesises (= "uploads") and holds ONLY the frames it extracts; the frames its canvas stripe reads arrive
    # from their owners inside the timed step (--frames-resident owned, the default).  Every rank holding all N frames would be 8 x the PCIe
    # upload in a deployment and 72 GB per GPU at C5 (VERDICT r05 missing #2).
    transport_is_rccl = (args.transport or ("rccl" if (args.backend == "nccl" or world == 1) else "torch")) == "rccl"
    owned_only = strong and world > 1 and args.frames_resident == "owned"
    owner = md.frame_owner(F, world, args.frame_owner)
    hold = md.owned_frames(F, rank, world, args.frame_owner) if owned_only else list(range(F))
    slot_of = {k: i for i, k in enumerate(hold)}
    frames = torch.empty((len(hold), h * ws), dtype=torch.uint8, device=dev)
    for k in hold:
        ctx.SynthFrameDev(frames[slot_of[k]].data_ptr(), w, h, ws, A[k], (0xC0FFEE + 977 * lay_rank) & 0xffffffff, (lay_rank * 1000003 + k) & 0xffffffff, gains[k], 2.0)
    ctx.synchronize()
    fptr = {k: frames[slot_of[k]].data_ptr() for k in hold}
    held = [frames[slot_of[k]] if k in slot_of else None for k in range(F)]
    if transport_is_rccl:
        held = [t.data_ptr() if t is not None else None for t in held]      # the C ABI takes addresses: no per-step walk over 2000 tensor objects
    if strong:
        own = md.owned_frames(F, rank, world, args.frame_owner)            # the frames this rank extracts (and, with --frames-resident owned, the only ones it holds)
        pairs = im.pair_schedule(F, args.window, rank, world)              # i mod G == rank (:5066), j in (i, i+window) (:5083)
        survey_pairs = len(im.pair_schedule(F, args.window))
        n_max_frames = (F + world - 1) // world
    else:
        own = list(range(F))
        pairs = im.pair_schedule(F, args.window)
        survey_pairs = len(pairs) * world
        n_max_frames = F
    n_pairs = len(pairs)
    results = torch.zeros((max(n_pairs, 1), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device=dev)
    res_host = torch.empty((max(n_pairs, 1), im.PAIR_RESULT.itemsize), dtype=torch.uint8).pin_memory()
    # canvas big enough for the ground-truth layout with margin (the step computes the real layout)
    Hgt = np.stack([(np.linalg.inv(affine3(A[0])) @ affine3(A[k])).reshape(9) for k in range(F)]).astype(np.float32)
    gw, gh, gws, _ = im.mosaic_layout([w] * F, [h] * F, Hgt)
    canvas_cap = int(1.2 * gws * gh) + (64 << 20)
    canvas = torch.empty(canvas_cap, dtype=torch.uint8, device=dev)
    wv, hv, wsv = [w] * F, [h] * F, [ws] * F
    state = {}

    phases = bool(os.environ.get("MI355_BENCH_PHASES"))     # also switched on for one untimed step after the timed region

    compact = torch.zeros((max(n_pairs, 1), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device=dev)

    def local_accepted():
        """this rank's accepted pair records on the host: compacted on the device first (what the reference appends to m_vecMatchPairs,
        MosaicWithoutPos.cpp:5201-5227) -- with the 182-frame window 97 % of the scheduled pairs are rejected and never cross PCIe"""
        k = ctx.CompactAcceptedDev(results.data_ptr(), n_pairs, compact.data_ptr())
        if k:
            res_host[:k].copy_(compact[:k], non_blocking=True)
        stream.synchronize()
        return res_host.numpy().view(im.PAIR_RESULT).reshape(-1)[:k]

    align_input = args.align_input
    if align_input == "auto":
        align_input = "moments" if (exchange and strong and world > 1) else "records"
    records_to_root = exchange and strong and align_input == "moments"      # the inlier lists still reach ONE host: rank 0, where the unchanged driver would run
    mom_dev = torch.zeros((max(n_pairs, 1), im.PAIR_MOMENTS.itemsize), dtype=torch.uint8, device=dev) if align_input == "moments" else None
    mom_host = torch.empty((max(n_pairs, 1), im.PAIR_MOMENTS.itemsize), dtype=torch.uint8).pin_memory() if align_input == "moments" else None

    def local_moments():
        """--align-input moments without an exchange: the accepted records are compacted on the device, their second moments formed there, 184 B per pair cross PCIe"""
        k = ctx.CompactAcceptedDev(results.data_ptr(), n_pairs, compact.data_ptr())
        if k:
            ctx.PairMomentsDev(compact.data_ptr(), k, mom_dev.data_ptr())
            mom_host[:k].copy_(mom_dev[:k], non_blocking=True)
        stream.synchronize()
        return mom_host.numpy().view(im.PAIR_MOMENTS).reshape(-1)[:k]

    def step(seed):
        nonlocal phases
        t0 = time.perf_counter()
        for k in own:
            ctx.SiftExtractDev(k, fptr[k], w, h, ws)
        if exchange and strong:
            # RCCL over xGMI: every rank receives every frame's keypoints + descriptors (the d:/feature_temp hand-off of the reference)
            ex.allgather_features(own, n_max_frames, dev)
        if phases:
            ctx.synchronize(); t1 = time.perf_counter()
        ctx.MatchPairsDev(pairs, results.data_ptr(), 2.5, seed)
        mom = None
        if align_input == "moments":
            # what the alignment needs of an accepted pair, formed on the device: 184 B instead of 9664 over xGMI and PCIe
            r = None
            if exchange:
                mom = ex.allgather_moments(results, n_pairs, copy=False)
                mom = mom[np.lexsort((mom["j"], mom["i"]))] if strong else local_moments()      # (the sort copies: 21 MB at C5) pair order independent of the rank count
                if records_to_root:
                    # ... and the records themselves to rank 0's host alone (ncclSend / ncclRecv into one pinned buffer; 1.1 GB at C5): enqueued,
                    # the copy runs while the host aligns; complete at the step's end (the timed region closes with a synchronisation)
                    r = ex.allgather_results(results, n_pairs, accepted_only=True, root=0, copy=False, wait=False)
            else:
                mom = local_moments()
        elif exchange:
            # RCCL over xGMI: H + inlier lists of every accepted pair of the survey, on every rank's host (pinned, the library's buffer)
            r = ex.allgather_results(results, n_pairs, accepted_only=True, copy=False)
            if strong:
                r = r[np.lexsort((r["j"], r["i"]))]      # pair order independent of the rank count
            else:
                # weak: the exchange is paid for, but every strip is its own survey -- this rank aligns and renders its own records
                r = local_accepted()
        else:
            r = local_accepted()
        if phases:
            t2 = time.perf_counter()
        # Select_Connected_Matched_Images + the global alignment straight from the pair records (the m_vecMatchPairs copy of the adaptor
        # path is 28 M correspondences = 1.1 GB at C5; same sums in the same order, tests/test_cabi.py)
        if mom is not None:
            label = im.select_connected_moments(mom, F) if len(mom) else np.zeros(F, np.int32)
        else:
            label = im.select_connected_results(r, F) if len(r) else np.zeros(F, np.int32)
        label[0] = 1
        ta = time.perf_counter()
        fixed_k = [1 if (k == 0 or label[k] == 0) else 0 for k in range(F)]
        T = im.global_affine_align_moments(mom, F, fixed=fixed_k, label=label) if mom is not None else im.global_affine_align_results(r, F, fixed=fixed_k, label=label)
        td = time.perf_counter()
        h9 = T["m"].copy()
        h9[label == 0, 8] = 0.0                                     # invalid images are skipped by the warp (MWP.cpp:4646-4652)
        cw, ch, cws, _ = im.mosaic_layout(wv, hv, h9)
        if phases:
            state["host_parts_ms"] = {"select_connected": (ta - t2) * 1e3, "global_affine_align": (td - ta) * 1e3, "layout": (time.perf_counter() - td) * 1e3,
                                      "correspondences": int((mom if mom is not None else r)["n_in"].astype(np.int64).sum()), "align_input": align_input}
        if cws * ch > canvas_cap:
            raise RuntimeError("canvas larger than provisioned (%d x %d)" % (cw, ch))
        if phases:
            t3 = time.perf_counter()
        if strong and world > 1:
            stripes = [((ch * q) // world, (ch * (q + 1)) // world - (ch * q) // world) for q in range(world)]      # canvas stripes: every image in index order per stripe
            mine = stripes[int(md.stripe_of_ranks(wv, hv, h9, owner, world)[rank])]      # the stripe that lies where this rank's own frames are (replicated geometry: the same deal on every rank)
            if owned_only:
                # the frames that give this stripe at least one pixel (the tile kernel's walk without its loads, on this rank's device); the rows of
                # all ranks are all-gathered inside the exchange, then every frame a stripe reads and its rank does not hold comes from its owner
                # (ncclSend / ncclRecv over xGMI)
                need_mine = ctx.StripeCover(wv, hv, h9, mine[0], mine[1], exact=md.exact_cover_pays(wv, hv, h9, cw, ch))
                ptrs, b_in, b_out = ex.exchange_frames(held, hv, wsv, need_mine, owner=owner)
                state["frame_exchange"] = {"bytes_received": b_in, "bytes_sent": b_out, "frames_read_by_the_stripe": int(need_mine.sum()), "frames_held": len(hold), "owner_rule": args.frame_owner}
            else:
                ptrs = [fptr[k] for k in range(F)]
            ctx.MosaicImagesRefinedDev(ptrs, wv, hv, wsv, h9, canvas.data_ptr(), cw, ch, cws, mine[0], mine[1])
        else:
            ctx.MosaicImagesRefinedDev([fptr[k] for k in range(F)], wv, hv, wsv, h9, canvas.data_ptr(), cw, ch, cws)
        if phases:
            ctx.synchronize(); t4 = time.perf_counter()
            state["warp_ms"] = (t4 - t3) * 1e3
            state["phase_ms"] = {"detect_describe" + ("+feature_allgather" if exchange and strong else ""): (t1 - t0) * 1e3,
                                 "match_select_ransac" + ("+result_allgather" if exchange else "_d2h"): (t2 - t1) * 1e3,
                                 "host_global_alignment": (t3 - t2) * 1e3, "warp": (t4 - t3) * 1e3}
            if os.environ.get("MI355_BENCH_PHASES"):
                print("[phases ms] sift %.1f  match+D2H %.1f  host align %.1f  warp %.1f" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3), file=sys.stderr)
        state.update(r=r, cw=cw, ch=ch, n_valid=int(label.sum()), h9=h9, cws=cws, rows=mine if (strong and world > 1) else (0, ch))

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if args.dump_outputs and args.steps < 1:
        raise SystemExit("--dump-outputs needs at least one timed step")
    for i in range(args.warmup):
        step(1 + i)
    # kernel events in the timed region feed the rooflines of --full only
    ctx.profile_enable((args.full or args.profile_all) and not os.environ.get("MI355_BENCH_NOPROF"))
    ctx.profile_only(None if args.profile_all else DOM + ",match,ransac")
    # the dominant class is launched 16 times per batch of frames (one launch per pyramid level of the wide octaves): bracket every 5th
    # launch (5 and 16 are coprime: every level is sampled equally often) -- two event records around each of ~500 launches per step
    # cost up to 15 % of the step on some boxes
    PROF_EVERY = 1 if args.profile_all else 5
    ctx.set_option("profile_every:" + DOM, PROF_EVERY)
    ctx.profile_reset()
    gc.collect(); gc.disable()      # the interpreter's cyclic collector is harness noise (a 60 ms pause at a fixed allocation count: found in the rank-share proxy)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(100 + i)
    barrier()
    dt = time.perf_counter() - t0
    gc.enable()
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev) if args.backend == "nccl" else torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, results, n_pairs, state["h9"], canvas, state["cw"], state["ch"], state["cws"], state["rows"])
    g_ms, g_n, g_bytes = ctx.profile_get(DOM)
    m_ms, m_n, _ = ctx.profile_get("match")
    rs_ms, rs_n, _ = ctx.profile_get("ransac")
    ctx.set_option("profile_every:" + DOM, 1)
    if world == 1 and args.full:         # one extra UNTIMED step with a synchronisation after every phase: where a step's time goes
        ctx.profile_enable(False)
        phases = True
        step(999)
        phases = bool(os.environ.get("MI355_BENCH_PHASES"))
        ctx.profile_enable(not os.environ.get("MI355_BENCH_NOPROF"))
    prof_all = {}
    if args.profile_all:
        for cls in ("gauss_stream", "gauss", "downsample", "extrema", "refine", "kp_select", "orient", "topk", "describe", "features", "match", "select", "ransac", "warp"):
            ms, n, b = ctx.profile_get(cls)
            prof_all[cls] = {"ms_per_step": ms / max(args.steps, 1), "launches_per_step": n / max(args.steps, 1)}
    ctx.profile_enable(False)
    # The timed region keeps three batches in flight: the bracketed blur_stream launches overlap other batches' kernels, so their event
    # durations double-count wall time.  `roofline.achieved` therefore comes from an extra UNTIMED pass over the same
    # frames with ONE batch work area in flight (exclusive_pass: nothing else on the chip while a bracketed launch runs -- the pass the
    # committed rocprofv3 serial summary traces).  Rounds 1-3 quoted a pass with the library option "serial_heavy" instead (the pyramid +
    # extrema phase of a batch waits for the previous batch's: no two chip-filling kernels overlap, checked right here, but the previous
    # batch's keypoint kernels share the chip with the bracketed launch): it stays in the line as shared_chip_pass, the in-situ figure
    # of the timed region as in_situ.
    excl, iso = None, None
    HEAVY = ("gauss_stream", "gauss", "downsample", "extrema")     # every class of the pyramid + extrema phase
    if args.full and not os.environ.get("MI355_BENCH_NO_STANDALONE"):
        ctx.synchronize()
        ctx.set_option("serial_heavy", 1)
        ctx.profile_enable(True); ctx.profile_only(",".join(HEAVY)); ctx.profile_reset()
        t_e = time.perf_counter()
        for k in own:
            ctx.SiftExtractDev(k, fptr[k], w, h, ws)
        ctx.synchronize()
        wall_ms = (time.perf_counter() - t_e) * 1e3
        e_ms, e_n, e_bytes = ctx.profile_get(DOM)
        x_ms, x_n, x_bytes = ctx.profile_get("extrema")
        heavy_ms = sum(ctx.profile_get(c)[0] for c in HEAVY)
        ctx.profile_enable(False)
        ctx.set_option("serial_heavy", 0)
        if e_ms > 0:
            excl = {"achieved": (e_bytes / 1e9) / (e_ms / 1e3), "launches": int(e_n), "avg_launch_us": e_ms * 1e3 / max(e_n, 1), "frames": len(own),
                    "dominant_kernel_ms": e_ms, "all_chip_filling_kernels_ms": heavy_ms, "pass_wall_ms": wall_ms,
                    "durations_are_exclusive": bool(heavy_ms <= wall_ms),
                    "extrema": {"ms": x_ms, "launches": int(x_n), "bytes": x_bytes}}
        # the same launches with ONE batch in flight (nothing else on the chip at all): the kernel's ceiling in this pipeline
        ctx.set_option("sift_slots", 1)
        ctx.profile_enable(True); ctx.profile_only(DOM); ctx.profile_reset()
        nf_iso = len(own)
        for k in own[:nf_iso]:
            ctx.SiftExtractDev(k, fptr[k], w, h, ws)
        i_ms, i_n, i_bytes = ctx.profile_get(DOM)
        ctx.profile_enable(False)
        ctx.set_option("sift_slots", SLOTS)
        ctx.set_option("sift_batch", BATCH)
        if i_ms > 0:
            iso = {"achieved": (i_bytes / 1e9) / (i_ms / 1e3), "frac": (i_bytes / 1e9) / (i_ms / 1e3) / HBM_PEAK_GBS, "frames": nf_iso, "dominant_kernel_ms": i_ms,
                   "launches": int(i_n), "avg_launch_us": i_ms * 1e3 / max(i_n, 1),
                   "note": "one batch work area in flight: no other kernel on the chip while a bracketed launch runs (what rocprofv3 --kernel-trace of scratch/sift_time.py ... serial reports: profiles/r06_rocprofv3_kernel_stats_serial_pass.txt), untimed extra pass"}

    # quality of the last step against ground truth (accepted pairs): corner transfer error in pixels
    if args.full:
        ctx.synchronize()
        r = state["r"]
        if r is None:                                                   # --align-input moments without the root gather: the records of the last step, fetched once, untimed
            if exchange and strong:
                r = ex.allgather_results(results, n_pairs, accepted_only=True)
            else:
                r = local_accepted()
        if exchange and strong and rank == 0:
            r = r[np.lexsort((r["j"], r["i"]))]                         # (rank 0 holds the records in both forms of the exchange)
        state["r"] = r
        errs = []
        corners = np.array([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], np.float64).T
        for rec in r:
            if not rec["accepted"]:
                continue
            i, j = int(rec["i"]), int(rec["j"])
            Hg = np.linalg.inv(affine3(A[i])) @ affine3(A[j])
            He = rec["H"].astype(np.float64).copy(); He[8] = 1.0; He = He.reshape(3, 3)
            a, b = He @ corners, Hg @ corners
            errs.append(float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max()))
        accepted = int(r["accepted"].sum()) if n_pairs else 0

    blend = None
    if args.blend and (world == 1 or strong):
        # LaplacianPyramidBlending of the survey as aligned by the last step: everything stays in HBM (device frames in, device canvas out).
        # N > 1 (one survey sharded): every rank blends ITS STRIPE of the canvas (mi355_mosaic_blended_rows_dev; the stripes are the whole
        # canvas's bytes: tests/test_blend.py, tests/test_gpu_full_size.py), the time reported is the slowest rank's
        h9b = state["h9"]
        keep = im.resample_by_overlap(wv, hv, h9b, 0.7)                 # MosaicImage.cpp:2227-2230
        bw_, bh_, _ = im.blend_layout(wv, hv, h9b, keep)
        sidx = int(md.stripe_of_ranks(wv, hv, h9b, owner, world)[rank]) if world > 1 else 0
        row0 = (bh_ * sidx) // world if world > 1 else 0
        rows = ((bh_ * (sidx + 1)) // world - row0) if world > 1 else -1
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        tb = []
        for rep in range(2):
            if world > 1:
                dist.barrier()
            t_b = time.perf_counter()
            if owned_only:
                # the blended stripe reads the chips that reach its rows plus the pyramids' reach: those frames come from their owners (timed)
                bneed = ctx.StripeCover(wv, hv, h9b, row0, rows, blended=True, keep=keep, band=5)
                bptrs, bb_in, bb_out = ex.exchange_frames(held, hv, wsv, bneed, owner=owner)
                blend_x = {"bytes_received": bb_in, "bytes_sent": bb_out, "frames_read_by_the_stripe": int(bneed.sum())}
            else:
                bptrs, blend_x = [fptr[k] for k in range(F)], None
            outb, bw_, bh_, bws_ = ctx.MosaicBlendedDev(bptrs, wv, hv, wsv, h9b, keep=keep, band=5, row0=row0, rows=rows)
            ctx.synchronize()
            tb.append((time.perf_counter() - t_b) * 1e3)
        if world > 1:
            tt = torch.tensor(tb, dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            tb = [float(v) for v in tt.cpu()]
        free1 = torch.cuda.mem_get_info()[0]
        tot = torch.cuda.mem_get_info()[1]
        blend = {"ms": min(tb), "ms_first_call": tb[0], "chips": int(keep.sum()), "canvas": [bw_, bh_], "bands": 5,
                 "stripes": world, "rows_of_rank0": rows if world > 1 else bh_,
                 "resident_gb": (tot - free1) / 1e9, "blend_buffers_gb": (free0 - free1) / 1e9, "frames_gb": len(hold) * h * ws / 1e9, "frame_exchange_rank0": blend_x,
                 "note": "mi355_mosaic_blended_dev / _rows_dev: chips (3 B) + masks (1 B per chip pixel) of the chips that reach the rank's rows + the rows of the canvas Laplacian / weight pyramids its output depends on, next to the frames; device in, device out (no PCIe); second call (buffers allocated); N > 1: max over the ranks"}
        del outb

    out = None
    # HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes of this same command
    # (profiles/pmc_traffic.py; counters cannot be read from inside the process): reported only when the workload matches
    traffic, traffic_src = None, None
    if args.full:
        try:
            pj = json.load(open(os.path.join(ROOT, "profiles", PMC_JSON)))
            if pj.get("frames") == str(F) and pj.get("frame") == "%dx%d" % (w, h) and pj.get("batch") == str(BATCH):
                traffic, traffic_src = float(pj["bytes_per_launch"]), "profiles/%s (FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes)" % PMC_JSON
        except Exception:
            pass
    if rank == 0:
        total_pairs = survey_pairs * args.steps
        value = total_pairs / dt
        out = {
            "metric": "image-pairs/sec (detect+match+H+warp), 4000x3000 UAV frames",
            "value": value, "unit": "image-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / max(args.steps, 1) * 1e3, "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "i16 fixed-point pyramid filtered in f32 (as the reference's OpenCV), f32 (RANSAC / warp coordinates), int8 MFMA with int32 accumulation (descriptor distances, exact), u8 (pixels)",
            "data": "synthetic",
            "transport": transport if exchange else None, "rccl_ranks": rccl_ranks,
            "config": {"workload": "%s: %s, pair window %d (%d pairs), SIFT(2000,3,0.01,20) + exact BF match + 3x3 grid select + Ransac2D + MosaicImagesRefined warp"
                                   % (("C3" if args.window == 2 else (("C5" if F >= 2000 else "C4") if args.window == 182 else "window-%d" % args.window)) + (" (block layout)" if args.layout == "block" else ""),
                                      ("ONE %d-frame %dx%d UAV survey" % (F, w, h)) if strong else ("%d-frame %dx%d UAV strip per GPU" % (F, w, h)),
                                      args.window, survey_pairs),
                       "frames": F if strong else F * world, "pairs": survey_pairs, "frames_per_gpu": len(own), "pairs_per_gpu": n_pairs,
                       "frame": [w, h], "canvas": [state["cw"], state["ch"]],
                       "sharding": ("single GPU" if world == 1 else
                                    ("frames %s, pairs i mod G, canvas stripes; %s exchanges: feature records, pair records / moments, frames" % ("in blocks of ceil(F/G)" if args.frame_owner == "blocks" else "k mod G", transport)) if strong else
                                    ("independent strip per rank; %s all-gather of accepted pair records" % transport))},
            "blend": blend,
        }
        if state.get("frame_exchange"):
            out["frame_exchange_rank0"] = state["frame_exchange"]
        out["frames_resident"] = (("owned (%s) + mi355_exchange_frames per step" % ("blocks of ceil(F/N)" if args.frame_owner == "blocks" else "k mod N")) if owned_only else "all frames on every rank") if world > 1 and strong else "single GPU"
        out["align_input"] = align_input + (" + records to rank 0's host (mi355_allgather_results root = 0, not waited for inside the step's host path)" if records_to_root else "")
    if rank == 0 and args.full:
        n_frames_total = F if strong else F * world
        in_situ = (g_bytes / 1e9) / (g_ms / 1e3) if g_ms > 0 else 0.0
        head = iso or excl                       # the kernel alone on the chip; the shared-chip pass if that one was skipped
        valu_of = lambda p: streamed_lane_ops(w, h) * p["frames"] / (p["dominant_kernel_ms"] / 1e3) / 1e12
        # ---- the pair stage's kernels.  ransac_kernel runs alone on the chip (the SIFT batches are done before the matcher starts, the host
        # waits for the records before it aligns): its bracketed duration is its own.  Lane-operations from the counted formula above on the
        # n_selected of THIS rank's pairs (last step's records, one strided field read back untimed).
        ransac_roof = None
        if rs_ms > 0 and n_pairs > 0:
            off_ns = im.PAIR_RESULT.fields["n_selected"][1]
            nsel = results[:n_pairs, off_ns:off_ns + 4].contiguous().cpu().numpy().view(np.int32).reshape(-1)
            ops_step = float(np.sum([ransac_lane_ops(int(v)) * c for v, c in zip(*np.unique(nsel, return_counts=True))]))
            rs_step_ms = rs_ms / max(args.steps, 1)
            ach = ops_step / (rs_step_ms / 1e3) / 1e12
            ransac_roof = {"bound": "valu", "kernel": "ransac_kernel (Ransac2D<SfPoint>: one workgroup per pair; draws solved, polished and counted lane per draw)",
                           "achieved": ach, "peak": VALU_PEAK_TOPS, "unit": "TFLOP/s", "frac": ach / VALU_PEAK_TOPS, "traffic": None,
                           "ms_per_step": rs_step_ms, "us_per_pair": rs_step_ms * 1e3 / n_pairs, "pairs_per_gpu": n_pairs,
                           "lane_ops_per_pair_mean": ops_step / n_pairs, "n_selected_mean": float(nsel.mean()), "pairs_with_fewer_than_4_selected": int((nsel < 4).sum()),
                           "ops": {"solve4": RANSAC_SOLVE_OPS, "gauss_newton_step": RANSAC_GN_STEP_OPS, "support_per_correspondence": RANSAC_SUPPORT_OPS,
                                   "per_pair": "1000 x (1.1 x solve4 [classification] + solve4 + 0.98 x 15 x gauss_newton_step + n_selected x support)"},
                           "note": "one separately rounded f32 operation = 1 FLOP (the reference's expression tree forbids fusing: -ffp-contract=off); peak = 256 CU x 128 lanes x 2.4 GHz "
                                   "non-fused f32 rate (the 157.3 TFLOP/s vector peak counts an fma as two); kernel time from HIP events around its one launch per step inside the timed region "
                                   "(it runs alone on the chip); the committed rocprofv3 --kernel-trace summary of this command reports the same average"}
        blur_step_ms = head["dominant_kernel_ms"] if head else 0.0
        pair_dominates = ransac_roof is not None and ransac_roof["ms_per_step"] > blur_step_ms
        out.update({
            "roofline": {"bound": "valu", "bound_note": "a streaming stencil priced against HBM as SURVEY 8d asks (achieved / peak / frac are GB/s of algorithmic bytes), but what limits it is f32 vector instruction issue: see `valu` (PMC traffic = 1.06 x the algorithmic bytes: nothing is re-read)",
                         "kernel": "blur16_stream<R,D,BGR> (streaming separable Gaussian 16S -> 32F -> 16S, one pyramid level of all frames of a batch per launch: every level at least 512 columns wide, the base level straight from the BGR frames)",
                         "achieved": head["achieved"] if head else in_situ, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": (head["achieved"] if head else in_situ) / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "note": "algorithmic bytes = 2 B read + 2 B written per pixel of a level (the reference's pyramid is 16-bit fixed point; base level: 3 B BGR read); the kernel is bound by f32 vector instruction issue, not by HBM: see valu",
                         "valu": ({"lane_ops_per_frame": streamed_lane_ops(w, h), "achieved": valu_of(head),
                                   "peak": VALU_PEAK_TOPS, "unit": "T f32 lane-operations/s", "frac": valu_of(head) / VALU_PEAK_TOPS,
                                   "shared_chip": ({"achieved": valu_of(excl), "frac": valu_of(excl) / VALU_PEAK_TOPS,
                                                    "note": "the same launches in the shared_chip_pass (the previous batch's keypoint kernels run beside them): the round-3 headline"} if excl else None),
                                   "note": "separately rounded f32 products and sums the definition requires (7R + 2 per output pixel; an fma would count once but changes the reference's bits); peak = 256 CU x 128 lanes x 2.4 GHz"} if head else None),
                         "measurement": ("HIP events around every launch of the kernel in an untimed extra pass over the same frames with ONE batch work area in flight: nothing else runs "
                                         "while a bracketed launch runs, the duration is the kernel's own (exclusive_pass; the committed rocprofv3 serial-pass summary measures the same). "
                                         "shared_chip_pass keeps the figure of rounds 1-3: option serial_heavy, the heavy phases of the batches take turns but the previous batch's "
                                         "keypoint kernels share the chip with the bracketed launch") if head else "HIP events in the timed region (launches overlap other batches' kernels)",
                         "exclusive_pass": iso, "shared_chip_pass": excl,
                         "shared_chip_frac": (excl["achieved"] / HBM_PEAK_GBS) if excl else None,      # the pipeline's figure next to the kernel's own (`frac`)
                         "in_situ": {"achieved": in_situ, "frac": in_situ / HBM_PEAK_GBS, "launches": int(g_n), "avg_launch_us": (g_ms * 1e3 / g_n) if g_n else None,
                                     "sampled": "every %d-th launch of the class" % PROF_EVERY,
                                     "note": "launches bracketed inside the timed region, three batches in flight: durations include other batches' kernels (sum > step time); rocprofv3 --kernel-trace of this command reports this average"},
                         "algorithmic_bytes_per_launch": (g_bytes / g_n) if g_n else None,
                         "algorithmic_bytes_per_frame": g_bytes * PROF_EVERY / max(args.steps * len(own), 1),
                         "frames_per_batch": BATCH, "batches_in_flight": SLOTS},
            # the other chip-filling kernels: exclusive durations of the same serial_heavy pass / the single warp launch of the last step
            "roofline_by_kernel": {
                "extrema_stream+extrema_kernel": ({"bound": "hbm", "algorithmic_bytes": "6 level reads x 2 B per pixel", "achieved": (excl["extrema"]["bytes"] / 1e9) / (excl["extrema"]["ms"] / 1e3),
                                                   "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": (excl["extrema"]["bytes"] / 1e9) / (excl["extrema"]["ms"] / 1e3) / HBM_PEAK_GBS,
                                                   "us_per_frame": excl["extrema"]["ms"] * 1e3 / excl["frames"]} if excl and excl["extrema"]["ms"] > 0 else None),
                "mosaic_tile_kernel": ({"bound": "hbm", "algorithmic_bytes": "6 B per frame pixel (SURVEY 8d B_W)", "achieved": 6.0 * w * h * len(own) / 1e9 / (state["warp_ms"] / 1e3),
                                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": 6.0 * w * h * len(own) / 1e9 / (state["warp_ms"] / 1e3) / HBM_PEAK_GBS,
                                        "ms": state["warp_ms"]} if state.get("warp_ms") else None)},
            # SURVEY 8(d)'s whole-path figure, with the pyramid the reference really builds (the survey priced a 2x doubled f32 pyramid, 256 P per
            # frame, which neither the reference nor this build forms: VERDICT r03 re-based it)
            "path_roofline": (lambda b: {"algorithmic_bytes_per_pair": b, "achieved": value / max(world, 1) * b / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                               "frac": value / max(world, 1) * b / 1e9 / HBM_PEAK_GBS,
                                               "note": "per GPU; (frames x 41 P + pairs x 1.04 MB) / pairs: 3 P BGR read + (4/3) P x 6 levels x 2 B x (1 write + 1 read) = 35 P per frame (16-bit pyramid, no doubled octave: oracle/oracle_sift.c), + 6 P warp, + 1.04 MB per pair"})(
                                       (n_frames_total * 41.0 * w * h + survey_pairs * 1.04e6) / max(survey_pairs, 1)),
            # north_star: MFMA utilisation of the only matrix kernel (exact all-pairs descriptor distances, v_mfma_i32_32x32x32_i8).
            # peak: MI355X_MICROARCH.md lists I8 at ~2x the bf16 rate (>= 3944 TOP/s measured there, 2 x 2500 nominal); on descriptor-like
            # operands scratch/mfma_bench.hip sustains 3.9 POP/s (4.9 on zeros: the pipe clocks lower on toggling data)
            "mfma": (lambda ops: {"kernel": "bf_match_kernel", "dtype": "i8 x i8 -> i32 (exact)", "op_per_pair": 2.0 * 2000 * 2000 * 128,
                                  "achieved": ops / (m_ms / 1e3) if m_ms > 0 else None, "peak": 5000.0, "unit": "TOP/s",
                                  "frac": (ops / (m_ms / 1e3) / 5000.0) if m_ms > 0 else None,
                                  "sustained_on_descriptor_operands": 3900.0, "frac_of_sustained": (ops / (m_ms / 1e3) / 3900.0) if m_ms > 0 else None,
                                  "ms_per_step": m_ms / max(args.steps, 1),
                                  "note": "nominal dense int8 rate (2 x the 2.5 PFLOP/s bf16 figure); round 2 ran this product in bf16 at 0.33 of 2500"})(
                         n_pairs * args.steps * 2.0 * 2000 * 2000 * 128 / 1e12),
            "phase_ms": state.get("phase_ms"), "host_parts_ms": state.get("host_parts_ms"),
            "roofline_shared_chip_frac": (excl["achieved"] / HBM_PEAK_GBS) if excl else None,      # dominant kernel with the other batches' keypoint kernels beside it (the pipeline's figure; roofline.frac is the kernel's own)
            "quality": {"pairs_accepted": accepted, "pairs": survey_pairs if strong else n_pairs, "images_aligned": state["n_valid"],
                        "h_corner_err_px_median": float(np.median(errs)) if errs else None,
                        "h_corner_err_px_max": float(np.max(errs)) if errs else None},
        })
        if prof_all:
            out["kernel_ms_per_step"] = prof_all
        # the line's `roofline` is the kernel that dominates THIS configuration's step: the blur for adjacent pairs (C3),
        # ransac_kernel once the pair window makes the pair stage the larger part (C4 / C5); the other one stays in roofline_by_kernel
        out["roofline_by_kernel"]["ransac_kernel"] = ransac_roof
        if pair_dominates:
            out["roofline_by_kernel"]["blur16_stream"] = out["roofline"]
            out["roofline"] = dict(ransac_roof, dominant_because="ransac_kernel %.1f ms per step against %.1f ms of blur16_stream (exclusive pass)" % (ransac_roof["ms_per_step"], blur_step_ms))
    # ---- CPU baseline: rank 0 at N=1 only, bounded sample; its pairs double as a parity sample for the GPU records ----
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        ns = min(20, F)
        fh = frames[:ns].cpu().numpy()
        try:
            cb, done = cpu_baseline([fh[k] for k in range(ns)], A, w, h, ws)
            out["cpu_baseline"] = cb
            cb["gpu_over_cpu"] = out["value"] / cb["value"]
            # the same pairs on the GPU with the oracle's seed: n_selected, n_in, inlier ids and H bits must be equal
            spairs = np.array([(k, k + 1) for k in range(ns - 1)], np.int32)
            g = ctx.MatchPairs(spairs, 2.5, 1)
            bad = []
            for p, (nin, i1, i2, Ho, nsel) in enumerate(done):
                r = g[p]
                ok = int(r["n_selected"]) == nsel and int(r["accepted"]) == int(nin > 30)
                if ok and nin > 30:
                    ok = int(r["n_in"]) == nin and np.array_equal(r["a"][:nin], i1[:nin]) and np.array_equal(r["b"][:nin], i2[:nin]) and \
                        np.array_equal(r["H"].view(np.uint32), Ho.view(np.uint32))
                if not ok:
                    bad.append(p)
            out["parity_sample"] = "equal" if not bad else "DIFFERS at sample pairs %s" % bad
            out["parity_sample_note"] = "%d adjacent pairs of the cpu_baseline sample: GPU records (features from the timed steps, seed 1) vs the oracle's n_selected / n_in / inlier lists / H bit patterns" % len(done)
            if args.window != 2:
                # window runs (C4 / C5): a sample of the LAST step's own records -- accepted and rejected pairs anywhere in the survey --
                # against oracle.match_pair on the GPU's features with that step's seed (the last step is the untimed phase step, seed 999)
                from tests import oracle_lib as ol
                orc = ol.load_oracle_fast() if hasattr(ol, "load_oracle_fast") else ol.load_oracle()
                res = results[:n_pairs].cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
                rng = np.random.default_rng(11)
                acc_i, rej_i = np.flatnonzero(res["accepted"] == 1), np.flatnonzero(res["accepted"] == 0)
                pick = np.concatenate([rng.choice(acc_i, min(24, len(acc_i)), replace=False), rng.choice(rej_i, min(24, len(rej_i)), replace=False)])
                fcache = {}

                def feat(k):
                    if k not in fcache:
                        kp, d = ctx.GetFeatures(k)
                        fcache[k] = (np.stack([kp["x"], kp["y"]], 1), d.astype(np.uint8))
                    return fcache[k]
                badw = []
                for pi in pick.tolist():
                    i_, j_ = int(pairs[pi][0]), int(pairs[pi][1])
                    (xi, di), (xj, dj) = feat(i_), feat(j_)
                    nin, i1, i2, Ho, nsel = orc.match_pair(xi, di, xj, dj, w, h, 2.5, 999)
                    r = res[pi]
                    ok = int(r["n_selected"]) == nsel and int(r["accepted"]) == int(nin > 30)
                    if ok and nin > 30:
                        ok = int(r["n_in"]) == nin and np.array_equal(r["a"][:nin], i1[:nin]) and np.array_equal(r["b"][:nin], i2[:nin]) and \
                            np.array_equal(r["H"].view(np.uint32), Ho.view(np.uint32))
                    if not ok:
                        badw.append((i_, j_))
                out["parity_window_sample"] = "equal" if not badw else "DIFFERS at pairs %s" % badw
                out["parity_window_sample_note"] = "%d accepted + %d rejected records of the last step (seed 999, window %d) vs oracle.match_pair on the GPU's features: n_selected / n_in / inlier lists / H bit patterns" % (
                    min(24, len(acc_i)), min(24, len(rej_i)), args.window)
        except Exception as e:       # the baseline must never take the GPU number down with it
            out["cpu_baseline"] = {"value": None, "unit": "image-pairs/s", "cores": None, "kind": "port", "sample": "failed: %r" % (e,)}
    elif rank == 0 and args.full:
        out["cpu_baseline"] = None
    # ---- what INTEGRATION.md's caller gets: frames in PAGEABLE host memory, as the reference's IplImages are, through
    # mi355_sift_extract (deferred form: staged into HBM, batched) -> mi355_match_pairs (records to the host) -> host alignment ->
    # mi355_mosaic_refined (host frames in, host canvas out).  Untimed extra on a bounded sample; `value` stays the resident figure.
    if rank == 0 and world == 1 and args.full and not args.no_host_frames:
        try:
            nH = min(F, 96)
            host = [frames[slot_of[k]].cpu().numpy() for k in range(nH)]
            imgs = [np.ascontiguousarray(f.reshape(h, ws)[:, :3 * w]).reshape(h, w, 3) for f in host]
            hp = im.pair_schedule(nH, args.window)

            def host_pass(seed):
                for k in range(nH):
                    ctx.SiftExtractHost(k, imgs[k])
                res = ctx.MatchPairs(hp, 2.5, seed)
                lab = im.select_connected_results(res, nH) if len(res) else np.zeros(nH, np.int32)
                lab[0] = 1
                T = im.global_affine_align_results(res, nH, fixed=[1 if (k == 0 or lab[k] == 0) else 0 for k in range(nH)], label=lab)
                hh = T["m"].copy()
                hh[lab == 0, 8] = 0.0
                _, cw_h, ch_h, _ = ctx.MosaicImagesRefined(imgs, hh, want_pixels=False)
                return int(res["accepted"].sum()), cw_h, ch_h
            host_pass(1)
            t_h = time.perf_counter()
            acc_h, cw_h, ch_h = host_pass(2)
            dt_h = time.perf_counter() - t_h
            out["host_frames"] = {"value": len(hp) / dt_h, "unit": "image-pairs/s", "frames_per_s": nH / dt_h, "ms": dt_h * 1e3, "pairs_accepted": acc_h, "canvas": [cw_h, ch_h],
                                  "sample": "%d frames %dx%d in pageable host memory (numpy), pair window %d (%d pairs): mi355_sift_extract (deferred form, %d MB upload per frame) -> mi355_match_pairs "
                                            "(records to the host) -> host alignment -> mi355_mosaic_refined (host frames uploaded again, canvas back to the host); second pass of two" % (nH, w, h, args.window, len(hp), h * ws >> 20),
                                  "note": "what a caller of include/mi355_adaptor.h gets (the reference passes host IplImages): bound by the PCIe uploads (each frame crosses twice: extraction and warp); "
                                          "`value` above is the HBM-resident figure the metric defines (SURVEY 8d excludes H2D)"}
        except Exception as e:
            out["host_frames"] = {"value": None, "sample": "failed: %r" % (e,)}
    if rank == 0:
        # RCCL prints a version banner through C stdio at communicator creation: flush it first so that the JSON line is the last line
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)
    if ex is not None:
        ex.close()
    ctx.set_stream(None)
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

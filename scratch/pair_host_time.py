"""the pair stage of the 60-frame benchmark configuration (60 synthetic frames of 4000 x 3000, SIFT 2000 keypoints, the 59 adjacent pairs) as the
   host sees it: wall time of one mi355_match_pairs_dev call with a device synchronise after it, and the time until the call itself returns
   (its host work and the one upload it waits for).  Also one pair alone, mi355_bf_match and mi355_select_grid, whose host side is most of them.
   One JSON line; run it with MI355_LIB set to compare two builds of the library, processes alternating.
       python scratch/pair_host_time.py [--reps 40]"""
import argparse, hashlib, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagemosaicing_amd as im
from tests.synth_survey import frame_layout

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=40)
args = ap.parse_args()
w, h, F = 4000, 3000, 60
ws = 3 * w
A, g = frame_layout(F, w, h, 0)
ctx = im.Context(0)
st = torch.cuda.Stream(); torch.cuda.set_stream(st); ctx.set_stream(st.cuda_stream)
frames = torch.empty((F, h * ws), dtype=torch.uint8, device='cuda')
for k in range(F): ctx.SynthFrameDev(frames[k].data_ptr(), w, h, ws, A[k], 0xC0FFEE, k, g[k], 2.0)
for k in range(F): ctx.SiftExtractDev(k, frames[k].data_ptr(), w, h, ws)
ctx.synchronize()
adj = [(i, i + 1) for i in range(F - 1)]
out = {"lib": os.environ.get("MI355_LIB", "in-tree"), "reps": args.reps}
for name, pairs in (("pairs_59", adj), ("pairs_1", adj[:1])):
    res = torch.zeros((len(pairs), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device='cuda')
    for _ in range(3): ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7)
    ctx.synchronize()
    call, wall = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 7); t1 = time.perf_counter(); ctx.synchronize(); t2 = time.perf_counter()
        call.append((t1 - t0) * 1e3); wall.append((t2 - t0) * 1e3)
    rec = np.frombuffer(res.cpu().numpy().tobytes(), im.PAIR_RESULT)
    out[name] = {"wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall), "call_ms_median": statistics.median(call), "call_ms_min": min(call),
                 "accepted": int(rec["accepted"].sum()), "records_sha1": hashlib.sha1(rec.tobytes()).hexdigest()}
ctx.BFMatch(0, 1)
ts = []
for _ in range(args.reps):
    t0 = time.perf_counter(); m = ctx.BFMatch(0, 1); ts.append((time.perf_counter() - t0) * 1e3)
out["bf_match"] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "matches": len(m[0])}
kp0, kp1 = ctx.GetFeatures(0)[0], ctx.GetFeatures(1)[0]
xy0, xy1 = np.stack([kp0["x"], kp0["y"]], 1), np.stack([kp1["x"], kp1["y"]], 1)
mm = np.stack([m[0]["queryIdx"], m[0]["trainIdx"]], 1).astype(np.int32)
ctx.SelectMatchPairs(mm, xy0, xy1, 400, w, h)
ts = []
for _ in range(args.reps):
    t0 = time.perf_counter(); s = ctx.SelectMatchPairs(mm, xy0, xy1, 400, w, h); ts.append((time.perf_counter() - t0) * 1e3)
out["select_grid"] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "selected": len(s[0])}
ctx.close()
print(json.dumps(out), flush=True)

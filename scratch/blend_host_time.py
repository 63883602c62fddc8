"""Host-side cost of mi355_mosaic_blended_dev, one library against another (the parent commit's build against this tree's): a refactor of the
blend's host path must leave every figure inside the parent's own spread between processes, and every canvas checksum equal.

Two surveys, each blended whole and as one stripe of an eighth of the rows:
  big    scratch/blend_dev_time.py's block of 200 resident 12 MP frames (kernel time dominates)
  small  60 chips of 640 x 480 (the host share is visible); for these also the time until the call returns
Every figure is the median over --reps calls after one untimed first call (buffers allocated).  Processes alternate parent, new, new, parent
(MI355_LIB chooses the library of a process); the spread of a figure is the distance between the parent's two processes.

    python scratch/blend_host_time.py --parent-lib PATH [--reps 15] [--frames 200] [--out profiles/blend_host_refactor_time.json]
    python scratch/blend_host_time.py --worker      (one process, one library: prints its figures as JSON)
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(a):
    import torch
    import imagemosaicing_amd as im
    from imagemosaicing_amd.capi import _p
    from tests.synth_survey import affine3, block_layout
    ctx = im.Context(0)
    out = {"lib": im.lib_path()}

    def survey(F, w, h, cols, extent, resample):
        ws = (3 * w + 3) & ~3
        A = block_layout(F, w, h, cols=cols, extent=extent)
        frames = torch.empty((F, h * ws), dtype=torch.uint8, device="cuda")
        for k in range(F):
            ctx.SynthFrameDev(frames[k].data_ptr(), w, h, ws, A[k], 0xC5C5C5, k, 1.0, 2.0)
        ctx.synchronize()
        A0i = np.linalg.inv(affine3(A[0]))
        h9 = np.stack([(A0i @ affine3(A[k])).reshape(9) for k in range(F)]).astype(np.float32)
        wv, hv, wsv = np.full(F, w, np.int32), np.full(F, h, np.int32), np.full(F, ws, np.int32)
        keep = im.resample_by_overlap(wv, hv, h9, 0.7) if resample else np.ones(F, np.uint8)
        return frames, (C.c_void_p * F)(*[frames[k].data_ptr() for k in range(F)]), wv, hv, wsv, h9, np.ascontiguousarray(keep, np.uint8)

    def measure(name, sv, returns):
        frames, ptrs, wv, hv, wsv, h9, keep = sv
        F = len(wv)
        cw, ch, cws = im.blend_layout(wv, hv, h9, keep)
        canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rows8 = ch // 8
        for what, row0, rows in (("whole", 0, ch), ("stripe", 3 * rows8, rows8)):
            wall, ret = [], []
            for rep in range(a.reps + 1):
                ctx.synchronize()
                t0 = time.perf_counter()
                if what == "whole":
                    rc = ctx.L.mi355_mosaic_blended_dev(ctx._h, ptrs, _p(wv), _p(hv), _p(wsv), F, _p(h9), _p(keep), 5, C.c_void_p(canvas.data_ptr()), cw, ch, cws)
                else:
                    rc = ctx.L.mi355_mosaic_blended_rows_dev(ctx._h, ptrs, _p(wv), _p(hv), _p(wsv), F, _p(h9), _p(keep), 5, C.c_void_p(canvas.data_ptr()), cw, ch, cws, row0, rows)
                t1 = time.perf_counter()
                ctx._chk(rc)
                ctx.synchronize()
                t2 = time.perf_counter()
                if rep:                                          # the first call allocates
                    wall.append((t2 - t0) * 1e3); ret.append((t1 - t0) * 1e3)
            got = canvas[:rows].cpu().numpy()
            r = {"wall_ms": round(float(np.median(wall)), 3), "wall_ms_min": round(min(wall), 3), "sha": hashlib.sha1(got.tobytes()).hexdigest()[:16]}
            if returns:
                r["return_ms"] = round(float(np.median(ret)), 3)
            out["%s_%s" % (name, what)] = r
        out[name] = {"chips": int(keep.sum()), "canvas": [cw, ch]}

    measure("small", survey(60, 640, 480, 10, 2500.0, False), True)
    if a.frames > 0:
        cols = 20
        measure("big", survey(a.frames, 4000, 3000, cols, 20000.0 * cols / 50.0 + 4000, True), False)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=200, help="frames of the big survey (0: leave it out)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's libmi355mosaic.so")
    runs = []
    for which in ("parent", "new", "new", "parent"):
        env = dict(os.environ)
        env.pop("MI355_LIB", None)
        if which == "parent":
            env["MI355_LIB"] = os.path.abspath(a.parent_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--frames", str(a.frames)], env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit("%s process failed (%d): %s" % (which, r.returncode, r.stderr[-2000:]))
        runs.append((which, json.loads(line[0][7:])))
        print(which, line[0][7:], flush=True)
    figures, ok = {}, True
    for key in [k for k in runs[0][1] if "_" in k]:
        for field in ("wall_ms", "return_ms"):
            if field not in runs[0][1][key]:
                continue
            p = [r[key][field] for w, r in runs if w == "parent"]
            n = [r[key][field] for w, r in runs if w == "new"]
            spread = abs(p[0] - p[1])
            slower_by = max(n) - sum(p) / 2                      # the requirement: no figure of the new library slower than the parent's (mean of its two) by more than the spread
            figures["%s.%s" % (key, field)] = {"parent": p, "new": n, "parent_spread": round(spread, 3), "new_worst_minus_parent_mean": round(slower_by, 3),
                                               "within_spread": bool(slower_by <= spread)}
            ok = ok and slower_by <= spread
        shas = {r[key]["sha"] for _, r in runs}
        figures[key + ".sha"] = {"values": sorted(shas), "equal": len(shas) == 1}
        ok = ok and len(shas) == 1
    out = {"order": [w for w, _ in runs], "reps": a.reps, "surveys": {k: v for k, v in runs[0][1].items() if k in ("small", "big")}, "figures": figures, "all_within_spread_and_equal": ok}
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(s)


if __name__ == "__main__":
    main()

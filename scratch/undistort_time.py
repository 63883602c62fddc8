"""Times the lens undistortion (csrc/undistort.hip) out of place and in place next to mi355_apply_gains_dev out of place and in place -- the pass
that moves exactly the same bytes with streaming loads -- on the same frames in the same process, and writes a JSON record
(profiles/undistort_time.json).

    python scratch/undistort_time.py [OUT.json] [--quick]

C3: 500 frames of 4000x3000 (tests/synth_survey.py strip layout).  The camera is the tests' barrel camera (f = 0.8 w, k1 = -0.25, k2 = 0.07)
with the output camera mi355_undistort_fit gives, and the pincushion camera with its own intrinsics (rim pixels without a sample).  Per pass:
kernel time from the library's profile brackets (classes "undistort" and "gain_apply"; one warm-up call, then 5 timed ones, the passes
alternating), the wall time of the calls (the in-place form's copies back are wall time only), and the achieved bytes per second over the
6 w h bytes a frame needs.  --quick: 60 frames."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import imagemosaicing_amd as im  # noqa: E402
from tests import undistort_ref as ur  # noqa: E402
from tests.synth_survey import frame_layout  # noqa: E402

W, H = 4000, 3000


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    reps = 5
    ctx = im.Context(0)
    F = 60 if quick else 500
    A, gains = frame_layout(F, W, H)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
    ctx.synchronize()
    dst = torch.empty_like(frames)
    sp = [frames[k].data_ptr() for k in range(F)]
    dp = [dst[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    cams = ur.cameras_for(W, H)
    barrel = im.Camera(**cams["barrel"])
    fitted = im.undistort_fit(barrel, W, H)
    pin = im.Camera(**cams["pincushion"])
    g = np.random.default_rng(2).uniform(0.9, 1.1, (F, 3)).astype(np.float32)
    outside = {}

    def ud(cam, prm, d, key):
        outside[key] = ctx.UndistortFramesDev(sp, d, wv, hv, wsv, wsv, cam, prm)

    passes = {
        "undistort_out_of_place": (lambda: ud(barrel, fitted, dp, "barrel_fitted"), "undistort"),
        "undistort_in_place": (lambda: ud(barrel, fitted, sp, "barrel_fitted_in_place"), "undistort"),
        "undistort_pincushion_own_out_of_place": (lambda: ud(pin, im.undistort_params(), dp, "pincushion_own"), "undistort"),
        "apply_gains_out_of_place": (lambda: ctx.ApplyGainsDev(sp, dp, wv, hv, wsv, g), "gain_apply"),
        "apply_gains_in_place": (lambda: ctx.ApplyGainsDev(sp, sp, wv, hv, wsv, g), "gain_apply"),
    }
    ctx.profile_enable(True)
    for name, (call, _) in passes.items():                                  # warm-up of every pass
        call()
    ctx.synchronize()
    kern = {k: [] for k in passes}
    wall = {k: [] for k in passes}
    for rep in range(reps):                                                 # the passes alternate
        for name, (call, cls) in passes.items():
            ctx.profile_reset()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            ms, n, _ = ctx.profile_get(cls)
            kern[name].append(ms)
        note("rep", rep, {k: round(v[-1], 3) for k, v in kern.items()})
    ctx.profile_enable(False)
    need = 6.0 * W * H * F
    rec = {"frames": F, "frame": "%dx%d" % (W, H), "pitch": ws, "bytes_needed": need, "reps": reps,
           "barrel_fit_j": int(round(fitted.out_fx * 256.0 / float(np.float32(cams["barrel"]["fx"])))),
           "n_outside_per_frame": {k: int(v[0]) for k, v in outside.items()}}
    for name in passes:
        k = float(np.median(kern[name]))
        rec[name] = {"kernel_ms_median": k, "kernel_ms_all": kern[name], "call_ms_median": float(np.median(wall[name])), "call_ms_all": wall[name],
                     "kernel_TB_per_s": need / (k * 1e-3) / 1e12}
    rec["undistort_over_apply_gains_out_of_place"] = rec["undistort_out_of_place"]["kernel_ms_median"] / rec["apply_gains_out_of_place"]["kernel_ms_median"]
    rec["undistort_over_apply_gains_in_place_calls"] = rec["undistort_in_place"]["call_ms_median"] / rec["apply_gains_in_place"]["call_ms_median"]
    print(json.dumps(rec, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""numpy restatement of what the candidates of a frame DO in SIFT's sub-pixel refinement: the pyramid, the extrema test and the Newton
loop of oracle/oracle_sift.c (orc_sift, adjust_extremum), operation by operation in float32, with every candidate's trajectory kept.

The oracle returns keypoints only; the tests of refine_kernel's movers need to know that their inputs hold a row-only move, a layer-only
move, a column move, a move of more than one pixel, a mover that converges, and candidates that come back to a location of their own
(test_gpu_sift_refine_movers.py), and the trajectory rule itself is checked on move tables (test_sift_refine_revisit_rule.py).
summary()["records"] is what ties the restatement to the oracle: the locations it accepts are those of the oracle's keep-all keypoints."""
import numpy as np

N_LAYERS, N_LEVELS, IMG_BORDER, MAX_INTERP, FIXPT_SCALE = 3, 6, 5, 5, 48
SIGMA = 1.6
CONTRAST_THR, EDGE_THR = np.float32(0.01), np.float32(20.0)
f32 = np.float32


def gauss_kernel(sigma):
    ksize = int(np.rint(sigma * 8.0 + 1.0)) | 1
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp((-0.5 / (sigma * sigma)) * x * x).astype(np.float32)
    s = 0.0
    for v in k:
        s += float(v)
    return (k.astype(np.float64) * (1.0 / s)).astype(np.float32), ksize // 2


def blur16(src, sigma):
    """gauss_blur16: row pass with ascending taps, column pass centre tap first then the symmetric pairs, round half to even into 16 bits"""
    h, w = src.shape
    k, r = gauss_kernel(sigma)
    ext = np.pad(src.astype(np.float32), ((0, 0), (r, r)), mode="reflect")
    t = k[0] * ext[:, 0:w]
    for i in range(1, 2 * r + 1):
        t = t + k[i] * ext[:, i:i + w]
    tp = np.pad(t, ((r, r), (0, 0)), mode="reflect")
    acc = k[r] * t
    for j in range(1, r + 1):
        acc = acc + k[r + j] * (tp[r + j:r + j + h] + tp[r - j:r - j + h])
    return np.clip(np.rint(acc), -32768, 32767).astype(np.int16)


def dog_pyramid(bgr):
    """per octave the five DoG planes as int32 [5, h, w]"""
    b = bgr.astype(np.int64)
    gray = (((1868 * b[..., 0] + 9617 * b[..., 1] + 4899 * b[..., 2] + 8192) >> 14) * FIXPT_SCALE).astype(np.int16)
    k = 2.0 ** (1.0 / N_LAYERS)
    sig = [SIGMA] + [np.sqrt((k ** i * SIGMA) ** 2 - (k ** (i - 1) * SIGMA) ** 2) for i in range(1, N_LEVELS)]
    sd = np.sqrt(np.maximum(f32(SIGMA) * f32(SIGMA) - f32(0.25), f32(0.01)), dtype=np.float32)
    out, lv0 = [], blur16(gray, float(sd))
    n_oct = int(np.rint(np.log(float(min(gray.shape))) / np.log(2.0) - 2.0))
    while len(out) < n_oct and min(lv0.shape) >= 2 * IMG_BORDER + 2:
        lv = [lv0]
        for i in range(1, N_LEVELS):
            lv.append(blur16(lv[-1], sig[i]))
        out.append(np.stack([lv[i + 1].astype(np.int32) - lv[i].astype(np.int32) for i in range(N_LEVELS - 1)]))
        h, w = lv0.shape
        lv0 = np.ascontiguousarray(lv[N_LAYERS][0:2 * (h >> 1):2, 0:2 * (w >> 1):2])
    return out


def extrema(D):
    """(layer, row, column) of the candidates of one octave, in generation order"""
    n, h, w = D.shape
    B = IMG_BORDER
    got = []
    for l in range(1, N_LAYERS + 1):
        v = D[l, B:h - B, B:w - B]
        mx, mn = np.ones(v.shape, bool), np.ones(v.shape, bool)
        for dl in (-1, 0, 1):
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    q = D[l + dl, B + dr:h - B + dr, B + dc:w - B + dc]
                    mx &= v >= q
                    mn &= v <= q
        r, c = np.nonzero((np.abs(v) > 20) & np.where(v > 0, mx, mn))
        got.append(np.stack([np.full(len(r), l), r + B, c + B], 1))
    return np.concatenate(got)


def _fit(D, L, R, C):
    """one Newton step at the locations: the offsets (xi, xr, xc) as adjust_extremum computes them"""
    img = f32(1.0) / f32(255 * FIXPT_SCALE)
    ds, ss, cs = img * f32(0.5), img, img * f32(0.25)
    d = lambda a, b, c: D[L + a, R + b, C + c]
    F = lambda x: x.astype(np.float32)
    dD = [F(d(0, 0, 1) - d(0, 0, -1)) * ds, F(d(0, 1, 0) - d(0, -1, 0)) * ds, F(d(1, 0, 0) - d(-1, 0, 0)) * ds]
    v2 = F(d(0, 0, 0)) * f32(2.0)
    dxx = (F(d(0, 0, 1) + d(0, 0, -1)) - v2) * ss
    dyy = (F(d(0, 1, 0) + d(0, -1, 0)) - v2) * ss
    dss = (F(d(1, 0, 0) + d(-1, 0, 0)) - v2) * ss
    dxy = F(d(0, 1, 1) - d(0, 1, -1) - d(0, -1, 1) + d(0, -1, -1)) * cs
    dxs = F(d(1, 0, 1) - d(1, 0, -1) - d(-1, 0, 1) + d(-1, 0, -1)) * cs
    dys = F(d(1, 1, 0) - d(1, -1, 0) - d(-1, 1, 0) + d(-1, -1, 0)) * cs
    a = [[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]]
    b = dD
    det = (a[0][0] * (a[1][1] * a[2][2] - a[2][1] * a[1][2]) - a[0][1] * (a[1][0] * a[2][2] - a[2][0] * a[1][2])) + a[0][2] * (a[1][0] * a[2][1] - a[2][0] * a[1][1])
    with np.errstate(all="ignore"):
        q = f32(1.0) / det
        x0 = q * ((b[0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (b[1] * a[2][2] - a[1][2] * b[2])) + a[0][2] * (b[1] * a[2][1] - a[1][1] * b[2]))
        x1 = q * ((a[0][0] * (b[1] * a[2][2] - a[1][2] * b[2]) - b[0] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) + a[0][2] * (a[1][0] * b[2] - b[1] * a[2][0]))
        x2 = q * ((a[0][0] * (a[1][1] * b[2] - b[1] * a[2][1]) - a[0][1] * (a[1][0] * b[2] - b[1] * a[2][0])) + b[0] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    z = det == 0
    xi, xr, xc = np.where(z, f32(0), -x2), np.where(z, f32(0), -x1), np.where(z, f32(0), -x0)
    # the contrast and edge tests of a converged location
    t = ((f32(0.0) + dD[0] * xc) + dD[1] * xr) + dD[2] * xi
    contr = F(d(0, 0, 0)) * img + t * f32(0.5)
    tr, dt = dxx + dyy, dxx * dyy - dxy * dxy
    ok = ~(np.abs(contr) * f32(N_LAYERS) < CONTRAST_THR) & ~((dt <= 0) | ((tr * tr) * EDGE_THR >= ((EDGE_THR + f32(1)) * (EDGE_THR + f32(1))) * dt))
    return xi, xr, xc, ok


CONVERGED, REJECTED, DIVERGED, LEFT, RAN_OUT = range(5)


def trajectories(D, cand):
    """The unshortened loop for every candidate of one octave.  Returns (path, end): path[n, MAX_INTERP + 1, 3] the locations fitted at, in
    order ((0, 0, 0) past the end; entry MAX_INTERP is where the last move of a candidate that ran out of steps went), end[n] how the loop ended"""
    n = len(cand)
    _, h, w = D.shape
    path = np.zeros((n, MAX_INTERP + 1, 3), np.int64)
    end = np.full(n, RAN_OUT)
    live = np.arange(n)
    loc = cand.astype(np.int64).copy()
    for it in range(MAX_INTERP):
        path[live, it] = loc
        xi, xr, xc, ok = _fit(D, loc[:, 0], loc[:, 1], loc[:, 2])
        conv = (np.abs(xi) < 0.5) & (np.abs(xr) < 0.5) & (np.abs(xc) < 0.5)
        bad = ~conv & ((np.abs(xi) > 7.0e8) | (np.abs(xr) > 7.0e8) | (np.abs(xc) > 7.0e8) | np.isnan(xi) | np.isnan(xr) | np.isnan(xc))
        end[live[conv]] = np.where(ok[conv], CONVERGED, REJECTED)
        end[live[bad]] = DIVERGED
        go = ~conv & ~bad
        live, loc = live[go], loc[go] + np.stack([np.rint(xi[go]), np.rint(xr[go]), np.rint(xc[go])], 1).astype(np.int64)
        out = (loc[:, 0] < 1) | (loc[:, 0] > N_LAYERS) | (loc[:, 2] < IMG_BORDER) | (loc[:, 2] >= w - IMG_BORDER) | (loc[:, 1] < IMG_BORDER) | (loc[:, 1] >= h - IMG_BORDER)
        end[live[out]] = LEFT
        live, loc = live[~out], loc[~out]
    path[live, MAX_INTERP] = loc
    return path, end


def early_exit_step(path, end, full_history=False):
    """The step (1 .. MAX_INTERP - 1) at which refine_kernel drops a candidate for coming back to a location of its own, 0 where it does
    not.  The kernel compares the location a move lands on with the one it left, the one before that and the first one -- of the at most
    four earlier locations that leaves out the second, at the last test; full_history compares with all of them."""
    n = len(path)
    step = np.zeros(n, np.int64)
    nfit = np.where(end == RAN_OUT, MAX_INTERP + 1, (path.any(2)).sum(1))        # locations reached, the target of the last move included
    for k in range(1, MAX_INTERP):
        reached = (nfit > k) & (step == 0)
        earlier = range(k) if full_history else sorted({0, k - 1, max(k - 2, 0)})
        back = np.zeros(n, bool)
        for j in earlier:
            back |= (path[:, k] == path[:, j]).all(1)
        step[reached & back] = k
    return step


def half_pixel_blobs(w, h, pitch=20):
    """Gaussian blobs, bright and dark, on a grid: centred half a pixel off in x, in y, in both and on a pixel in turn, with thirteen
    widths from 1.3 to 5.2 pixels in steps of a sixth of an octave, so that half of them lie between two DoG layers.  The extremum
    of such a blob sits between two pixels or two layers, and its Newton offset flips across 0.5."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 128.0)
    k = 0
    for cy in range(pitch // 2 + 2, h - pitch // 2, pitch):
        for cx in range(pitch // 2 + 2, w - pitch // 2, pitch):
            ox, oy = ((0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.0, 0.0))[k % 4]
            sg = 1.3 * 2.0 ** ((k % 13) / 6.0)
            a = 90.0 if (k // 4) % 2 == 0 else -90.0
            img += a * np.exp(-((xx - cx - ox) ** 2 + (yy - cy - oy) ** 2) / (2 * sg * sg))
            k += 1
    g = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))


def summary(bgr):
    """what the frame's candidates do: counts over all octaves (see the keys), and the accepted locations as a set of (octave, layer, row, column)"""
    s = dict(candidates=0, row_only=0, layer_only=0, column=0, far=0, mover_converged=0, early_exits=0, early_exits_full=0, ran_out=0, early_exits_by_octave=[], records=set())
    for o, D in enumerate(dog_pyramid(bgr)):
        cand = extrema(D)
        s["early_exits_by_octave"].append(0)
        if not len(cand):
            continue
        path, end = trajectories(D, cand)
        assert not (early_exit_step(path, end, True)[end != RAN_OUT]).any(), "a candidate came back to a location of its own and did not run out of steps"
        nloc = np.where(end == RAN_OUT, MAX_INTERP + 1, path.any(2).sum(1))
        es = early_exit_step(path, end)
        for k in range(1, MAX_INTERP):                   # the moves that refine_kernel follows with a fit: not the one it drops a candidate at
            m = (nloc > k) & ((es == 0) | (k < es))
            d = np.abs(path[m, k] - path[m, k - 1])
            far = (d > 1).any(1)
            s["far"] += int(far.sum())
            s["column"] += int((~far & (d[:, 2] == 1)).sum())
            s["row_only"] += int((~far & (d[:, 2] == 0) & (d[:, 1] == 1) & (d[:, 0] == 0)).sum())
            s["layer_only"] += int((~far & (d[:, 2] == 0) & (d[:, 1] == 0) & (d[:, 0] == 1)).sum())
        s["candidates"] += len(cand)
        s["mover_converged"] += int(((end == CONVERGED) & (nloc > 1)).sum())
        s["ran_out"] += int((end == RAN_OUT).sum())
        s["early_exits"] += int((es > 0).sum())
        s["early_exits_by_octave"][o] = int((es > 0).sum())
        s["early_exits_full"] += int((early_exit_step(path, end, True) > 0).sum())
        last = path[np.arange(len(path)), np.maximum(nloc - 1, 0)]
        for L, R, C in last[end == CONVERGED]:
            s["records"].add((o, int(L), int(R), int(C)))
    return s

"""The warps and the distance-map ownership once more, in plain numpy with float32 intermediates: a second opinion on oracle/oracle_warp.c,
written from what the reference's code means and not from the oracle's text.

  * destination -> source through the INVERSE homography: x = (m0 X + m1 Y + m2) / (m6 X + m7 Y + m8), y likewise -- two divisions by the
    same denominator expression; every product and every sum is rounded to float32 on its own, sums run left to right;
  * a destination pixel has a sample when 0 <= x < w - 1 and 0 <= y < h - 1 (a NaN has none);
  * the sample is the four-term bilinear sum  s00 (1-p)(1-q) + s01 (1-p) q + s10 p (1-q) + s11 p q  with p, q the fractions of y, x; each
    term is ((s * a) * b), the terms are added left to right and the float is truncated to a byte;
  * the refined render composites the frames in ascending index: the LAST frame with a sample wins;
  * a chip's ownership value is the distance of the pixel to the nearest of the four quad edges divided by the chip's maximum of it; a
    canvas pixel belongs to the chip with the largest value, and among equals to the FIRST (a value must be strictly larger to take over,
    the start is 0: a pixel on an edge line, value 0, is owned by nobody).

The 3 x 3 inverse is an input of the warps; inverse() below gives it: Gauss-Jordan on [A | I] in float32 -- for column i the pivot is the first
row not used yet whose entry exceeds eps in magnitude (none: no inverse), the pivot row is divided by it, and -entry times the pivot row is
added to every other row whose entry in that column is at least eps in magnitude; at the end the rows are put in the order of their leading
ones.  Everything is vectorised over the destination pixels; nothing here is fast or meant to be.
"""
import numpy as np

f32 = np.float32
BIG = f32(1 << 29)


def _m(h9):
    return [f32(v) for v in np.asarray(h9, np.float32).reshape(9)]


def inverse(h9, eps):
    """float32[9] or None"""
    t = np.concatenate([np.asarray(h9, np.float32).reshape(3, 3), np.eye(3, dtype=np.float32)], 1)
    eps = f32(eps)
    used = []
    with np.errstate(all="ignore"):
        for i in range(3):
            rows = [j for j in range(3) if j not in used and abs(t[j, i]) > eps]
            if not rows:
                return None
            r = rows[0]
            used.append(r)
            t[r] = t[r] / t[r, i]
            for j in range(3):
                if j != r and not abs(t[j, i]) < eps:
                    t[j] = t[j] + (-t[j, i]) * t[r]
        for r in range(3):                           # the row whose entry in column r is 1, first in row order, goes to place r
            hit = [i for i in range(3) if t[i, r] == 1]
            if hit and hit[0] != r:
                t[[r, hit[0]]] = t[[hit[0], r]]
    return np.ascontiguousarray(t[:, 3:]).reshape(9)


def project(h9, x, y):
    """two divisions by the same denominator"""
    m = _m(h9)
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        den = (m[6] * x + m[7] * y) + m[8]
        return ((m[0] * x + m[1] * y) + m[2]) / den, ((m[3] * x + m[4] * y) + m[5]) / den


def project_recip(h9, x, y):
    """one reciprocal, two products (the quad corners of the chips)"""
    m = _m(h9)
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        r = f32(1.0) / ((m[6] * x + m[7] * y) + m[8])
        return ((m[0] * x + m[1] * y) + m[2]) * r, ((m[3] * x + m[4] * y) + m[5]) * r


def denominators(inv, xf, yf):
    m = _m(inv)
    with np.errstate(all="ignore"):
        return (m[6] * np.asarray(xf, np.float32) + m[7] * np.asarray(yf, np.float32)) + m[8]


def corners(w, h):
    return np.array([0, w - 1, w - 1, 0], np.float32), np.array([0, 0, h - 1, h - 1], np.float32)


def _box(X, Y, lo=BIG, hi=-BIG):
    """running minimum / maximum with strict comparisons in corner order (a NaN corner changes nothing)"""
    minX, minY, maxX, maxY = lo, lo, hi, hi
    for x, y in zip(X, Y):
        if x > maxX: maxX = x
        if x < minX: minX = x
        if y > maxY: maxY = y
        if y < minY: minY = y
    return minX, minY, maxX, maxY


def _extent(lo, hi):
    return int(f32(f32(hi - lo) + f32(1.5)))


def sample(img, ws_ch, xs, ys, ok, xi_shift=0):
    """bytes of the destination pixels `ok` of a [h, w, ch] (or [h, w]) image: truncating four-term bilinear.  xi_shift: a deliberately wrong
    neighbour (the cases' predicates use it to show that a case can tell)"""
    a = img if img.ndim == 3 else img[:, :, None]
    h, w, _ = a.shape
    x, y = xs[ok], ys[ok]
    xi, yi = x.astype(np.int32), y.astype(np.int32)
    p, q = (y - yi.astype(np.float32))[:, None], (x - xi.astype(np.float32))[:, None]
    xj = np.minimum(xi + xi_shift, w - 2)
    s00, s01 = a[yi, xj].astype(np.float32), a[yi, xj + 1].astype(np.float32)
    s10, s11 = a[yi + 1, xj].astype(np.float32), a[yi + 1, xj + 1].astype(np.float32)
    omp, omq = f32(1.0) - p, f32(1.0) - q
    v = (((s00 * omp) * omq + (s01 * omp) * q) + (s10 * p) * omq) + (s11 * p) * q
    return v.astype(np.int32).astype(np.uint8)


def _has_sample(xs, ys, w, h):
    with np.errstate(invalid="ignore"):
        return (xs >= 0) & (xs < f32(w - 1)) & (ys >= 0) & (ys < f32(h - 1))


def image_projection_transform(img, h9, inv, xi_shift=0):
    """(buffer [dh, dws], dw, dh, dws) and the source coordinates (xs, ys, ok) of every destination pixel; None when the result is empty"""
    h, w = img.shape[:2]
    ch = img.shape[2] if img.ndim == 3 else 1
    X, Y = project(h9, *corners(w, h))
    minX, minY, maxX, maxY = _box(X, Y)
    nw, nh = _extent(minX, maxX), _extent(minY, maxY)
    if nw <= 0 or nh <= 0:
        return None
    nws = (nw * ch + 3) // 4 * 4
    dx, dy = -minX, -minY
    xf = (np.arange(nw, dtype=np.float32) - dx)[None, :].repeat(nh, 0)
    yf = (np.arange(nh, dtype=np.float32) - dy)[:, None].repeat(nw, 1)
    xs, ys = project(inv, xf, yf)
    ok = _has_sample(xs, ys, w, h)
    out = np.zeros((nh, nw, ch), np.uint8)
    out[ok] = sample(img, None, xs, ys, ok, xi_shift)
    buf = np.zeros((nh, nws), np.uint8)
    buf[:, :nw * ch] = out.reshape(nh, nw * ch)
    return (buf, nw, nh, nws), (xs, ys, ok, xf, yf)


def mosaic_images_refined(imgs, h9s, invs):
    """invs[k]: the inverse of frame k, or None where it has none (the frame then counts for the canvas size and gives no pixel).
    Returns (canvas [ch, cws], cw, ch, cws), winner [ch, cw] (frame index or -1) and nan_seen: a source coordinate inside some frame's
    box was NaN"""
    h9s = np.asarray(h9s, np.float32).reshape(-1, 9)
    live = [k for k in range(len(imgs)) if h9s[k, 8] != 0]
    minX, minY, maxX, maxY = BIG, BIG, -BIG, -BIG
    proj = {}
    for k in live:
        hh, ww = imgs[k].shape[:2]
        X, Y = project(h9s[k], *corners(ww, hh))
        proj[k] = (X, Y)
        for x, y in zip(X, Y):
            if x < minX: minX = x
            if x > maxX: maxX = x
            if y < minY: minY = y
            if y > maxY: maxY = y
    mw, mh = _extent(minX, maxX), _extent(minY, maxY)
    if mw <= 0 or mh <= 0:
        return None
    mws = (mw * 3 + 3) & ~3
    dGX, dGY = -minX, -minY
    canvas = np.zeros((mh, mw, 3), np.uint8)
    winner = np.full((mh, mw), -1, np.int32)
    nan_seen = False
    for k in live:
        if invs[k] is None:
            continue
        hh, ww = imgs[k].shape[:2]
        X, Y = proj[k]
        X = X + (f32(0) + dGX); Y = Y + (f32(0) + dGY)
        bminX, bminY, bmaxX, bmaxY = _box(X, Y)
        x0, x1 = max(int(f32(bminX - f32(0.5))), 0), min(int(f32(bmaxX + f32(0.5))), mw - 1)
        y0, y1 = max(int(f32(bminY - f32(0.5))), 0), min(int(f32(bmaxY + f32(0.5))), mh - 1)
        if x1 < x0 or y1 < y0:
            continue
        xf = (np.arange(x0, x1 + 1).astype(np.float32) - dGX)[None, :].repeat(y1 - y0 + 1, 0)
        yf = (np.arange(y0, y1 + 1).astype(np.float32) - dGY)[:, None].repeat(x1 - x0 + 1, 1)
        xs, ys = project(invs[k], xf, yf)
        nan_seen = nan_seen or bool(np.isnan(xs).any() or np.isnan(ys).any())
        ok = _has_sample(xs, ys, ww, hh)
        canvas[y0:y1 + 1, x0:x1 + 1][ok] = sample(imgs[k], None, xs, ys, ok)
        winner[y0:y1 + 1, x0:x1 + 1][ok] = k
    buf = np.zeros((mh, mws), np.uint8)
    buf[:, :mw * 3] = canvas.reshape(mh, mw * 3)
    return (buf, mw, mh, mws), winner, nan_seen


def chips_and_masks(imgs, h9s, invs, keep=None, find_masks=True):
    """the chips' layout (a canvas that always contains the origin), one chip + validity mask per kept frame, and the ownership; the same
    dictionary as Oracle.chips_and_masks plus nan_seen and best (the owner map, chip position or -1)"""
    h9s = np.asarray(h9s, np.float32).reshape(-1, 9)
    n = len(imgs)
    kept = [k for k in range(n) if (keep is None or keep[k]) and h9s[k, 8] != 0]
    zero = f32(0)
    minX, minY, maxX, maxY = zero, zero, zero, zero
    boxes = {}
    for k in kept:
        hh, ww = imgs[k].shape[:2]
        X, Y = project(h9s[k], *corners(ww, hh))
        boxes[k] = _box(X, Y)
        for x, y in zip(X, Y):
            if x > maxX: maxX = x
            if x < minX: minX = x
            if y > maxY: maxY = y
            if y < minY: minY = y
    dGx, dGy = -minX, -minY
    cw, ch = _extent(minX, maxX), _extent(minY, maxY)
    from tests.oracle_lib import CHIPINFO
    chips = np.zeros(len(kept), CHIPINFO)
    cimgs, valid = [], []
    nan_seen = False
    for v, k in enumerate(kept):
        hh, ww = imgs[k].shape[:2]
        b = boxes[k]
        bX, bY, eX, eY = b[0] + dGx, b[1] + dGy, b[2] + dGx, b[3] + dGy
        begX, begY, endX, endY = int(bX), int(bY), int(f32(eX + f32(0.5))), int(f32(eY + f32(0.5)))
        sx, sy = f32(begX) - bX, f32(begY) - bY
        w, h = endX - begX + 1, endY - begY + 1
        c = chips[v]
        c["x0"], c["y0"], c["w"], c["h"], c["img"], c["sx"], c["sy"] = begX, begY, w, h, k, sx, sy
        tx, ty = project_recip(h9s[k], *corners(ww, hh))
        c["quad"][0::2] = ((tx + dGx) + sx) - f32(begX)
        c["quad"][1::2] = ((ty + dGy) + sy) - f32(begY)
        xT = (((np.arange(w, dtype=np.float32) - dGx) - sx) + f32(begX))[None, :].repeat(h, 0)
        yT = (((np.arange(h, dtype=np.float32) - dGy) - sy) + f32(begY))[:, None].repeat(w, 1)
        xs, ys = project(invs[k], xT, yT)
        nan_seen = nan_seen or bool(np.isnan(xs).any() or np.isnan(ys).any())
        ok = _has_sample(xs, ys, ww, hh)
        px = np.zeros((h, w, 3), np.uint8)
        px[ok] = sample(imgs[k], None, xs, ys, ok)
        chip = np.zeros((h, (3 * w + 3) & ~3), np.uint8); chip[:, :3 * w] = px.reshape(h, 3 * w)
        mask = np.zeros((h, (w + 3) & ~3), np.uint8); mask[:, :w] = ok * np.uint8(255)
        cimgs.append(chip); valid.append(mask)
    out = dict(cw=cw, ch=ch, dG=np.array([dGx, dGy], np.float32), chips=chips, chip_imgs=cimgs, valid=valid, masks=[m.copy() for m in valid],
               nan_seen=nan_seen, best=None)
    if find_masks and len(kept):
        out["masks"], out["best"] = ownership(valid, chips, cw, ch)
    return out


def _line(x1, y1, x2, y2):
    """a x + b y + c = 0 through two points; a vertical line when the x's differ by less than 1e-6"""
    with np.errstate(all="ignore"):
        if abs(float(f32(x1 - x2))) < 0.000001:
            return f32(1), f32(0), -x1
        a = f32(y1 - y2) / f32(x1 - x2)
        return a, f32(-1), f32(y1 - f32(a * x1))


def edge_lines(quad):
    q = [f32(v) for v in quad]
    return [_line(q[2 * i], q[2 * i + 1], q[(2 * i + 2) % 8], q[(2 * i + 3) % 8]) for i in range(4)]


def distance_map(mask, chip):
    """normalised distance to the nearest quad edge on the chip's pixels (0 where the mask is 0, before the division), and the maximum"""
    w, h = int(chip["w"]), int(chip["h"])
    cc = np.arange(w, dtype=np.float32)[None, :]
    rr = np.arange(h, dtype=np.float32)[:, None]
    near = np.full((h, w), BIG, np.float32)
    with np.errstate(all="ignore"):
        for a, b, c in edge_lines(chip["quad"]):
            r = f32(1.0) / np.sqrt(f32(a * a + b * b))
            d = np.abs((a * cc + b * rr) + c) * r
            near = np.where(d < near, d, near)
        on = mask[:, :w] != 0
        dist = np.where(on, near, f32(0))
        vals = dist[on]
        vals = vals[~np.isnan(vals)]             # the maximum is a chain of `v > top` from 0: a NaN never becomes it
        top = f32(max(vals.max(), 0)) if len(vals) else f32(0)
        return dist / top, top


def ownership(valid, chips, cw, ch, upto=None, strict=True):
    """(masks, best): best[y, x] = position of the owning chip or -1; only the first `upto` chips take part when it is given.  strict=False is
    the WRONG rule (`>=`: the last of equals wins, a value of 0 finds an owner), for the tests that show that the cases can tell"""
    n = len(chips) if upto is None else min(upto, len(chips))
    bd = np.zeros((ch, cw), np.float32)
    best = np.full((ch, cw), -1, np.int32)
    for k in range(n):
        c = chips[k]
        x0, y0, w, h = int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])
        d, _ = distance_map(valid[k], c)
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, ch), max(x0, 0), min(x0 + w, cw)
        if yb <= ya or xb <= xa:
            continue
        sub = d[ya - y0:yb - y0, xa - x0:xb - x0]
        with np.errstate(invalid="ignore"):
            take = (sub > bd[ya:yb, xa:xb]) if strict else (sub >= bd[ya:yb, xa:xb])
        bd[ya:yb, xa:xb][take] = sub[take]
        best[ya:yb, xa:xb][take] = k
    masks = []
    for k in range(len(chips)):
        c = chips[k]
        x0, y0, w, h = int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])
        m = np.zeros_like(valid[k])
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, ch), max(x0, 0), min(x0 + w, cw)
        if yb > ya and xb > xa:
            m[ya - y0:yb - y0, xa - x0:xb - x0] = (best[ya:yb, xa:xb] == k) * np.uint8(255)
        masks.append(m)
    return masks, best

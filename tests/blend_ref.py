"""numpy restatement of the multiband blend, written from the definition at the top of oracle/oracle_blend.c (REDUCE / EXPAND / feed / blend
and the level-count rule) -- a second statement of the arithmetic, independent of the oracle's loop nest and of csrc/blend.hip.

Integers are int64 throughout ((v + 128) >> 8, (v + 32) >> 6, saturation and 16-bit wrap-around applied where the definition applies them);
weights are np.float32 arrays and every product and sum is a separate float32 operation in the stated order; (short)(float) conversions are
np.trunc.  Whole-array operations only: one chip of a few hundred pixels squared takes milliseconds.
"""
import math

import numpy as np

F = np.float32


def reflect101(p, n):
    """BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) of integer positions p into 0 .. n - 1, any distance"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q >= n, 2 * n - 2 - q, q)


def reflect(p, n):
    """BORDER_REFLECT (fedcba|abcdefgh|hgfedcb: the edge pixel is repeated), any distance"""
    p = np.asarray(p, np.int64)
    q = np.mod(p, 2 * n)
    return np.where(q >= n, 2 * n - 1 - q, q)


def sat16(v):
    return np.clip(v, -32768, 32767)


def _taps(n):
    x = np.arange(n // 2, dtype=np.int64)
    return [reflect101(2 * x + d, n) for d in (-2, -1, 0, 1, 2)]


def reduce16(s):
    """REDUCE of an [h, w, C] integer array (h, w even): rows then columns, (v + 128) >> 8"""
    s = np.asarray(s, np.int64)
    h, w = s.shape[:2]
    a, b, c, d, e = _taps(w)
    r = s[:, c] * 6 + (s[:, b] + s[:, d]) * 4 + s[:, a] + s[:, e]
    a, b, c, d, e = _taps(h)
    v = r[c] * 6 + (r[b] + r[d]) * 4 + r[a] + r[e]
    return (v + 128) >> 8


def reduce_f(s):
    """REDUCE of an [h, w] float32 array: s[2x]*6 + (s[2x-1] + s[2x+1])*4 + s[2x-2] + s[2x+2], left to right, the same over the rows,
    then * (1 / 256) -- every operation rounded to float32"""
    s = np.asarray(s, F)
    h, w = s.shape
    a, b, c, d, e = _taps(w)
    r = s[:, c] * F(6)
    t = s[:, b] + s[:, d]
    t = t * F(4)
    r = r + t
    r = r + s[:, a]
    r = r + s[:, e]
    a, b, c, d, e = _taps(h)
    v = r[c] * F(6)
    t = r[b] + r[d]
    t = t * F(4)
    v = v + t
    v = v + r[a]
    v = v + r[e]
    v = v * F(1.0 / 256.0)
    assert v.dtype == F
    return v


def _expand_h(s):
    """horizontal EXPAND of [h, w, C] into [h, 2w, C] (before the >> 6): the stated interior values and border pairs"""
    h, w = s.shape[:2]
    out = np.zeros((h, 2 * w) + s.shape[2:], np.int64)
    if w == 1:
        out[:, 0] = s[:, 0] * 8
        out[:, 1] = s[:, 0] * 8
        return out
    out[:, 2:2 * w - 2:2] = s[:, :-2] + s[:, 1:-1] * 6 + s[:, 2:]
    out[:, 3:2 * w - 2:2] = (s[:, 1:-1] + s[:, 2:]) * 4
    out[:, 0] = s[:, 0] * 6 + s[:, 1] * 2
    out[:, 1] = (s[:, 0] + s[:, 1]) * 4
    out[:, 2 * w - 2] = s[:, w - 2] + s[:, w - 1] * 7
    out[:, 2 * w - 1] = s[:, w - 1] * 8
    return out


def expand16(s):
    """EXPAND of [h, w, C] to [2h, 2w, C]: even = r[y-1] + 6 r[y] + r[y+1], odd = 4 (r[y] + r[y+1]) over the horizontally expanded rows,
    row(-1) := row(1), row(h) := row(h-1) (so a single row stands for all three); (v + 32) >> 6"""
    s = np.asarray(s, np.int64)
    h = s.shape[0]
    r = _expand_h(s)
    y = np.arange(h)
    up = np.where(y == 0, min(1, h - 1), y - 1)
    dn = np.where(y == h - 1, h - 1, y + 1)
    out = np.zeros((2 * h,) + r.shape[1:], np.int64)
    out[0::2] = r[up] + r * 6 + r[dn]
    out[1::2] = (r + r[dn]) * 4
    return (out + 32) >> 6


def level_count(W, H, band):
    """bands = min(band, ceil(log2(max(W, H)))), with the logarithm taken as log(n) / log(2.0) in double precision"""
    nb = int(math.ceil(math.log(float(max(W, H))) / math.log(2.0)))
    return max(0, min(nb, int(band)))


def feed_geometry(x0, y0, w, h, W, H, nb):
    """region of one chip: (tlx, tly, rw, rh, left, top, dx, dy).  The chip rectangle grown by 3 * 2^bands, clipped to the padded canvas,
    its top-left snapped down and its size rounded up to multiples of 2^bands, then pulled back by (dx, dy) when that leaves the canvas."""
    al = 1 << nb
    Wp, Hp = (W + al - 1) // al * al, (H + al - 1) // al * al
    gap = 3 * al
    out = []
    for p0, n, P in ((x0, w, Wp), (y0, h, Hp)):
        tl = max(0, p0 - gap)
        br = min(P, p0 + n + gap)
        tl = (tl >> nb) << nb
        size = br - tl
        size += (al - size % al) % al
        d = max(tl + size - P, 0)
        tl -= d
        out.append((tl, size, p0 - tl, d))
    (tlx, rw, left, dx), (tly, rh, top, dy) = out
    return tlx, tly, rw, rh, left, top, dx, dy


def chip_pyramids(chip, mask, w, h, geo, nb):
    """(Laplacian levels int64 [rh >> l, rw >> l, 3], weight levels float32) of one chip over its region"""
    tlx, tly, rw, rh, left, top = geo[:6]
    px = np.asarray(chip, np.uint8)[:h, :3 * w].reshape(h, w, 3).astype(np.int64)
    sy = reflect(np.arange(rh) - top, h)
    sx = reflect(np.arange(rw) - left, w)
    g = [px[sy][:, sx]]
    wt = np.zeros((rh, rw), F)
    wt[top:top + h, left:left + w] = np.asarray(mask, np.uint8)[:h, :w].astype(F) * F(1.0 / 255.0)
    wts = [wt]
    for l in range(nb):
        g.append(reduce16(g[l]))
        wts.append(reduce_f(wts[l]))
    lap = [sat16(g[l] - expand16(g[l + 1])) for l in range(nb)] + [g[nb]]
    return lap, wts


def multiband_blend(rects, chips, masks, W, H, band, wide_accumulator=False, stats=None):
    """rects: (x0, y0, w, h) per chip; chips: u8 rows of >= 3w bytes (BGR); masks: u8 rows of >= w bytes.  Returns (out u8 [H, (3W+3)&~3], bands).
    wide_accumulator: the canvas Laplacian is NOT wrapped to 16 bits on each add (what a wider accumulator would compute) -- a variant for
    the tests, not the definition.  stats (a dict): 'left_int16' = some canvas sum left the int16 range before the cast."""
    nb = level_count(W, H, band)
    al = 1 << nb
    Wp, Hp = (W + al - 1) // al * al, (H + al - 1) // al * al
    dl = [np.zeros((Hp >> l, Wp >> l, 3), np.int64) for l in range(nb + 1)]
    dw = [np.zeros((Hp >> l, Wp >> l), F) for l in range(nb + 1)]
    left16 = False
    for (x0, y0, w, h), chip, mask in zip(rects, chips, masks):
        geo = feed_geometry(int(x0), int(y0), int(w), int(h), W, H, nb)
        tlx, tly, rw, rh = geo[:4]
        lap, wts = chip_pyramids(chip, mask, int(w), int(h), geo, nb)
        for l in range(nb + 1):
            ys, xs = slice(tly >> l, (tly + rh) >> l), slice(tlx >> l, (tlx + rw) >> l)
            prod = lap[l].astype(F) * wts[l][:, :, None]
            assert prod.dtype == F
            s = dl[l][ys, xs] + np.trunc(prod).astype(np.int64)
            left16 = left16 or bool((s < -32768).any() or (s > 32767).any())
            dl[l][ys, xs] = s if wide_accumulator else s.astype(np.int16).astype(np.int64)
            dw[l][ys, xs] = dw[l][ys, xs] + wts[l]
    if stats is not None:
        stats["left_int16"] = left16
    for l in range(nb + 1):
        q = dl[l].astype(F) / (dw[l] + F(1e-5))[:, :, None]
        assert q.dtype == F
        dl[l] = np.trunc(q).astype(np.int64).astype(np.int16).astype(np.int64)
    for l in range(nb - 1, -1, -1):
        dl[l] = sat16(expand16(dl[l + 1]) + dl[l])
    res = np.where((dw[0] > F(1e-5))[:, :, None], np.clip(dl[0], 0, 255), 0)[:H, :W]
    out = np.zeros((H, (W * 3 + 3) & ~3), np.uint8)
    out[:, :3 * W] = res.reshape(H, 3 * W).astype(np.uint8)
    return out, nb

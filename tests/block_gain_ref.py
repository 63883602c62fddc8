"""numpy restatement of block gain compensation (include/mi355_mosaic.h, "block gain compensation"; csrc/gain.hip), written from the contract.

Source coordinates come from tests/warp_ref.py (inverse, project, _has_sample: the refined render's map, equal to the oracle bit for bit);
the cells come from them.  Samples come either from the oracle's refined render as in tests/gain_ref.py (frame_sample_maps) or from
warp_ref.sample (sample_maps, no oracle needed).  Statistics are integer sums, the dense normal equations (gain_ref.normal_equations over the
nodes (frame, cell)) go through np.linalg.solve, smoothing is the separable [1/4, 1/2, 1/4] filter in float64 and the apply is integer.
"""
import numpy as np

from tests import gain_ref as gr
from tests import warp_ref as wr

f32 = np.float32
REC = np.dtype([("pair", "<i4"), ("cell_a", "<i4"), ("cell_b", "<i4"), ("reserved", "<i4"), ("n", "<i8"), ("sum_a", "<i8", (3,)), ("sum_b", "<i8", (3,))])
NODE_STATS = np.dtype([("a", "<i8"), ("b", "<i8"), ("n", "<i8"), ("sum_a", "<i8", (3,)), ("sum_b", "<i8", (3,))])


def coord_maps(sizes, h9s, eps=1e-12):
    """sizes: [(w, h)].  Per frame None (the render skips it) or (xs, ys, ok) on the whole canvas [ch, cw]: the source coordinate the refined
    render maps each canvas pixel to (float32; NaN outside the frame's clipped box) and whether the frame has a sample there.  Also (cw, ch)."""
    n = len(sizes)
    h9s = np.asarray(h9s, np.float32).reshape(n, 9)
    live = [k for k in range(n) if h9s[k, 8] != 0]
    minX, minY, maxX, maxY = wr.BIG, wr.BIG, -wr.BIG, -wr.BIG
    proj = {}
    for k in live:
        X, Y = wr.project(h9s[k], *wr.corners(*sizes[k]))
        proj[k] = (X, Y)
        for x, y in zip(X, Y):
            if x < minX: minX = x
            if x > maxX: maxX = x
            if y < minY: minY = y
            if y > maxY: maxY = y
    mw, mh = wr._extent(minX, maxX), wr._extent(minY, maxY)
    dGX, dGY = -minX, -minY
    out = [None] * n
    for k in live:
        inv = wr.inverse(h9s[k], eps)
        if inv is None:
            continue
        ww, hh = sizes[k]
        X, Y = proj[k]
        X = X + (f32(0) + dGX); Y = Y + (f32(0) + dGY)
        bminX, bminY, bmaxX, bmaxY = wr._box(X, Y)
        x0, x1 = max(int(f32(bminX - f32(0.5))), 0), min(int(f32(bmaxX + f32(0.5))), mw - 1)
        y0, y1 = max(int(f32(bminY - f32(0.5))), 0), min(int(f32(bmaxY + f32(0.5))), mh - 1)
        if x1 < x0 or y1 < y0:
            continue
        xf = (np.arange(x0, x1 + 1).astype(np.float32) - dGX)[None, :].repeat(y1 - y0 + 1, 0)
        yf = (np.arange(y0, y1 + 1).astype(np.float32) - dGY)[:, None].repeat(x1 - x0 + 1, 1)
        xs, ys = wr.project(inv, xf, yf)
        XS = np.full((mh, mw), np.nan, np.float32); YS = np.full((mh, mw), np.nan, np.float32)
        XS[y0:y1 + 1, x0:x1 + 1] = xs; YS[y0:y1 + 1, x0:x1 + 1] = ys
        out[k] = (XS, YS, wr._has_sample(XS, YS, ww, hh))
    return out, (mw, mh)


def sample_maps(imgs, coords):
    """gain_ref.frame_sample_maps without the oracle: (samples [ch, cw, 3] int64, cover [ch, cw] bool) per frame through warp_ref.sample"""
    out = []
    for img, c in zip(imgs, coords):
        if c is None:
            out.append(None)
            continue
        xs, ys, ok = c
        samp = np.zeros(ok.shape + (3,), np.int64)
        samp[ok] = wr.sample(img, None, xs, ys, ok)
        out.append((samp, ok))
    return out


def cells_of(coord, w, h, gx, gy):
    """cell index [ch, cw] of the frame's sample (garbage where it has none)"""
    xs, ys, ok = coord
    xi = np.where(ok, xs, 0).astype(np.int64); yi = np.where(ok, ys, 0).astype(np.int64)
    return ((yi * gy) // h) * gx + (xi * gx) // w


def stats_ref(maps, coords, sizes, pairs, step, gx, gy):
    """(REC records sorted by (pair, cell_a, cell_b), cell_cover [n, cells] int64)"""
    n, cells = len(maps), gx * gy
    shape = next(m for m in maps if m is not None)[1].shape
    L = gr.lattice(shape[0], shape[1], step)
    cell = [None if coords[k] is None else cells_of(coords[k], sizes[k][0], sizes[k][1], gx, gy) for k in range(n)]
    cover = np.zeros((n, cells), np.int64)
    for k in range(n):
        if maps[k] is not None:
            cover[k] = np.bincount(cell[k][maps[k][1] & L], minlength=cells)
    recs = []
    for p, (a, b) in enumerate(pairs):
        if maps[a] is None or maps[b] is None:
            continue
        both = maps[a][1] & maps[b][1] & L
        if not both.any():
            continue
        key = cell[a][both] * cells + cell[b][both]
        uniq, inv = np.unique(key, return_inverse=True)
        r = np.zeros(len(uniq), REC)
        r["pair"], r["cell_a"], r["cell_b"] = p, uniq // cells, uniq % cells
        r["n"] = np.bincount(inv, minlength=len(uniq))
        for c in range(3):                                          # integer sums below 2^53: exact as float64 weights
            r["sum_a"][:, c] = np.bincount(inv, weights=maps[a][0][both][:, c], minlength=len(uniq))
            r["sum_b"][:, c] = np.bincount(inv, weights=maps[b][0][both][:, c], minlength=len(uniq))
        recs.append(r)
    return (np.concatenate(recs) if recs else np.zeros(0, REC)), cover


def node_stats(recs, pairs, cells):
    """the records as pairs between nodes (frame * cells + cell): what gain_ref.normal_equations takes"""
    ab = np.asarray(pairs, np.int64).reshape(-1, 2)
    st = np.zeros(len(recs), NODE_STATS)
    st["a"] = ab[recs["pair"], 0] * cells + recs["cell_a"]
    st["b"] = ab[recs["pair"], 1] * cells + recs["cell_b"]
    st["n"], st["sum_a"], st["sum_b"] = recs["n"], recs["sum_a"], recs["sum_b"]
    return st


def normal_equations(recs, pairs, cell_cover, **kw):
    cover = np.asarray(cell_cover, np.int64)
    return gr.normal_equations(node_stats(recs, pairs, cover.shape[1]), cover.reshape(-1), **kw)


def solve_ref(recs, pairs, cell_cover, gx, gy, **kw):
    """exact node gains [n, gy, gx, 3] float64 before smoothing (nodes without an equation: 1)"""
    cover = np.asarray(cell_cover, np.int64)
    g = gr.solve_ref(node_stats(recs, pairs, cover.shape[1]), cover.reshape(-1), **kw)
    return g.reshape(cover.shape[0], gy, gx, 3)


def smooth_ref(g, passes):
    """`passes` times [1/4, 1/2, 1/4] along x then along y on [n, gy, gx, 3] float64, edges replicated"""
    g = np.asarray(g, np.float64)
    for _ in range(passes):
        e = np.concatenate([g[:, :, :1], g, g[:, :, -1:]], axis=2)
        g = 0.25 * e[:, :, :-2] + 0.5 * e[:, :, 1:-1] + 0.25 * e[:, :, 2:]
        e = np.concatenate([g[:, :1], g, g[:, -1:]], axis=1)
        g = 0.25 * e[:, :-2] + 0.5 * e[:, 1:-1] + 0.25 * e[:, 2:]
    return g


def gains_ref(recs, pairs, cell_cover, gx, gy, smooth, **kw):
    return smooth_ref(solve_ref(recs, pairs, cell_cover, gx, gy, **kw), smooth).astype(np.float32)


def _axis(nx, g):
    x = np.arange(nx, dtype=np.int64)
    num = np.clip((2 * x + 1) * g - nx, 0, 2 * nx * (g - 1))
    i0 = num // (2 * nx)
    f = ((num % (2 * nx)) * 256) // (2 * nx)
    return i0, np.minimum(i0 + 1, g - 1), f


def apply_ref(img, gmap):
    """the header's integer apply of a [gy, gx, 3] float32 map on an h x w x 3 image"""
    gmap = np.asarray(gmap, np.float32)
    gy, gx, _ = gmap.shape
    h, w, _ = img.shape
    q = np.clip(np.floor(gmap.astype(np.float64) * 4096 + 0.5), 0, 32767).astype(np.int64)
    i0, i1, fx = _axis(w, gx)
    j0, j1, fy = _axis(h, gy)
    R = (256 - fy)[:, None, None] * q[j0] + fy[:, None, None] * q[j1]              # [h, gx, 3]
    G = (256 - fx)[None, :, None] * R[:, i0] + fx[None, :, None] * R[:, i1]        # [h, w, 3]
    assert G.max() < 2 ** 31
    Gq = (G + 128) >> 8
    return np.minimum(255, (Gq * img.astype(np.int64) + (1 << 19)) >> 20).astype(np.uint8)


def overlap_mad(maps, pairs, step):
    """mean absolute difference of the two frames' samples over the lattice points of the listed pairs' overlaps"""
    shape = next(m for m in maps if m is not None)[1].shape
    L = gr.lattice(shape[0], shape[1], step)
    tot, cnt = 0.0, 0
    for a, b in pairs:
        if maps[a] is None or maps[b] is None:
            continue
        both = maps[a][1] & maps[b][1] & L
        tot += float(np.abs(maps[a][0][both] - maps[b][0][both]).sum())
        cnt += 3 * int(both.sum())
    return tot / max(cnt, 1)


def ten_frames():
    """the 10-frame 320 x 240 case of tests/test_gpu_gain.py: affine and projective frames, a skipped one, a listed pair without overlap, clipped boxes"""
    from tests.synth import texture, warp_cases
    Hs = warp_cases()
    n = 10
    imgs = [(texture(320, 240, 40 + k).astype(np.float64) * (0.88 + 0.03 * k)).clip(0, 255).astype(np.uint8) for k in range(n)]
    h9s = np.zeros((n, 9), np.float32)
    off = [(0, 0), (140, 10), (280, -20), (60, 150), (200, 170), (330, 140), (-40, 90), (120, 60), (250, 90), (2000, 0)]
    for k in range(n):
        h9s[k] = Hs[[0, 2, 1, 3, 4, 5, 2, 3, 1, 0][k]]
        h9s[k, 2] += off[k][0]
        h9s[k, 5] += off[k][1]
    h9s[8, 8] = 0.0                                         # skipped by the render
    pairs = [(0, 1), (1, 2), (0, 3), (3, 4), (4, 5), (1, 4), (2, 5), (0, 6), (6, 3), (7, 0), (7, 1), (7, 4), (3, 7), (8, 7), (0, 9), (5, 9), (2, 8)]
    return imgs, h9s, pairs


def vignette_frames(n=12, w=256, h=192, seed=11):
    """n frames of w x h cut by integer translation from one scene (3 rows of n / 3, about 40 % overlap), each multiplied by 1 - 0.3 r^2 (r the
    distance from the frame centre over the half diagonal) and by a per-frame gain; (imgs, h9s, pairs of neighbours)"""
    rng = np.random.default_rng(seed)
    per_row = n // 3
    dx, dy = int(0.6 * w), int(0.6 * h)
    SW, SH = dx * (per_row - 1) + w + 8, dy * 2 + h + 8
    yy, xx = np.mgrid[0:SH, 0:SW]
    scene = np.stack([150 + 40 * np.sin(xx * 0.021 * (c + 1) + c) * np.cos(yy * 0.017 + 2 * c) + rng.integers(-6, 7, (SH, SW)) for c in range(3)], axis=2)
    fy, fx = np.mgrid[0:h, 0:w]
    r2 = (((fx - (w - 1) / 2) ** 2 + (fy - (h - 1) / 2) ** 2) / (((w - 1) / 2) ** 2 + ((h - 1) / 2) ** 2))[:, :, None]
    gains = rng.uniform(0.85, 1.15, n)
    imgs, h9s, pos = [], np.zeros((n, 9), np.float32), []
    for k in range(n):
        ox, oy = dx * (k % per_row) + int(rng.integers(0, 8)), dy * (k // per_row) + int(rng.integers(0, 8))
        pos.append((ox, oy))
        imgs.append((scene[oy:oy + h, ox:ox + w] * (1 - 0.3 * r2) * gains[k]).clip(0, 255).astype(np.uint8))
        h9s[k] = [1, 0, ox, 0, 1, oy, 0, 0, 1]
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n) if abs(pos[a][0] - pos[b][0]) < w - 8 and abs(pos[a][1] - pos[b][1]) < h - 8]
    return imgs, h9s, pairs


def vignette_ranking(apply_block, apply_frame, step=4, gx=8, gy=6):
    """the mean absolute overlap differences [block-compensated, frame-compensated, uncompensated] of the vignetting inputs.  The callbacks
    return the compensated images: apply_block(imgs, h9s, pairs, maps_ref) with the restatement's gain maps at hand, apply_frame(imgs, h9s,
    pairs, gains_ref) likewise with its per-frame gains."""
    imgs, h9s, pairs = vignette_frames()
    sizes = [(i.shape[1], i.shape[0]) for i in imgs]
    coords, _ = coord_maps(sizes, h9s)
    maps = sample_maps(imgs, coords)
    recs, cover = stats_ref(maps, coords, sizes, pairs, step, gx, gy)
    gmaps = gains_ref(recs, pairs, cover, gx, gy, 2)
    fr, fcov = gr.stats_ref(maps, pairs, step)
    fg = gr.solve_ref(gr.to_records(fr, pairs), fcov).astype(np.float32)
    return [overlap_mad(sample_maps(apply_block(imgs, h9s, pairs, gmaps), coords), pairs, step),
            overlap_mad(sample_maps(apply_frame(imgs, h9s, pairs, fg), coords), pairs, step),
            overlap_mad(maps, pairs, step)]

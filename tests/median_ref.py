"""numpy restatement of the median render (include/mi355_mosaic.h, "median render"; csrc/median.hip).

Built like tests/seamline_ref.py, from the oracle's refined render alone: gain_ref.frame_sample_maps gives every frame's sample bytes and cover
on the unchanged layout; a second call with every image replaced by its three-channel Wk image (feather_ref.wk_images) gives omega_k - 1.  Per
pixel the covering frames are sorted by (omega_k, k) -- one np.sort over packed keys, no running top-K -- the `depth` largest are the selected
set, and each channel of their samples is sorted for the median.
"""
import numpy as np

from tests import feather_ref as fr
from tests import gain_ref as gr
from tests import seamline_ref as sr

DEFAULT_DEPTH = 5
MAX_DEPTH = 9


def pick(maps, wmaps, depth):
    """(canvas [ch, cw, 3] uint8, spread [ch, cw] uint8, count [ch, cw] uint16, selected [depth, ch, cw] uint16 = frame + 1 in descending
    (omega, k) order, 0 where fewer frames cover, boundary_tie [ch, cw] bool: the depth-th and the (depth + 1)-th frame have the same omega)
    from per-frame (samples, cover) and the same maps of the Wk images"""
    depth = int(depth) or DEFAULT_DEPTH
    assert 1 <= depth <= MAX_DEPTH
    n = len(maps)
    shape = next(m for m in maps if m is not None)[1].shape
    keys = np.zeros((max(n, depth + 1),) + shape, np.int32)              # omega << 16 | k + 1 where frame k covers, else 0
    samp = np.zeros((n + 1,) + shape + (3,), np.uint8)                  # samp[k + 1]: frame k's samples; samp[0]: nobody
    for k, (m, wm) in enumerate(zip(maps, wmaps)):
        if m is None:
            continue
        s, cover = m
        om = (1 + wm[0][..., 0]) * cover
        assert om.max() <= 255 and n <= 65535
        keys[k] = (om << 16 | (k + 1)) * cover
        samp[k + 1] = s
    count = (keys > 0).sum(axis=0)
    keys = np.sort(keys, axis=0)[::-1]                                  # descending: distinct wherever non-zero
    top = keys[:depth]
    selected = top & 0xffff
    tie = (keys[depth] > 0) & ((keys[depth] >> 16) == (keys[depth - 1] >> 16))
    m = np.minimum(count, depth)
    assert np.array_equal((top > 0).sum(axis=0), m)
    vals = np.take_along_axis(samp, selected[..., None].astype(np.int64), axis=0).astype(np.int64)      # [depth, ch, cw, 3]
    vals[top == 0] = 256                                                # absent: sorts last
    v = np.sort(vals, axis=0)
    at = lambda idx: np.take_along_axis(v, np.broadcast_to(np.clip(idx, 0, depth - 1)[None, ..., None], (1,) + shape + (3,)), axis=0)[0]
    some = (m > 0)[..., None]
    out = np.where(some, (at((m - 1) >> 1) + at(m >> 1) + 1) >> 1, 0)
    spread = np.where(some, at(m - 1) - v[0], 0).max(axis=2)
    assert out.min() >= 0 and out.max() <= 255 and spread.min() >= 0 and spread.max() <= 255 and count.max() <= 65535
    return out.astype(np.uint8), spread.astype(np.uint8), count.astype(np.uint16), selected.astype(np.uint16), tie


def median_ref(orc, imgs, h9s, ramp=0, depth=0, maps=None, full=False):
    """(canvas [ch, cw, 3], spread [ch, cw] uint8, count [ch, cw] uint16); full: also (selected [depth, ch, cw], boundary_tie).  depth 0: the
    default, 5.  maps: gain_ref.frame_sample_maps(orc, imgs, h9s) when the caller already has it"""
    if maps is None:
        maps = gr.frame_sample_maps(orc, imgs, h9s)
    r = pick(maps, sr.weight_maps(orc, imgs, h9s, ramp, maps), depth)
    return r if full else r[:3]


def selected_samples(maps, selected):
    """(lo, hi) [ch, cw, 3]: the smallest and the largest selected sample per pixel and channel (255 / 0 where nothing is selected)"""
    shape = selected.shape[1:]
    lo, hi = np.full(shape + (3,), 255, np.int64), np.zeros(shape + (3,), np.int64)
    for k, m in enumerate(maps):
        if m is None:
            continue
        mine = (selected == k + 1).any(axis=0)[..., None]
        lo = np.where(mine, np.minimum(lo, m[0]), lo)
        hi = np.where(mine, np.maximum(hi, m[0]), hi)
    return lo, hi


def moving_object_case(w=64, h=48, block=10, colour=(250, 5, 240)):
    """five w x h frames cut from one tests.synth.texture scene at distinct integer offsets, pure integer translations as h9: every clean
    sample is the scene's byte exactly.  Frame 2 carries a block x block square of a constant colour -- something that was there in one
    exposure only -- inside the region at least three frames cover.  (clean imgs, dirty imgs, h9s, (bx, by) of the block on the canvas)"""
    from tests.synth import texture
    offs = [(0, 0), (9, 4), (17, 11), (5, 14), (13, 7)]
    W, H = w + max(o[0] for o in offs), h + max(o[1] for o in offs)
    scene = texture(W, H, seed=91)
    clean = [np.ascontiguousarray(scene[oy:oy + h, ox:ox + w]) for ox, oy in offs]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (len(offs), 1))
    for k, (ox, oy) in enumerate(offs):
        h9s[k, 2], h9s[k, 5] = ox, oy
    bx, by = 30, 22                                                     # canvas position of the block: min offset is (0, 0), so canvas = scene
    dirty = [c.copy() for c in clean]
    ox, oy = offs[2]
    dirty[2][by - oy:by - oy + block, bx - ox:bx - ox + block] = colour
    return clean, dirty, h9s, (bx, by, block)


def boundary_tie_case(w=40, h=64):
    """three equal w x h frames at dx = 0, 13, 6: at column 26, rows 13 .. 50, frame 2 is deepest (border distance 19) and frames 0 and 1 tie
    (13 each), so that with depth = 2 the index decides who is selected beside frame 2: frame 1.  (imgs, h9s, column, row slice)"""
    from tests.synth import texture
    imgs = [texture(w, h, seed=81 + k) for k in range(3)]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (3, 1))
    h9s[1, 2], h9s[2, 2] = 13, 6
    return imgs, h9s, 26, slice(13, 51)


def window_ref(orc, get_img, w, h, h9s, window, ramp=0, depth=0, threads=4):
    """bytes [wh, ww, 3], spread and count [wh, ww] of the canvas window (x0, y0, ww, wh) of a large survey (every frame w x h), the way
    seamline_ref.window_ref works: only the frames whose canvas box (grown by 2 px) reaches the window are rendered, each alone inside the
    full canvas geometry, once with its pixels and once as (Wk, 255, 255).  Returns (bytes, spread, count, number of frames rendered)."""
    from tests import oracle_lib as ol
    x0, y0, ww, wh = window
    n = len(h9s)
    h9s = np.asarray(h9s, np.float32).reshape(n, 9)
    c = np.array([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], np.float64).T
    boxes = []
    for k in range(n):
        if h9s[k, 8] == 0:
            boxes.append(None)
            continue
        p = h9s[k].reshape(3, 3).astype(np.float64) @ c
        p = p[:2] / p[2]
        boxes.append((p[0].min(), p[1].min(), p[0].max(), p[1].max()))
    live = [k for k in range(n) if boxes[k]]
    minx, miny = min(boxes[k][0] for k in live), min(boxes[k][1] for k in live)
    extreme = sorted({min(live, key=lambda k: boxes[k][0]), min(live, key=lambda k: boxes[k][1]),
                      max(live, key=lambda k: boxes[k][2]), max(live, key=lambda k: boxes[k][3])})
    sub = [k for k in live if boxes[k][0] - minx - 2 < x0 + ww and boxes[k][2] - minx + 2 > x0 and
           boxes[k][1] - miny - 2 < y0 + wh and boxes[k][3] - miny + 2 > y0]
    zero = np.zeros((h, w, 3), np.uint8)
    wimg = fr.wk_images([zero], ramp)[0].copy()
    wimg[..., 1:] = 255

    def one(k):
        others = [e for e in extreme if e != k]
        hs = h9s[others + [k]]
        cut = []
        for last in (get_img(k), wimg):
            rc, (canvas, cw, ch, cws) = orc.mosaic_images_refined([zero] * len(others) + [last], hs)
            assert rc == 0
            cut.append(canvas[y0:y0 + wh, 3 * x0:3 * (x0 + ww)].reshape(wh, ww, 3).astype(np.int64))
            del canvas
        return cut

    if not sub:
        return np.zeros((wh, ww, 3), np.uint8), np.zeros((wh, ww), np.uint8), np.zeros((wh, ww), np.uint16), 0
    # the window's frames in ascending caller order, renumbered: the order (omega, k) among them is unchanged
    maps, wmaps = [], []
    for samp, wc in ol.parallel_map(one, sub, threads=threads):
        maps.append((samp, wc[..., 1] != 0))
        wmaps.append((wc, wc[..., 1] != 0))
    out, spread, count, _, _ = pick(maps, wmaps, depth)
    return out, spread, count, len(sub)

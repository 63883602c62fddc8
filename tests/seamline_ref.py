"""numpy restatement of the seamline render (include/mi355_mosaic.h, "seamline render"; csrc/seamline.hip).

Built like tests/feather_ref.py, from the oracle's refined render alone: gain_ref.frame_sample_maps gives every frame's sample bytes and cover
on the unchanged layout; a second call with every image replaced by its three-channel Wk image (feather_ref.wk_images) gives omega_k - 1.  The
owner of a pixel is the lexicographic argmax of (omega_k, k) over the frames that cover it; the canvas takes the owner's sample.
"""
import os

import numpy as np

from tests import feather_ref as fr
from tests import gain_ref as gr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pick(maps, wmaps):
    """(canvas [ch, cw, 3] uint8, owner [ch, cw] uint16 = owning frame + 1 or 0, count [ch, cw] uint16, omega_max [ch, cw] int64, ties
    [ch, cw] bool: the winning omega is held by more than one frame) from per-frame (samples, cover) and the same maps of the Wk images"""
    shape = next(m for m in maps if m is not None)[1].shape
    best = np.zeros(shape, np.int64)                     # omega of the owner so far; 0: nobody (omega >= 1)
    ties = np.zeros(shape, bool)
    owner = np.zeros(shape, np.int64)
    count = np.zeros(shape, np.int64)
    out = np.zeros(shape + (3,), np.int64)
    for k, (m, wm) in enumerate(zip(maps, wmaps)):       # ascending k: an equal omega later in the walk is a larger k and wins
        if m is None:
            continue
        samp, cover = m
        om = (1 + wm[0][..., 0]) * cover
        assert om.max() <= 255
        eq = cover & (om == best)
        gt = om > best
        ties = np.where(gt, False, ties | eq)
        win = gt | eq
        best = np.where(win, om, best)
        owner = np.where(win, k + 1, owner)
        out = np.where(win[..., None], samp, out)
        count += cover
    assert out.min() >= 0 and out.max() <= 255 and count.max() <= 65535
    return out.astype(np.uint8), owner.astype(np.uint16), count.astype(np.uint16), best, ties


def weight_maps(orc, imgs, h9s, ramp, maps):
    wmaps = gr.frame_sample_maps(orc, fr.wk_images(imgs, ramp), h9s)
    for m, wm in zip(maps, wmaps):
        # the Wk image is zero on the frame's border: its own 255-render must still give the frame's cover
        assert (m is None) == (wm is None) and (m is None or np.array_equal(m[1], wm[1]))
    return wmaps


def seamline_ref(orc, imgs, h9s, ramp=0, maps=None, full=False):
    """(canvas [ch, cw, 3], owner [ch, cw] uint16, count [ch, cw] uint16); full: also (omega_max, ties).  maps:
    gain_ref.frame_sample_maps(orc, imgs, h9s) when the caller already has it"""
    if maps is None:
        maps = gr.frame_sample_maps(orc, imgs, h9s)
    r = pick(maps, weight_maps(orc, imgs, h9s, ramp, maps))
    return r if full else r[:3]


def top_frame(maps):
    """the refined render's choice: the highest covering index + 1 (0: nobody)"""
    shape = next(m for m in maps if m is not None)[1].shape
    top = np.zeros(shape, np.int64)
    for k, m in enumerate(maps):
        if m is not None:
            top = np.where(m[1], k + 1, top)
    return top


def golden_survey(step=2):
    """the reference's committed run (tests/golden: DSC00004 .. DSC00023.JPG and the transforms of tran0.txt, image 0 at the identity),
    decimated by `step` (every step-th pixel, translations divided by step) so that the per-frame maps of 20 frames stay small: (imgs, h9s)"""
    from PIL import Image
    imgs = [np.ascontiguousarray(np.array(Image.open(os.path.join(GOLD, "DSC%05d.JPG" % (4 + k))).convert("RGB"))[::step, ::step, ::-1]) for k in range(20)]
    rows = np.loadtxt(os.path.join(GOLD, "tran0.txt"), dtype=np.float64).reshape(19, 9)
    h9s = np.zeros((20, 9), np.float64)
    h9s[0] = np.eye(3).reshape(9)
    h9s[1:, :8] = rows[:, :8]
    h9s[:, 8] = 1.0
    h9s[:, [2, 5]] /= step
    h9s[:, [6, 7]] *= step
    return imgs, h9s.astype(np.float32)


def tie_case(w=40, h=64, dx=13, dy=0):
    """two equal w x h frames under integer translations dx apart, w - 1 + dx even: the column x = (w - 1 + dx) / 2 has the same border
    distance in both frames (x in frame 0, x - dx = w - 1 - x in frame 1), hence the same omega: the index decides.  (imgs, h9s, midline x)"""
    from tests.synth import texture
    assert (w - 1 + dx) % 2 == 0 and 0 < dx < w - 2
    imgs = [texture(w, h, seed=71), texture(w, h, seed=72)]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    h9s[1, 2], h9s[1, 5] = dx, dy
    return imgs, h9s, (w - 1 + dx) // 2


def window_ref(orc, get_img, w, h, h9s, window, ramp=0, threads=4):
    """bytes [wh, ww, 3], owner and count [wh, ww] of the canvas window (x0, y0, ww, wh) of a large survey (every frame w x h), the way
    feather_ref.window_ref works: only the frames whose canvas box (grown by 2 px) reaches the window are rendered, each alone inside the full
    canvas geometry -- the frames that define the canvas box ride along as zero images -- once with its pixels and once as (Wk, 255, 255):
    channel 0 gives omega - 1, channel 1 the cover.  Returns (bytes, owner, count, number of frames rendered)."""
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
        return np.zeros((wh, ww, 3), np.uint8), np.zeros((wh, ww), np.uint16), np.zeros((wh, ww), np.uint16), 0
    maps, wmaps = [None] * n, [None] * n
    for k, (samp, wc) in zip(sub, ol.parallel_map(one, sub, threads=threads)):
        maps[k] = (samp, wc[..., 1] != 0)
        wmaps[k] = (wc, wc[..., 1] != 0)
    out, owner, count, _, _ = pick(maps, wmaps)
    return out, owner, count, len(sub)

"""numpy restatement of weighted (feather) blending (include/mi355_mosaic.h, "weighted (feather) blending"; csrc/feather.hip).

Built from the oracle's refined render alone, the way tests/gain_ref.py is: gain_ref.frame_sample_maps gives every frame's sample bytes and
cover on the unchanged layout; a second call with every image replaced by its three-channel Wk image gives omega_k - 1 (the byte the refined
render takes from the weight image).  The blend itself is int64 numpy.
"""
import numpy as np

from tests import gain_ref as gr


def ramp_of(w, h, ramp=0):
    """R of a w x h frame: params.ramp, or a full tent (min(w, h) + 1) / 2 for ramp == 0"""
    return int(ramp) if ramp > 0 else (min(int(w), int(h)) + 1) // 2


def wk_image(w, h, ramp=0):
    """Wk [h, w] uint8: (254 * min(d, R)) / R with d the integer border distance min(i, w-1-i, j, h-1-j)"""
    R = ramp_of(w, h, ramp)
    i, j = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    d = np.minimum.outer(np.minimum(j, h - 1 - j), np.minimum(i, w - 1 - i))
    return ((254 * np.minimum(d, R)) // R).astype(np.uint8)


def wk_images(imgs, ramp=0):
    return [np.ascontiguousarray(np.repeat(wk_image(i.shape[1], i.shape[0], ramp)[:, :, None], 3, axis=2)) for i in imgs]


def blend(maps, wmaps):
    """(canvas [ch, cw, 3] uint8, layers [ch, cw] int64) from per-frame (samples, cover) and the same maps of the Wk images"""
    shape = next(m for m in maps if m is not None)[1].shape
    num = np.zeros(shape + (3,), np.int64)
    den = np.zeros(shape, np.int64)
    layers = np.zeros(shape, np.int64)
    for m, wm in zip(maps, wmaps):
        if m is None:
            continue
        samp, cover = m
        om = (1 + wm[0][..., 0]) * cover
        num += om[..., None] * samp
        den += om
        layers += cover
    out = np.where(den[..., None] > 0, (num + (den // 2)[..., None]) // np.maximum(den, 1)[..., None], 0)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8), layers


def feather_ref(orc, imgs, h9s, ramp=0, maps=None):
    """the feathered canvas [ch, cw, 3] and the number of contributing frames per pixel; maps: gain_ref.frame_sample_maps(orc, imgs, h9s)
    when the caller already has it"""
    if maps is None:
        maps = gr.frame_sample_maps(orc, imgs, h9s)
    wmaps = gr.frame_sample_maps(orc, wk_images(imgs, ramp), h9s)
    for m, wm in zip(maps, wmaps):
        # the Wk image is zero on the frame's border: its own 255-render must still give the frame's cover
        assert (m is None) == (wm is None) and (m is None or np.array_equal(m[1], wm[1]))
    return blend(maps, wmaps)


def window_ref(orc, get_img, w, h, h9s, window, ramp=0, threads=4):
    """the feathered bytes [wh, ww, 3] of the canvas window (x0, y0, ww, wh) of a large survey (every frame w x h): only the frames whose
    canvas box (grown by 2 px) reaches the window are rendered, each alone inside the full canvas geometry -- the frames that define the
    canvas box ride along as zero images -- once with its pixels and once as (Wk, 255, 255): channel 0 gives omega - 1, channel 1 the cover.
    get_img(k): frame k as h x w x 3.  Returns (bytes, number of frames rendered)."""
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
    wimg = wk_images([zero], ramp)[0].copy()
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

    num = np.zeros((wh, ww, 3), np.int64)
    den = np.zeros((wh, ww), np.int64)
    for samp, wc in ol.parallel_map(one, sub, threads=threads):
        om = (1 + wc[..., 0]) * (wc[..., 1] != 0)
        num += om[..., None] * samp
        den += om
    out = np.where(den[..., None] > 0, (num + (den // 2)[..., None]) // np.maximum(den, 1)[..., None], 0)
    return out.astype(np.uint8), len(sub)

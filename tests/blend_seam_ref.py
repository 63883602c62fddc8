"""numpy restatement of the multiband blend along optimised seams (include/mi355_mosaic.h, "multiband blend along optimised seams";
csrc/blend_seam.hip): candidates in the blend's own geometry, the label stage of tests/seamcut_ref.py as it is, the ownership that follows a
cell map, and the oracle's multiband blend fed the restated masks.

Built on tests/warp_ref.py: chips_and_masks gives the blend's canvas, the chips' bytes and validity masks, distance_map the float32 value
FindMasksByDistMap compares (the distance to the nearest edge line over the chip's maximum), ownership the owner map `best`.

  candidates  per cell of the s x s grid the min(|C|, depth) chips that are largest in (d descending, chip position ascending) at the cell's
              probe pixel among those with a valid sample and d > 0 there; frame = the chip's image + 1, omega = 1 + (int) min(d * 254, 254) in
              float32, gray = the rounded mean of the integer gray of the chip's own bytes over the cell's pixels where its validity is 255;
  labels      seamcut_ref.labels, unchanged;
  ownership   a pixel whose cell names the image of a chip that is valid there belongs to that chip; every other pixel keeps `best`.
`mutate` switches one rule off (tests/test_blend_seam_ref.py shows that each is seen by some case):
  tie      among equal d the HIGHER position comes first;
  dpos     the map overrides only where the named chip has d > 0;
  round    omega rounds d * 254 to nearest instead of truncating;
  probe    gray is the chip's gray at the probe pixel alone.
"""
import numpy as np

from tests import seamcut_ref as sc
from tests import warp_ref as wr

f32 = np.float32
SLOTS = sc.SLOTS
MUTATIONS = ("tie", "dpos", "round", "probe")


def params(**kw):
    p = sc.params(**kw)
    assert p["ramp"] == 0, "ramp has no meaning for the blend's seams"
    return p


def chip_set(imgs, h9s, keep=None):
    """warp_ref.chips_and_masks (find_masks=True) plus, per chip on the canvas: d [ch, cw] float32 (FindMasksByDistMap's value, 0 off the chip),
    cover [ch, cw] bool (validity 255) and gray [ch, cw] (the header's integer gray of the chip's own bytes)"""
    h9s = np.asarray(h9s, np.float32).reshape(-1, 9)
    invs = [wr.inverse(m, 1e-12) if (keep is None or keep[k]) and m[8] != 0 else None for k, m in enumerate(h9s)]
    r = wr.chips_and_masks(imgs, h9s, invs, keep=keep, find_masks=True)
    cw, ch = r["cw"], r["ch"]
    if r["best"] is None:
        r["best"] = np.full((ch, cw), -1, np.int32)
    nv = len(r["chips"])
    r["d"] = np.zeros((nv, ch, cw), np.float32)
    r["cover"] = np.zeros((nv, ch, cw), bool)
    r["gray"] = np.zeros((nv, ch, cw), np.int64)
    for v, c in enumerate(r["chips"]):
        x0, y0, w, h = int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, ch), max(x0, 0), min(x0 + w, cw)
        if yb <= ya or xb <= xa:
            continue
        sub = np.s_[ya - y0:yb - y0, xa - x0:xb - x0]
        d, _ = wr.distance_map(r["valid"][v], c)
        r["d"][v, ya:yb, xa:xb] = d[sub]
        r["cover"][v, ya:yb, xa:xb] = r["valid"][v][:, :w][sub] == 255
        r["gray"][v, ya:yb, xa:xb] = sc.gray_of(r["chip_imgs"][v][:, :3 * w].reshape(h, w, 3))[sub]
    return r


def candidates(r, level, depth, mutate=None):
    """(frame [gh, gw, 8] uint16, omega [gh, gw, 8] uint8, gray [gh, gw, 8] uint8) and slot0 [gh, gw]: the chip position in slot 0 or -1"""
    cw, ch = r["cw"], r["ch"]
    nv = len(r["chips"])
    assert nv <= 65535
    s = 1 << level
    gw, gh = sc.grid_of(cw, ch, level)
    py = np.minimum(np.arange(gh) * s + s // 2, ch - 1)
    px = np.minimum(np.arange(gw) * s + s // 2, cw - 1)
    rows = max(nv, SLOTS)
    dp = np.full((rows, gh, gw), -1, np.float32)                            # d at the probe, -1: no candidate
    pos = np.arange(rows)[:, None, None] * np.ones((1, gh, gw), np.int64)
    mean = np.zeros((rows, gh, gw), np.int64)
    img = np.zeros(rows, np.int64)
    for v in range(nv):
        d = r["d"][v][np.ix_(py, px)]
        with np.errstate(invalid="ignore"):
            cand = r["cover"][v][np.ix_(py, px)] & (d > 0)                  # false for NaN and for 0
        dp[v] = np.where(cand, d, f32(-1))
        g = np.zeros((gh * s, gw * s), np.int64)
        c = np.zeros((gh * s, gw * s), np.int64)
        g[:ch, :cw] = r["gray"][v] * r["cover"][v]
        c[:ch, :cw] = r["cover"][v]
        tot = g.reshape(gh, s, gw, s).sum(axis=(1, 3))
        cnt = c.reshape(gh, s, gw, s).sum(axis=(1, 3))
        mean[v] = r["gray"][v][np.ix_(py, px)] if mutate == "probe" else (tot + cnt // 2) // np.maximum(cnt, 1)
        assert (cnt[cand] > 0).all()                                        # a candidate has at least the probe
        img[v] = int(r["chips"][v]["img"])
    order = np.lexsort((-pos if mutate == "tie" else pos, -dp), axis=0)[:SLOTS]      # d descending, then the position
    dsel = np.take_along_axis(dp, order, axis=0)
    on = dsel > 0
    on[depth:] = False
    with np.errstate(invalid="ignore"):
        scaled = np.where(on, dsel, f32(0)) * f32(254.0)
        if mutate == "round":
            scaled = np.rint(scaled)
        omega = (1 + np.minimum(scaled, f32(254.0)).astype(np.int64)) * on
    frame = (img[order] + 1) * on
    gray = np.take_along_axis(mean, order, axis=0) * on
    assert omega.max(initial=0) <= 255 and gray.max(initial=0) <= 255
    slot0 = np.where(on[0], order[0], -1)
    mv = lambda a: np.moveaxis(a, 0, 2)
    return mv(frame).astype(np.uint16), mv(omega).astype(np.uint8), mv(gray).astype(np.uint8), slot0


def ownership_under(r, cells, level, mutate=None):
    """(masks, best): the ownership that follows the cell map"""
    cw, ch = r["cw"], r["ch"]
    s = 1 << level
    want = np.repeat(np.repeat(np.asarray(cells).astype(np.int64), s, axis=0), s, axis=1)[:ch, :cw] - 1
    best = r["best"].copy()
    for v, c in enumerate(r["chips"]):
        mine = (want == int(c["img"])) & r["cover"][v]
        if mutate == "dpos":
            with np.errstate(invalid="ignore"):
                mine &= r["d"][v] > 0
        best[mine] = v
    masks = []
    for v, c in enumerate(r["chips"]):
        x0, y0, w, h = int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])
        m = np.zeros_like(r["valid"][v])
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, ch), max(x0, 0), min(x0 + w, cw)
        if yb > ya and xb > xa:
            m[ya - y0:yb - y0, xa - x0:xb - x0] = (best[ya:yb, xa:xb] == v) * np.uint8(255)
        masks.append(m)
    return masks, best


def blend_seam_ref(orc, imgs, h9s, p, keep=None, cells=None, mutate=None, band=5, chips=None, blend=True):
    """everything of one case: dict(set, frame, omega, gray, records, slot0, cells (the label stage's), report, masks, best (under `cells` when
    given, else under the label stage's map), canvas (the oracle's multiband blend of those masks; None without blend))"""
    assert p["ramp"] == 0
    r = chip_set(imgs, h9s, keep) if chips is None else chips
    frame, omega, gray, slot0 = candidates(r, p["level"], p["depth"], mutate)
    own, report = sc.labels(frame, omega, gray, p)
    masks, best = ownership_under(r, own if cells is None else cells, p["level"], mutate)
    canvas = orc.multiband_blend(r["chips"], r["chip_imgs"], masks, r["cw"], r["ch"], band)[0] if blend else None
    return dict(set=r, frame=frame, omega=omega, gray=gray, records=sc.record_bytes(frame, omega, gray), slot0=slot0, cells=own, report=report,
                masks=masks, best=best, canvas=canvas)


def owner_frames(r, best):
    """the owner map by image: image + 1, 0 where nobody owns (the form seamcut_ref.seam_disagreement takes)"""
    img = np.array([int(c["img"]) + 1 for c in r["chips"]] + [0], np.int64)
    return img[best]


def sample_maps(r, n):
    """per image (sample bytes [ch, cw, 3], cover [ch, cw]) on the blend's canvas, None for an image without a chip: seam_disagreement's maps"""
    cw, ch = r["cw"], r["ch"]
    maps = [None] * n
    for v, c in enumerate(r["chips"]):
        x0, y0, w, h = int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])
        samp = np.zeros((ch, cw, 3), np.uint8)
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, ch), max(x0, 0), min(x0 + w, cw)
        if yb > ya and xb > xa:
            samp[ya:yb, xa:xb] = r["chip_imgs"][v][:, :3 * w].reshape(h, w, 3)[ya - y0:yb - y0, xa - x0:xb - x0]
        maps[int(c["img"])] = (samp, r["cover"][v])
    return maps

"""numpy restatement of the optimised seamlines (include/mi355_mosaic.h, "optimised seamlines"; csrc/seamcut.hip): candidates, labels, render.

Built like tests/median_ref.py, from the oracle's refined render alone: gain_ref.frame_sample_maps gives every frame's sample bytes and cover on
the unchanged layout, seamline_ref.weight_maps the weight omega_k.  Everything after that is integers.

  candidates  per cell of the s x s grid (s = 1 << level) the min(|C|, depth) frames that are largest in the seamline order (omega, k) at the
              cell's probe pixel, each with omega and the rounded mean of its gray over the cell's pixels it gives a sample;
  labels      four-direction scanline aggregation of data cost + pairwise seam cost over the cells' slots, argmin, energy check; the cell map
              names a frame only where the label left slot 0;
  render      the seamline render, except that a pixel whose cell names a frame that gives it a sample takes that frame.
`mutate` switches one rule of the label stage off (tests/test_seamcut_ref.py shows that each rule is seen by some case):
  tie      the higher slot wins an argmin tie;
  restart  a cell without candidates does not end the path: the costs of the last cell that had some are carried over it;
  miss     miss_cost counts as 0;
  nosub    the minimum over the cell before is not subtracted.  In exact arithmetic that shifts all slots of a cell alike and changes no label:
           the subtraction is there to keep L bounded, and the mutation shows only through the 16 bits the sums are kept in (modelled
           here as in the kernel); it is a check of that bound, not of the cost arithmetic;
  dir      the fourth direction is left out.
"""
import numpy as np

from tests import gain_ref as gr
from tests import seamline_ref as sr

SLOTS = 8                                                                   # slots of a cell record (MI355_SEAMCUT_MAX_DEPTH)
DEFAULTS = dict(ramp=0, level=3, depth=4, data_weight=1, diff_weight=2, seam_penalty=2, miss_cost=32)
RANGES = dict(ramp=(0, None), level=(2, 5), depth=(1, 8), data_weight=(0, 16), diff_weight=(0, 16), seam_penalty=(0, 255), miss_cost=(0, 255))
MUTATIONS = ("tie", "restart", "miss", "nosub", "dir")
INF = 1 << 28


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = int(v)
    for k, (lo, hi) in RANGES.items():
        assert p[k] >= lo and (hi is None or p[k] <= hi), (k, p[k])
    return p


def gray_of(samp):
    """the header's integer gray of B G R sample bytes"""
    s = samp.astype(np.int64)
    return (1868 * s[..., 0] + 9617 * s[..., 1] + 4899 * s[..., 2] + 8192) >> 14


def grid_of(cw, ch, level):
    s = 1 << level
    return (cw + s - 1) // s, (ch + s - 1) // s


def candidates(maps, wmaps, level, depth):
    """(frame [gh, gw, 8] uint16 = frame + 1 or 0, omega [gh, gw, 8] uint8, gray [gh, gw, 8] uint8): the cell records"""
    n = len(maps)
    ch, cw = next(m for m in maps if m is not None)[1].shape
    s = 1 << level
    gw, gh = grid_of(cw, ch, level)
    py = np.minimum(np.arange(gh) * s + s // 2, ch - 1)
    px = np.minimum(np.arange(gw) * s + s // 2, cw - 1)
    keys = np.zeros((max(n, SLOTS), gh, gw), np.int64)                      # omega << 16 | k + 1 where frame k covers the probe
    mean = np.zeros((n + 1, gh, gw), np.int64)                              # mean[k + 1]: frame k's gray signature
    for k, (m, wm) in enumerate(zip(maps, wmaps)):
        if m is None:
            continue
        samp, cover = m
        om = ((1 + wm[0][..., 0]) * cover)[np.ix_(py, px)]
        assert om.max() <= 255 and n <= 65535
        keys[k] = (om << 16 | (k + 1)) * (om > 0)
        g = np.zeros((gh * s, gw * s), np.int64)
        c = np.zeros((gh * s, gw * s), np.int64)
        g[:ch, :cw] = gray_of(samp) * cover
        c[:ch, :cw] = cover
        tot = g.reshape(gh, s, gw, s).sum(axis=(1, 3))
        cnt = c.reshape(gh, s, gw, s).sum(axis=(1, 3))
        mean[k + 1] = (tot + cnt // 2) // np.maximum(cnt, 1)
        assert (cnt[om > 0] > 0).all()                                      # a candidate has at least the probe
    keys = np.sort(keys, axis=0)[::-1][:SLOTS]
    keys[depth:] = 0
    frame = np.moveaxis(keys & 0xffff, 0, 2)
    omega = np.moveaxis(keys >> 16, 0, 2)
    gray = np.take_along_axis(mean, np.moveaxis(frame, 2, 0), axis=0)
    gray = np.moveaxis(gray, 0, 2) * (frame > 0)
    assert gray.max() <= 255
    return frame.astype(np.uint16), omega.astype(np.uint8), gray.astype(np.uint8)


def record_bytes(frame, omega, gray):
    """the cell records as the C ABI stores them: [gh, gw, 32] uint8 (mi355_seam_cell: uint16 frame[8], uint8 omega[8], uint8 gray[8])"""
    f = np.ascontiguousarray(frame.astype("<u2")).view(np.uint8).reshape(frame.shape[:2] + (16,))
    return np.concatenate([f, omega, gray], axis=2)


def pair_cost(fp, gp, fq, gq, p, mutate=None):
    """V[..., a, b] between slot a of cell p and slot b of cell q (leading axes: any), empty slots included (their value is not used)"""
    fp, gp, fq, gq = (x.astype(np.int64) for x in (fp, gp, fq, gq))
    miss = 0 if mutate == "miss" else p["miss_cost"]
    match = (fp[..., :, None] == fq[..., None, :]) & (fp[..., :, None] > 0)
    has_p = match.any(axis=-2)                                              # [.., b]: frame l of slot b is a candidate of p
    gp_l = (match * gp[..., :, None]).sum(axis=-2)
    dp = np.where(has_p[..., None, :], np.abs(gp[..., :, None] - gp_l[..., None, :]), miss)
    has_q = match.any(axis=-1)                                              # [.., a]: frame k of slot a is a candidate of q
    gq_k = (match * gq[..., None, :]).sum(axis=-1)
    dq = np.where(has_q[..., :, None], np.abs(gq_k[..., :, None] - gq[..., None, :]), miss)
    return np.where(match, 0, p["seam_penalty"] + p["diff_weight"] * (dp + dq))


def _sweep(frame, gray, D, p, mutate):
    """L of the direction that walks axis 1 upwards: [lines, cells, 8]"""
    lines, cells = frame.shape[:2]
    valid = frame > 0
    L = np.zeros((lines, cells, SLOTS), np.int64)
    qf = np.zeros((lines, SLOTS), np.int64); qg = qf.copy(); qL = qf.copy()
    for x in range(cells):
        f, g, d = frame[:, x].astype(np.int64), gray[:, x].astype(np.int64), D[:, x]
        qv = qf > 0
        some = qv.any(axis=1)
        V = pair_cost(f, g, qf, qg, p, mutate)
        cand = np.where(qv[:, None, :], qL[:, None, :] + V, INF).min(axis=2)
        mp = np.where(qv, qL, INF).min(axis=1)
        if mutate == "nosub":
            mp = np.zeros_like(mp)
        cur = np.where(some[:, None], d + cand - mp[:, None], d) * valid[:, x]
        assert mutate == "nosub" or cur.max() <= 12479
        L[:, x] = cur
        keep = (mutate == "restart") & ~valid[:, x].any(axis=1)             # the mutation: a hole does not end the path
        qf = np.where(keep[:, None], qf, f); qg = np.where(keep[:, None], qg, g); qL = np.where(keep[:, None], qL, cur)
    return L


def energy(frame, omega, gray, slot, p):
    """sum of D over the cells + sum of V over the 4-neighbour pairs whose two cells both have a candidate"""
    f = frame.astype(np.int64); g = gray.astype(np.int64); om = omega.astype(np.int64)
    some = f[..., 0] > 0
    pick = lambda a, s: np.take_along_axis(a, s[..., None], axis=2)[..., 0]
    e = int((p["data_weight"] * (om[..., 0] - pick(om, slot)) * some).sum())
    for sl_p, sl_q in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        V = pair_cost(f[sl_p], g[sl_p], f[sl_q], g[sl_q], p)
        v = np.take_along_axis(np.take_along_axis(V, slot[sl_p][..., None, None], axis=-2), slot[sl_q][..., None, None], axis=-1)[..., 0, 0]
        e += int((v * (some[sl_p] & some[sl_q])).sum())
    return e


def labels(frame, omega, gray, p, mutate=None, full=False):
    """(cells [gh, gw] uint16 = frame + 1 where the returned label is not slot 0, else 0 -- there the render keeps the seamline rule --, report
    dict(energy_before, energy_after, changed, fallback)); full: also (slot [gh, gw] of the returned labelling, S)"""
    om = omega.astype(np.int64)
    valid = frame > 0
    D = p["data_weight"] * (om[..., :1] - om) * valid
    S = np.zeros(frame.shape, np.int64)                                     # L <= 16 * 254 + 255 + 16 * 510 = 12479 per direction: no wrap
    dirs = (lambda a: a, lambda a: a[:, ::-1], lambda a: a.swapaxes(0, 1), lambda a: a.swapaxes(0, 1)[:, ::-1])
    undo = (lambda a: a, lambda a: a[:, ::-1], lambda a: a.swapaxes(0, 1), lambda a: a[:, ::-1].swapaxes(0, 1))
    for r, (t, u) in enumerate(zip(dirs, undo)):
        if mutate == "dir" and r == 3:
            continue
        S = (S + u(_sweep(t(frame), t(gray), t(D), p, mutate))) & 0xffff   # the sums are kept in 16 bits: only the nosub mutation wraps
    Sv = np.where(valid, S, INF)
    slot = (SLOTS - 1 - np.argmin(Sv[..., ::-1], axis=2)) if mutate == "tie" else np.argmin(Sv, axis=2)
    slot = slot * valid[..., 0]
    before = energy(frame, omega, gray, np.zeros_like(slot), p)
    after = energy(frame, omega, gray, slot, p)
    fallback = after > before
    if fallback:
        slot = np.zeros_like(slot)
    cells = (np.take_along_axis(frame, slot[..., None], axis=2)[..., 0] * (slot > 0)).astype(np.uint16)
    report = dict(energy_before=before, energy_after=after, changed=int((slot > 0).sum()), fallback=int(fallback))
    return (cells, report, slot, S) if full else (cells, report)


def render(maps, wmaps, cells, level):
    """(canvas [ch, cw, 3] uint8, owner [ch, cw] uint16, count [ch, cw] uint16): the seamline render, a pixel whose cell names a frame that
    gives it a sample taking that frame"""
    out, owner, count, _, _ = sr.pick(maps, wmaps)
    ch, cw = owner.shape
    s = 1 << level
    want = np.repeat(np.repeat(cells.astype(np.int64), s, axis=0), s, axis=1)[:ch, :cw]
    out, owner = out.copy(), owner.copy()
    for k, m in enumerate(maps):
        if m is None:
            continue
        mine = (want == k + 1) & m[1]
        owner[mine] = k + 1
        out[mine] = m[0][mine]
    return out, owner, count


def seamcut_ref(orc, imgs, h9s, p, maps=None, wmaps=None, cells=None, mutate=None):
    """everything of one case: dict(maps, wmaps, frame, omega, gray, records, cells, report, slot, canvas, owner, count)"""
    if maps is None:
        maps = gr.frame_sample_maps(orc, imgs, h9s)
    if wmaps is None:
        wmaps = sr.weight_maps(orc, imgs, h9s, p["ramp"], maps)
    frame, omega, gray = candidates(maps, wmaps, p["level"], p["depth"])
    own, report, slot, S = labels(frame, omega, gray, p, mutate, full=True)
    canvas, owner, count = render(maps, wmaps, own if cells is None else cells, p["level"])
    return dict(maps=maps, wmaps=wmaps, frame=frame, omega=omega, gray=gray, records=record_bytes(frame, omega, gray), cells=own, report=report,
                slot=slot, S=S, canvas=canvas, owner=owner, count=count)


def seam_disagreement(maps, owner):
    """the full-resolution seam disagreement of an owner map: over the 4-neighbour pixel pairs (x, y) with different owners k, l the sum of
    |gray_k - gray_l| at x and at y, each term where both frames give the pixel a sample"""
    own = owner.astype(np.int64)
    n = len(maps)
    g = np.zeros((n + 1,) + own.shape, np.int64)
    c = np.zeros((n + 1,) + own.shape, bool)
    for k, m in enumerate(maps):
        if m is not None:
            g[k + 1], c[k + 1] = gray_of(m[0]), m[1]
    total = 0
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        k, l = own[a], own[b]
        seam = (k != l) & (k > 0) & (l > 0)
        for at in (a, b):
            gk = np.take_along_axis(g[(slice(None),) + at], k[None], axis=0)[0]
            gl = np.take_along_axis(g[(slice(None),) + at], l[None], axis=0)[0]
            both = np.take_along_axis(c[(slice(None),) + at], k[None], axis=0)[0] & np.take_along_axis(c[(slice(None),) + at], l[None], axis=0)[0]
            total += int((np.abs(gk - gl) * (seam & both)).sum())
    return total

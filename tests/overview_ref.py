"""numpy restatement of the overview levels of include/mi355_mosaic.h ("overview levels of a canvas"): no reliance on the library.

Pixel (X, Y) of level l owns the level-0 block [X 2^l, (X+1) 2^l) x [Y 2^l, (Y+1) 2^l) clipped to the canvas; n = its valid pixels,
S[c] = their channel sums, out[c] = n ? (S[c] + n // 2) // n : 0; rows padded with zeros to ows_l = (3 ow_l + 3) & ~3; cover = n.
Block sums: the canvas padded with invalid pixels to a multiple of 2^l, reshaped, summed in uint64.
"""
import numpy as np

NONE, ZERO, MAP = 0, 1, 2


def layout(cw, ch, levels):
    """[(ow_l, oh_l, ows_l) for l = 1 .. levels]"""
    out = []
    for l in range(1, levels + 1):
        ow, oh = (cw + (1 << l) - 1) >> l, (ch + (1 << l) - 1) >> l
        out.append((ow, oh, (3 * ow + 3) & ~3))
    return out


def pixels(canvas, cw):
    """[ch, cws] uint8 rows -> [ch, cw, 3]"""
    canvas = np.asarray(canvas)
    return canvas if canvas.ndim == 3 else np.ascontiguousarray(canvas[:, :3 * cw]).reshape(canvas.shape[0], cw, 3)


def valid_map(pix, nodata, vmap=None):
    if nodata == NONE:
        return np.ones(pix.shape[:2], bool)
    if nodata == ZERO:
        return pix.any(axis=2)
    assert nodata == MAP and vmap is not None
    return np.asarray(vmap) != 0


def block_sums(a, l):
    """sums of a [ch, cw, ...] array over the 2^l x 2^l blocks (clipped at the canvas's edge), uint64"""
    b = 1 << l
    ch, cw = a.shape[:2]
    oh, ow = (ch + b - 1) >> l, (cw + b - 1) >> l
    p = np.zeros((oh * b, ow * b) + a.shape[2:], np.uint64)
    p[:ch, :cw] = a
    return p.reshape((oh, b, ow, b) + a.shape[2:]).sum(axis=(1, 3), dtype=np.uint64)


def finish(S, n):
    """(sums [oh, ow, 3], counts [oh, ow]) -> (level [oh, ows] uint8 with zeroed padding, cover [oh, ow] uint16)"""
    oh, ow = n.shape
    nn = np.maximum(n, 1)[..., None]
    px = np.where(n[..., None] > 0, (S + (n // 2)[..., None]) // nn, 0)
    assert px.max(initial=0) <= 255 and n.max(initial=0) <= 16384
    out = np.zeros((oh, (3 * ow + 3) & ~3), np.uint8)
    out[:, :3 * ow] = px.astype(np.uint8).reshape(oh, 3 * ow)
    return out, n.astype(np.uint16)


def overview_ref(canvas, cw, levels, nodata=NONE, vmap=None):
    """the direct definition: every level from level 0.  Returns [(level, cover) for l = 1 .. levels]."""
    pix = pixels(canvas, cw)
    V = valid_map(pix, nodata, vmap)
    masked = pix.astype(np.uint64) * V[..., None]
    return [finish(block_sums(masked, l), block_sums(V, l)) for l in range(1, levels + 1)]


def overview_carried(canvas, cw, levels, nodata=NONE, vmap=None):
    """the form a one-pass kernel uses: sums and counts carried from level l - 1 to level l (2 x 2 cells at a time), never re-derived from
    level 0 and never from the rounded bytes"""
    pix = pixels(canvas, cw)
    V = valid_map(pix, nodata, vmap)
    S, n = pix.astype(np.uint64) * V[..., None], V.astype(np.uint64)
    out = []
    for _ in range(levels):
        S, n = block_sums(S, 1), block_sums(n, 1)
        out.append(finish(S, n))
    return out


def block_min_max(pix, V, l):
    """per block the smallest and largest VALID sample of each channel (255 / 0 where the block has none)"""
    b = 1 << l
    ch, cw = V.shape
    oh, ow = (ch + b - 1) >> l, (cw + b - 1) >> l
    lo = np.full((oh * b, ow * b, 3), 255, np.uint8)
    hi = np.zeros((oh * b, ow * b, 3), np.uint8)
    lo[:ch, :cw] = np.where(V[..., None], pix, 255)
    hi[:ch, :cw] = np.where(V[..., None], pix, 0)
    return lo.reshape(oh, b, ow, b, 3).min(axis=(1, 3)), hi.reshape(oh, b, ow, b, 3).max(axis=(1, 3))


def stripes(canvas, cw, levels, cuts, nodata=NONE, vmap=None, fill=0xA5):
    """the whole canvas as stripes [cuts[i], cuts[i+1]): each stripe is reduced ON ITS OWN ROWS (a canvas of its own whose blocks are cut
    where the whole canvas's are) and lands in rows [row0 >> l, (row0 + rows + 2^l - 1) >> l) of prefilled outputs"""
    pix = pixels(canvas, cw)
    ch = pix.shape[0]
    geo = layout(cw, ch, levels)
    outs = [(np.full((oh, ows), fill, np.uint8), np.full((oh, ow), 0xA5A5, np.uint16)) for ow, oh, ows in geo]
    for row0, row1 in zip(cuts[:-1], cuts[1:]):
        assert row0 % (1 << levels) == 0 and (row1 == ch or row1 % (1 << levels) == 0)
        part = overview_ref(pix[row0:row1], cw, levels, nodata, None if vmap is None else np.asarray(vmap)[row0:row1])
        for l in range(1, levels + 1):
            y0, y1 = row0 >> l, (row1 + (1 << l) - 1) >> l
            outs[l - 1][0][y0:y1] = part[l - 1][0]
            outs[l - 1][1][y0:y1] = part[l - 1][1]
    return outs

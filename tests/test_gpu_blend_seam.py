"""GPU: the multiband blend along optimised seams (mi355_blend_seam_cells_dev, mi355_chips_and_masks_seam, mi355_mosaic_blended_seam / _dev /
_into, csrc/blend_seam.hip) byte for byte against tests/blend_seam_ref.py on every case of tests/blend_seam_patterns.py, with pre-filled
outputs so that unwritten bytes show.

  * per case: the candidate records, the cell map, the report, every mask and chip and the blended canvas;
  * the device, host, _into and two-stage forms agree; cell maps given by the caller are followed;
  * an all-zero map, depth = 1, and diff_weight = seam_penalty = 0 each give the bytes of ChipsAndMasks / MosaicBlended;
  * every refusal, and the ctx goes on working.
"""
import numpy as np
import pytest

from tests import blend_seam_patterns as bp

pytestmark = pytest.mark.gpu
BAND = 5


def _upload(torch, imgs):
    from tests.test_gpu_gain import _upload as up
    return up(torch, imgs)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _canvas(torch, im, w, h, h9s, keep, fill=7):
    cw, ch, cws = im.blend_layout(w, h, h9s, keep)
    t = torch.full((ch, cws), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                                # the fill runs on torch's stream, the library on the ctx's own
    return t, cw, ch, cws


def _same_set(got, r, what):
    s = r["set"]
    assert (got["cw"], got["ch"]) == (s["cw"], s["ch"]) and len(got["chips"]) == len(s["chips"]), what
    for f in ("x0", "y0", "w", "h", "img"):
        assert np.array_equal(got["chips"][f], s["chips"][f]), (what, f)
    for v, (a, b) in enumerate(zip(got["masks"], r["masks"])):
        bad = a != b
        assert a.shape == b.shape and not bad.any(), "%s mask %d: %d bytes differ, first %s" % (what, v, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    for v, (a, b) in enumerate(zip(got["chip_imgs"], s["chip_imgs"])):
        assert np.array_equal(a, b), "%s chip %d" % (what, v)


def _same_canvas(a, b, what):
    bad = a != b
    assert a.shape == b.shape and not bad.any(), "%s canvas: %d bytes differ, first %s" % (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("name", sorted(bp.CASES))
def test_case_equals_restatement(oracle, name):
    import torch
    import imagemosaicing_amd as im
    case, cells, r = bp.reference(oracle, name)
    imgs, h9s, p, keep = case.imgs, case.h9s, case.p, case.keep
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    gh, gw = r["cells"].shape
    assert im.blend_seam_grid(w, h, h9s, p["level"], keep) == (gw, gh)
    # stages 1 and 2
    d_cand = torch.full((gh * gw * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    d_cells = torch.full((gh * gw,), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rep = ctx.BlendSeamCellsDev(ptrs, w, h, ws, h9s, d_cells.data_ptr(), gw, gh, keep=keep, d_cand=d_cand.data_ptr(), **p)
    rec = d_cand.cpu().numpy().reshape(gh, gw, 32)
    bad = (rec != r["records"]).any(axis=2)
    assert not bad.any(), "records: %d cells differ, first %s" % (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    got_cells = d_cells.cpu().numpy().view(np.uint16).reshape(gh, gw)
    assert np.array_equal(got_cells, r["cells"]), np.argwhere(got_cells != r["cells"])[:5].tolist()
    assert rep == r["report"], (rep, r["report"])
    d2 = torch.full((gh * gw,), 0x1111, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert ctx.BlendSeamCellsDev(ptrs, w, h, ws, h9s, d2.data_ptr(), gw, gh, keep=keep, **p) == r["report"] and torch.equal(d2, d_cells)      # without d_cand
    # the two-stage form: masks and chips under the case's map (the caller's, or the label stage's made inside the call) ...
    two = ctx.ChipsAndMasksSeam(imgs, h9s, keep=keep, cells=cells, **p)
    _same_set(two, r, name + ", two-stage")
    if cells is None:
        _same_set(ctx.ChipsAndMasksSeam(imgs, h9s, keep=keep, cells=got_cells, **p), r, name + ", two-stage, the map handed back")
    # ... feed the blender
    buf, ow, oh, ows = ctx.MultiBandBlend(two["chips"], two["chip_imgs"], two["masks"], two["cw"], two["ch"], BAND)
    _same_canvas(buf, r["canvas"], name + ", two-stage")
    # the device form under the same map
    d_map = _dev(torch, cells) if cells is not None else None
    t, cw, ch, cws = _canvas(torch, im, w, h, h9s, keep)
    ctx.MosaicBlendedSeamDev(ptrs, w, h, ws, h9s, t.data_ptr(), cw, ch, cws, keep=keep, band=BAND, d_cells=d_map.data_ptr() if cells is not None else 0, **p)
    _same_canvas(t.cpu().numpy(), r["canvas"], name + ", device")
    if cells is None:
        # the host and _into forms make the map themselves; the device form takes the one made above
        t2, _, _, _ = _canvas(torch, im, w, h, h9s, keep, fill=9)
        ctx.MosaicBlendedSeamDev(ptrs, w, h, ws, h9s, t2.data_ptr(), cw, ch, cws, keep=keep, band=BAND, d_cells=d_cells.data_ptr(), gw=gw, gh=gh, **p)
        assert torch.equal(t, t2)
        hb, hw, hh, hws = ctx.MosaicBlendedSeam(imgs, h9s, keep=keep, band=BAND, **p)
        assert (hw, hh, hws) == (cw, ch, cws)
        _same_canvas(hb, r["canvas"], name + ", host")
        pitch = cws + 8
        out = np.full((ch, pitch), 0x5A, np.uint8)
        ctx.MosaicBlendedSeamInto(imgs, None, h9s, keep=keep, band=BAND, out=out, pitch=pitch, **p)
        _same_canvas(out[:, :3 * cw], r["canvas"][:, :3 * cw], name + ", into")
        assert (out[:, 3 * cw:] == 0x5A).all()
    ctx.close()


@pytest.mark.parametrize("name", ("crafted3", "nine_depth4", "projective", "many65", "big"))
def test_consequences(name):
    """an all-zero map, depth = 1, and diff_weight = seam_penalty = 0 each give the bytes of ChipsAndMasks(find_masks=True) and of MosaicBlended"""
    import torch
    import imagemosaicing_amd as im
    case = bp.CASES[name]()
    imgs, h9s, p, keep = case.imgs, case.h9s, case.p, case.keep
    ctx = im.Context(0)
    plain = ctx.ChipsAndMasks(imgs, h9s, keep=keep, find_masks=True)
    blended = ctx.MosaicBlended(imgs, h9s, keep=keep, band=BAND)[0]
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    gw, gh = im.blend_seam_grid(w, h, h9s, p["level"], keep)
    for what, q, cells in (("zero map", p, np.zeros((gh, gw), np.uint16)), ("depth 1", dict(p, depth=1), None),
                           ("free seams", dict(p, diff_weight=0, seam_penalty=0), None)):
        got = ctx.ChipsAndMasksSeam(imgs, h9s, keep=keep, cells=cells, **q)
        assert (got["cw"], got["ch"]) == (plain["cw"], plain["ch"]) and got["chips"].tobytes() == plain["chips"].tobytes(), what
        assert all(np.array_equal(a, b) for a, b in zip(got["masks"], plain["masks"])), what
        assert all(np.array_equal(a, b) for a, b in zip(got["chip_imgs"], plain["chip_imgs"])), what
        t, cw, ch, cws = _canvas(torch, im, w, h, h9s, keep)
        d_map = _dev(torch, cells) if cells is not None else None
        ctx.MosaicBlendedSeamDev(ptrs, w, h, ws, h9s, t.data_ptr(), cw, ch, cws, keep=keep, band=BAND, d_cells=d_map.data_ptr() if cells is not None else 0, **q)
        _same_canvas(t.cpu().numpy(), blended, name + ", " + what)
        if cells is None:
            _same_canvas(ctx.MosaicBlendedSeam(imgs, h9s, keep=keep, band=BAND, **q)[0], blended, name + ", host, " + what)
    ctx.close()


def test_refusals(oracle):
    """every parameter field outside its range, ramp != 0, a grid that is not the layout's, a wrong canvas, a missing frame: MI355_ERR_ARG,
    nothing written, and the ctx goes on working"""
    import torch
    import imagemosaicing_amd as im
    case, _, r = bp.reference(oracle, "crafted3")
    imgs, h9s, p = case.imgs, case.h9s, case.p
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    gh, gw = r["cells"].shape
    t, cw, ch, cws = _canvas(torch, im, w, h, h9s, None)
    d_cells = torch.full((gh * gw,), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    out = np.full((ch, cws), 0x5A, np.uint8)

    def forms(q, gw_=gw, gh_=gh, ptrs_=ptrs, imgs_=imgs, cw_=cw, geom=None):
        return (lambda: ctx.BlendSeamCellsDev(ptrs_, w, h, ws, h9s, d_cells.data_ptr(), gw_, gh_, **q),
                lambda: ctx.MosaicBlendedSeamDev(ptrs_, w, h, ws, h9s, t.data_ptr(), cw_, ch, cws, gw=gw_, gh=gh_, **q),
                lambda: ctx.ChipsAndMasksSeam(imgs_, h9s, cells=np.zeros((gh_, gw_), np.uint16), **q),
                lambda: ctx.MosaicBlendedSeam(imgs_, h9s, **q),
                lambda: ctx.MosaicBlendedSeamInto(imgs_, None, h9s, out=out, geom=geom, **q))

    def refused(fns, match, code=-1):
        for fn in fns:
            with pytest.raises(im.Mi355Error) as e:
                fn()
            assert e.value.code == code and match in str(e.value), str(e.value)
        assert (t == 7).all() and (d_cells == 0x7777).all() and (out == 0x5A).all()

    for field, bad in (("ramp", -1), ("ramp", 1), ("level", 1), ("level", 6), ("depth", 0), ("depth", 9), ("data_weight", -1), ("data_weight", 17),
                       ("diff_weight", -1), ("diff_weight", 17), ("seam_penalty", -1), ("seam_penalty", 256), ("miss_cost", -1), ("miss_cost", 256)):
        refused(forms(dict(p, **{field: bad})), field + "=")
    refused(forms(p, gw_=gw + 1)[:3], "grid")
    refused(forms(p, gh_=gh - 1)[:3], "grid")
    refused(forms(dict(p, level=p["level"] + 1))[:3], "grid")                        # the grid of another level
    refused(forms(p, cw_=cw + 1)[1:2], "geometry")
    missing = list(ptrs)
    missing[1] = 0
    refused(forms(p, ptrs_=missing)[:2], "image 1 ")
    refused(forms(p, imgs_=[imgs[0], None, imgs[2]], geom=[None, (w[1], h[1], ws[1]), None])[4:], "image 1")
    # a withheld frame that is dropped or skipped is not asked for
    keep = np.array([1, 0, 1], np.uint8)
    gwk, ghk = im.blend_seam_grid(w, h, h9s, p["level"], keep)
    dk = torch.zeros((ghk * gwk,), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.BlendSeamCellsDev(missing, w, h, ws, h9s, dk.data_ptr(), gwk, ghk, keep=keep, **p)
    # the ctx goes on working
    assert ctx.BlendSeamCellsDev(ptrs, w, h, ws, h9s, d_cells.data_ptr(), gw, gh, **p) == r["report"]
    ctx.MosaicBlendedSeamDev(ptrs, w, h, ws, h9s, t.data_ptr(), cw, ch, cws, **p)
    _same_canvas(t.cpu().numpy(), r["canvas"], "after the refusals")
    ctx.close()

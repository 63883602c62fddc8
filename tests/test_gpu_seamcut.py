"""GPU: the optimised seamlines (mi355_seam_candidates_dev / _labels_dev / _cells_dev, mi355_mosaic_seamcut / _dev / _into / _cover,
csrc/seamcut.hip) byte for byte against tests/seamcut_ref.py on every case of tests/seamcut_patterns.py, with pre-filled outputs so that
unwritten bytes show.

  * per case: the candidate records, the cell map, the report, and canvas, owner and count of the render; the one-call forms agree;
  * the label stage on records that come from no survey; the host twin and the device agree;
  * stripes down to single rows give the whole canvas's bytes;
  * the cover is exact: NULL for a frame it names is MI355_ERR_ARG before anything is written, NULL for any other changes nothing;
  * the host form, the _into form and the device form agree; every range error is refused and the ctx goes on working.
"""
import numpy as np
import pytest

from tests import seamcut_patterns as sp
from tests import seamcut_ref as sc
from tests import seamline_ref as sr

pytestmark = pytest.mark.gpu
FILL = (7, 0x3333, 0x5555)                                                  # canvas, owner, count before a call


def _upload(torch, imgs):
    from tests.test_gpu_gain import _upload as up
    return up(torch, imgs)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _pix(a, cw):
    return np.ascontiguousarray(a[:, :3 * cw]).reshape(a.shape[0], cw, 3)


class Out:
    """device canvas [ch, cws] uint8, owner and count [ch, cw] (int16 storage, read as uint16), pre-filled"""
    def __init__(self, torch, im, w, h, h9s, canvas=True):
        self.cw, self.ch, self.cws, _ = im.mosaic_layout(w, h, h9s)
        self.canvas = torch.full((self.ch, self.cws), FILL[0], dtype=torch.uint8, device="cuda") if canvas else None
        self.owner = torch.full((self.ch, self.cw), FILL[1], dtype=torch.int16, device="cuda")
        self.count = torch.full((self.ch, self.cw), FILL[2], dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()                                            # the fills run on torch's stream, the library on the ctx's own

    def render(self, ctx, ptrs, w, h, ws, h9s, p, d_cells, row0=0, rows=-1):
        ctx.MosaicSeamCutDev(ptrs, w, h, ws, h9s, self.canvas.data_ptr() if self.canvas is not None else 0, self.cw, self.ch, self.cws, row0, rows,
                             d_cells=d_cells, d_owner=self.owner.data_ptr(), d_count=self.count.data_ptr(), **p)
        return self

    def host(self):
        return (None if self.canvas is None else self.canvas.cpu().numpy(), self.owner.cpu().numpy().view(np.uint16), self.count.cpu().numpy().view(np.uint16))

    def untouched(self):
        return all(a is None or np.all(a == fill) for a, fill in zip(self.host(), FILL))


def _same(got, r, cw, what=""):
    canvas, owner, count = got
    for name, a, b in (("count", count, r["count"]), ("owner", owner, r["owner"]), ("canvas", _pix(canvas, cw), r["canvas"])):
        bad = a != b
        bad = bad.any(axis=2) if bad.ndim == 3 else bad
        assert a.shape == b.shape and not bad.any(), "%s %s: %d pixels differ, first %s" % (what, name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert not canvas[:, 3 * cw:].any()                                     # row padding zeroed


def _stages(torch, im, ctx, imgs, h9s, p, r):
    """stages 1 and 2 on the device, checked against r; returns (upload, d_cells tensor)"""
    up = _upload(torch, imgs)
    ts, ptrs, w, h, ws = up
    gh, gw = r["cells"].shape
    assert im.seam_grid(w, h, h9s, p["level"]) == (gw, gh)
    d_cand = torch.full((gh * gw * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    d_cells = torch.full((gh * gw,), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.SeamCandidatesDev(ptrs, w, h, ws, h9s, d_cand.data_ptr(), gw, gh, **p)
    rec = d_cand.cpu().numpy().reshape(gh, gw, 32)
    bad = (rec != r["records"]).any(axis=2)
    assert not bad.any(), "records: %d cells differ, first %s" % (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    rep = ctx.SeamLabelsDev(d_cand.data_ptr(), gw, gh, d_cells.data_ptr(), **p)
    cells = d_cells.cpu().numpy().view(np.uint16).reshape(gh, gw)
    assert np.array_equal(cells, r["cells"]), np.argwhere(cells != r["cells"])[:5].tolist()
    assert rep == r["report"], (rep, r["report"])
    return up, d_cells


@pytest.mark.parametrize("name", sorted(sp.CASES))
def test_case_equals_restatement(oracle, name):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, p, r = sp.reference(oracle, name)
    ctx = im.Context(0)
    (ts, ptrs, w, h, ws), d_cells = _stages(torch, im, ctx, imgs, h9s, p, r)
    gh, gw = r["cells"].shape
    # stages 1 and 2 in one call
    d2 = torch.full((gh * gw,), 0x1111, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert ctx.SeamCellsDev(ptrs, w, h, ws, h9s, d2.data_ptr(), gw, gh, **p) == r["report"]
    assert torch.equal(d2, d_cells)
    # the host twin on the device's records
    cells_h, rep_h = im.seam_labels_host(r["records"].copy().view(im.SEAM_CELL).reshape(gh, gw), **p)
    assert np.array_equal(cells_h, r["cells"]) and rep_h == r["report"]
    # stage 3, and all three stages in one call
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, p, d_cells.data_ptr())
    assert (o.ch, o.cw) == r["owner"].shape
    _same(o.host(), r, o.cw, name)
    o2 = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, p, 0)
    _same(o2.host(), r, o.cw, name + ", one call")
    # the maps alone: nothing is sampled, no frames needed
    o3 = Out(torch, im, w, h, h9s, canvas=False).render(ctx, None, w, h, None, h9s, p, d_cells.data_ptr())
    assert np.array_equal(o3.host()[1], r["owner"]) and np.array_equal(o3.host()[2], r["count"])
    # an all-zero cell map is the seamline render
    z = torch.zeros((gh * gw,), dtype=torch.int16, device="cuda")
    s = torch.full((o.ch, o.cws), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    oz = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, p, z.data_ptr())
    ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, s.data_ptr(), o.cw, o.ch, o.cws, ramp=p["ramp"])
    assert torch.equal(s, oz.canvas)
    ctx.close()


@pytest.mark.parametrize("name", sorted(sp.RECORD_CASES))
def test_labels_on_records(name):
    import torch
    import imagemosaicing_amd as im
    frame, omega, gray, p, cells, report, _ = sp.record_reference(name)
    gh, gw = cells.shape
    rec = sc.record_bytes(frame, omega, gray)
    ctx = im.Context(0)
    d_cand = _dev(torch, rec)
    d_cells = torch.full((gh * gw,), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rep = ctx.SeamLabelsDev(d_cand.data_ptr(), gw, gh, d_cells.data_ptr(), **p)
    got = d_cells.cpu().numpy().view(np.uint16).reshape(gh, gw)
    cells_h, rep_h = im.seam_labels_host(rec.copy().view(im.SEAM_CELL).reshape(gh, gw), **p)
    assert np.array_equal(got, cells) and rep == report
    assert np.array_equal(got, cells_h) and rep == rep_h
    ctx.close()


@pytest.mark.parametrize("name", ["crafted3", "projective"])
def test_stripes_equal_the_whole_canvas(oracle, name):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, p, r = sp.reference(oracle, name)
    ctx = im.Context(0)
    (ts, ptrs, w, h, ws), d_cells = _stages(torch, im, ctx, imgs, h9s, p, r)
    ch = r["owner"].shape[0]
    for cut in (1, 7, 100):
        o = Out(torch, im, w, h, h9s)
        for row0 in range(0, ch, cut):
            o.render(ctx, ptrs, w, h, ws, h9s, p, d_cells.data_ptr(), row0, min(cut, ch - row0))
        _same(o.host(), r, o.cw, "%s in stripes of %d" % (name, cut))
    # a stripe call writes its own rows only, in all three outputs
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, p, d_cells.data_ptr(), 30, 11)
    for a, fill in zip(o.host(), FILL):
        assert np.all(a[:30] == fill) and np.all(a[41:] == fill) and not np.all(a[30:41] == fill)
    ctx.close()


@pytest.mark.parametrize("name", ["crafted3", "nine_depth8", "skipped_level3"])
def test_cover_is_exact(oracle, name):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, p, r = sp.reference(oracle, name)
    n = len(imgs)
    ctx = im.Context(0)
    (ts, ptrs, w, h, ws), d_cells = _stages(torch, im, ctx, imgs, h9s, p, r)
    ch = r["owner"].shape[0]
    checked = 0
    for row0, rows in ((0, ch), (0, 9), (ch // 2, 1), (ch - 6, 6)):
        need = ctx.SeamCutCover(w, h, h9s, d_cells.data_ptr(), row0, rows, **p)
        own = np.unique(r["owner"][row0:row0 + rows])
        assert np.array_equal(np.flatnonzero(need), own[own > 0].astype(int) - 1), (row0, rows)
        # NULL for every frame the cover does not name: the same bytes
        held = [q if need[k] else 0 for k, q in enumerate(ptrs)]
        got = Out(torch, im, w, h, h9s).render(ctx, held, w, h, ws, h9s, p, d_cells.data_ptr(), row0, rows).host()
        for a, b in zip((_pix(got[0], r["owner"].shape[1]), got[1], got[2]), (r["canvas"], r["owner"], r["count"])):
            assert np.array_equal(a[row0:row0 + rows], b[row0:row0 + rows]), (row0, rows)
        # NULL for any frame it names: refused, naming it, before anything is written
        for k in np.flatnonzero(need):
            bad = list(held)
            bad[k] = 0
            o = Out(torch, im, w, h, h9s)
            with pytest.raises(im.Mi355Error) as e:
                o.render(ctx, bad, w, h, ws, h9s, p, d_cells.data_ptr(), row0, rows)
            assert e.value.code == -1 and "image %d " % k in str(e.value), str(e.value)
            assert o.untouched()
            checked += 1
    assert checked >= 4
    # the cover of the seamcut render is not the seamline render's wherever a frame lost all its pixels, and the ctx still works
    _same(Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, p, d_cells.data_ptr()).host(), r, r["owner"].shape[1], "after the refusals")
    ctx.close()


def test_host_into_and_device_forms_agree(oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, p, r = sp.reference(oracle, "relief3")
    ctx = im.Context(0)
    host, cw, ch, cws, own = ctx.MosaicSeamCut(imgs, h9s, want_owner=True, **p)
    assert (ch, cw) == r["owner"].shape and np.array_equal(_pix(host, cw), r["canvas"]) and np.array_equal(own, r["owner"]) and not host[:, 3 * cw:].any()
    host2, _, _, _ = ctx.MosaicSeamCut(imgs, h9s, **p)
    assert np.array_equal(host2, host)
    pitch = 3 * cw + 29
    out = np.full((ch, pitch), 201, np.uint8)
    out, cw3, ch3 = ctx.MosaicSeamCutInto(imgs, None, h9s, out=out, **p)
    assert (cw3, ch3) == (cw, ch) and np.array_equal(_pix(out, cw), r["canvas"]) and np.all(out[:, 3 * cw:] == 201)
    assert r["report"]["changed"] > 0 and (r["owner"] != sr.pick(r["maps"], r["wmaps"])[1]).any()      # not the seamline render
    ctx.close()


def test_refusals(oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, p, r = sp.reference(oracle, "crafted3")
    ctx = im.Context(0)
    (ts, ptrs, w, h, ws), d_cells = _stages(torch, im, ctx, imgs, h9s, p, r)
    gh, gw = r["cells"].shape
    o = Out(torch, im, w, h, h9s)
    d_cand = torch.full((gh * gw * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    d_new = torch.full((gh * gw,), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()

    def err(fn, code, match=""):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == code and match in str(e.value), str(e.value)

    for k, (lo, hi) in sc.RANGES.items():
        for v in ([lo - 1] if hi is None else [lo - 1, hi + 1]):
            q = dict(p, **{k: v})
            tag = "%s=%d" % (k, v)
            gwq, ghq = (gw, gh) if k != "level" else (1, 1)
            err(lambda: ctx.SeamCandidatesDev(ptrs, w, h, ws, h9s, d_cand.data_ptr(), gwq, ghq, **q), -1, tag)
            err(lambda: ctx.SeamLabelsDev(d_cand.data_ptr(), gw, gh, d_new.data_ptr(), **q), -1, tag)
            err(lambda: ctx.SeamCellsDev(ptrs, w, h, ws, h9s, d_new.data_ptr(), gwq, ghq, **q), -1, tag)
            err(lambda: o.render(ctx, ptrs, w, h, ws, h9s, q, d_cells.data_ptr()), -1, tag)
            err(lambda: o.render(ctx, ptrs, w, h, ws, h9s, q, 0), -1, tag)
            err(lambda: ctx.SeamCutCover(w, h, h9s, d_cells.data_ptr(), **q), -1, tag)
            err(lambda: ctx.MosaicSeamCut(imgs, h9s, **q), -1, tag)
            err(lambda: ctx.MosaicSeamCutInto(imgs, None, h9s, **q), -1, tag)
    # a grid that is not the layout's; a frame of stage 1 without a pointer; all outputs NULL; a canvas without frames; a wrong canvas
    err(lambda: ctx.SeamCandidatesDev(ptrs, w, h, ws, h9s, d_cand.data_ptr(), gw + 1, gh, **p), -1, "grid")
    err(lambda: ctx.SeamCellsDev(ptrs, w, h, ws, h9s, d_new.data_ptr(), gw, gh + 1, **p), -1, "grid")
    err(lambda: ctx.SeamCellsDev(ptrs, w, h, ws, h9s, d_new.data_ptr(), 1 << 20, 1 << 20, **p), -1, "grid")      # refused before 2^40 records are asked for
    err(lambda: ctx.SeamCandidatesDev([ptrs[0], 0] + list(ptrs[2:]), w, h, ws, h9s, d_cand.data_ptr(), gw, gh, **p), -1, "image 1 ")
    err(lambda: ctx.MosaicSeamCutDev(ptrs, w, h, ws, h9s, 0, o.cw, o.ch, o.cws, d_cells=d_cells.data_ptr(), **p), -1, "all NULL")
    err(lambda: ctx.MosaicSeamCutDev(None, w, h, ws, h9s, o.canvas.data_ptr(), o.cw, o.ch, o.cws, d_cells=d_cells.data_ptr(), **p), -1, "d_imgs")
    err(lambda: ctx.MosaicSeamCutDev(ptrs, w, h, ws, h9s, o.canvas.data_ptr(), o.cw + 1, o.ch, o.cws, d_cells=d_cells.data_ptr(), **p), -1, "canvas geometry")
    err(lambda: ctx.MosaicSeamCut(imgs[:1], h9s[:1], **p), -2)
    assert o.untouched() and np.all(d_cand.cpu().numpy() == 0xAB) and np.all(d_new.cpu().numpy() == 0x7777)             # no refusal wrote anything
    _same(Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, p, d_cells.data_ptr()).host(), r, o.cw, "after the refusals")
    ctx.close()

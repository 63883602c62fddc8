"""GPU: the optimised seamlines (csrc/seamcut.hip: seam_candidates_kernel, seam_path_kernel, seam_argmin_kernel, seam_energy_kernel,
seam_finish_kernel, seamcut_tile_kernel) at the warp stage's edges and past a wave of frames, byte for byte against tests/seamcut_ref.py.

  * every case of tests/render_patterns.py -- quarter turns, mirrors, m8 = 2, -1 and 0, a frame without an inverse, 40 frames on one tile,
    canvases 1 .. 257 wide and high, overlap across a list-block corner -- at seamcut_patterns.EDGE_SETTINGS: the records, the cell map and
    report, the render with the device's cell map, in one call, and the maps alone;
  * the same cases under cell maps that stage 2 did not make: random ones that name nobody or any frame (skipped ones, the one without an
    inverse, frames that do not touch the cell), and one that names a frame beyond the last, which is the seamline render;
  * stripes of 1, 7 and 100 rows; the cover and withheld frames under random cell maps; a layout that is refused;
  * seamcut_patterns.WAVE_CASES (more frames in one list block than a wave has lanes: the per-lane top 8 of seam_candidates_kernel holds more
    than one key, loses its ninth, and is popped eight times) at depth 8, 4 and 1, and REM_CASES (the probe clamp at every level);
  * seamcut_patterns.RECORD_EDGE_CASES (up to 8 filled slots, frame ids up to 65535) through the device's label stage and the host twin.
Every comparison is np.array_equal on bytes or integers or equality of the report dict.  Outputs are pre-filled with a sentinel and carry a
guard (a canvas row, 64 map entries, 64 cells, two records) beyond their end that must stay as it was.
(tests/test_seamcut_edges_ref.py shows without a GPU that each case holds what it is for.)
"""
import numpy as np
import pytest

from tests import render_patterns as rp
from tests import seamcut_patterns as sp
from tests import seamcut_ref as sc
from tests.test_gpu_render_edges import COVER_TAGS, FILL, GUARD, SENT8, _frames, _only, _refused, _some, check_canvas, check_map

pytestmark = pytest.mark.gpu

CASES = rp.cases()
TAGS = {c.tag: c for c in CASES}
LEVELS = tuple(l for l, _, _ in sp.EDGE_SETTINGS)
CASE_LEVELS = [(c, l) for c in CASES for l in LEVELS]
CASE_LEVEL_IDS = ["%s-L%d" % (c.tag, l) for c, l in CASE_LEVELS]
STRIPE_TAGS = ("straddle_overlap", "turns", "forty", "canvas_h257")
SENT_REC, SENT_CELL = 0xAB, 0x7777
KINDS = ("canvas", "owner", "count")


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


class Out:
    """sentinel-filled device outputs of a cw x ch canvas: "canvas" [ch + 1, cws] uint8, "owner" / "count" [ch * cw + GUARD] uint16"""
    def __init__(self, d, h9s, kinds=KINDS):
        import torch
        import imagemosaicing_amd as im
        self.cw, self.ch, self.cws, _ = im.mosaic_layout(d[2], d[3], h9s)
        self.t = {k: (torch.full((self.ch + 1, self.cws), SENT8, dtype=torch.uint8, device="cuda") if k == "canvas" else
                      torch.full((self.ch * self.cw + GUARD,), FILL[k], dtype=torch.int16, device="cuda")) for k in kinds}
        torch.cuda.synchronize()                                            # the fills run on torch's stream, the library on the ctx's own

    def ptr(self, k):
        return self.t[k].data_ptr() if k in self.t else 0

    def render(self, ctx, d, h9s, p, d_cells, ptrs=None, row0=0, rows=-1):
        """with a canvas: the frames d (ptrs: d's pointers with some withheld); without: the maps alone, no frames given"""
        frames = "canvas" in self.t
        ctx.MosaicSeamCutDev((d[1] if ptrs is None else ptrs) if frames else None, d[2], d[3], d[4] if frames else None, h9s, self.ptr("canvas"),
                             self.cw, self.ch, self.cws, row0, rows, d_cells=d_cells, d_owner=self.ptr("owner"), d_count=self.ptr("count"), **p)
        return self

    def host(self, k):
        a = self.t[k].cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a

    def untouched(self):
        return all((self.host(k) == FILL[k]).all() for k in self.t)

    def check(self, ref, what, rows=None):
        """ref: (canvas, owner, count) or a dict that holds them"""
        ref = dict(zip(KINDS, ref)) if isinstance(ref, tuple) else ref
        assert ref["owner"].shape == (self.ch, self.cw), what
        for k in self.t:
            if k == "canvas":
                check_canvas(self.host(k), ref[k], self.cw, self.ch, what, rows)
            else:
                check_map(self.host(k), ref[k], self.cw, self.ch, FILL[k], f"{what} {k}", rows)


def _upload(imgs):
    import torch
    ts = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in imgs]
    torch.cuda.synchronize()
    return (ts, [t.data_ptr() for t in ts], [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], [3 * a.shape[1] for a in imgs])


class Cells:
    """a uint16 [gh, gw] cell map on the device with GUARD entries behind it: sentinel-filled for a stage to write, or holding `cells`"""
    def __init__(self, gw, gh, cells=None):
        import torch
        self.gw, self.gh = gw, gh
        a = np.full(gh * gw + GUARD, SENT_CELL, np.uint16)
        if cells is not None:
            assert cells.shape == (gh, gw)
            a[:gh * gw] = cells.ravel()
        self.t = torch.from_numpy(a.view(np.int16)).cuda()
        torch.cuda.synchronize()

    def ptr(self):
        return self.t.data_ptr()

    def host(self, what):
        a = self.t.cpu().numpy().view(np.uint16)
        assert (a[self.gh * self.gw:] == SENT_CELL).all(), f"{what}: cells beyond gh * gw were written"
        return a[:self.gh * self.gw].reshape(self.gh, self.gw)


def _stages(ctx, d, h9s, p, r, what):
    """stages 1 and 2 on the device against r (records, cells, report), in two calls and in one; returns the device's cell map"""
    import torch
    import imagemosaicing_amd as im
    gh, gw = r["cells"].shape
    assert im.seam_grid(d[2], d[3], h9s, p["level"]) == (gw, gh), what
    d_cand = torch.full(((gh * gw + 2) * 32,), SENT_REC, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.SeamCandidatesDev(d[1], d[2], d[3], d[4], h9s, d_cand.data_ptr(), gw, gh, **p)
    rec = d_cand.cpu().numpy()
    assert (rec[gh * gw * 32:] == SENT_REC).all(), f"{what}: records beyond gh * gw were written"
    rec = rec[:gh * gw * 32].reshape(gh, gw, 32)
    bad = (rec != r["records"]).any(axis=2)
    if bad.any():
        y, x = (int(v) for v in np.argwhere(bad)[0])
        got = rec[y, x].copy().view(im.SEAM_CELL)[0]
        raise AssertionError(f"{what} records: {int(bad.sum())} of {gh * gw} cells differ, first at cell x {x} y {y}: got frame {got['frame'].tolist()} omega "
                             f"{got['omega'].tolist()} gray {got['gray'].tolist()}, expected frame {r['frame'][y, x].tolist()} omega {r['omega'][y, x].tolist()} "
                             f"gray {r['gray'][y, x].tolist()}")
    one = Cells(gw, gh)
    rep = ctx.SeamLabelsDev(d_cand.data_ptr(), gw, gh, one.ptr(), **p)
    cells = one.host(what)
    assert np.array_equal(cells, r["cells"]), f"{what} cells: first differences at {np.argwhere(cells != r['cells'])[:5].tolist()}"
    assert rep == r["report"], (what, rep, r["report"])
    both = Cells(gw, gh)
    assert ctx.SeamCellsDev(d[1], d[2], d[3], d[4], h9s, both.ptr(), gw, gh, **p) == r["report"], what
    assert np.array_equal(both.host(what + ", stages 1 and 2 in one call"), cells), what
    return one


def _renders(ctx, d, h9s, p, r, cells, what):
    """stage 3 with a cell map, all three stages in one call, and the maps alone without frames"""
    Out(d, h9s).render(ctx, d, h9s, p, cells.ptr()).check(r, what)
    Out(d, h9s).render(ctx, d, h9s, p, 0).check(r, what + ", all stages in one call")
    Out(d, h9s, ("owner", "count")).render(ctx, d, h9s, p, cells.ptr()).check(r, what + ", the maps alone")


def _foreign_maps(case, r, level):
    """[(name, cells)]: two random cell maps, and one that names a frame beyond the last everywhere"""
    gh, gw = r["cells"].shape
    n = len(case.imgs)
    return [("random cell map %d" % seed, sp.random_cells(n, gw, gh, 1000 * level + seed)) for seed in (0, 1)] + [("cell map of n + 1", np.full((gh, gw), n + 1, np.uint16))]


# ---- the cases of tests/render_patterns.py ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,level", CASE_LEVELS, ids=CASE_LEVEL_IDS)
def test_gpu_stages_equal_restatement_on_render_patterns(ctx, oracle, case, level):
    p, r = sp.edge_reference(oracle, case, level)
    d = _frames(case)
    what = f"{case.tag} level {level}"
    cells = _stages(ctx, d, case.h9s, p, r, what)
    _renders(ctx, d, case.h9s, p, r, cells, what)


@pytest.mark.parametrize("case,level", CASE_LEVELS, ids=CASE_LEVEL_IDS)
def test_gpu_render_follows_foreign_cell_maps(ctx, oracle, case, level):
    """stage 3 under cell maps stage 2 did not make: wanted frames that cover part of a cell, none of it, are skipped (m8 == 0), have no
    inverse, or are no frame at all"""
    R = rp.restate(oracle, case)
    p, r = sp.edge_reference(oracle, case, level)
    d = _frames(case)
    gh, gw = r["cells"].shape
    for name, cells in _foreign_maps(case, r, level):
        want = sc.render(R.maps, R.weights(p["ramp"]), cells, level)
        dc = Cells(gw, gh, cells)
        what = f"{case.tag} level {level}, {name}"
        Out(d, case.h9s).render(ctx, d, case.h9s, p, dc.ptr()).check(want, what)
        Out(d, case.h9s, ("owner", "count")).render(ctx, d, case.h9s, p, dc.ptr()).check(want, what + ", the maps alone")
        assert np.array_equal(dc.host(what), cells)                         # the render reads the cell map only
        if name.endswith("n + 1"):
            s = R.seamline(p["ramp"])
            assert all(np.array_equal(a, b) for a, b in zip(want, s[:3])), what


@pytest.mark.parametrize("tag", STRIPE_TAGS)
def test_gpu_stripes_equal_the_whole(ctx, oracle, tag):
    """stripes of 1, 7 and 100 rows, side by side in one sentinel-filled set of outputs, are the whole canvas and its maps, under the device's
    cell map (level 3) and under random ones (levels 2 and 5); one stripe call writes its own rows only"""
    case = TAGS[tag]
    R = rp.restate(oracle, case)
    d = _frames(case)
    for level in LEVELS:
        p, r = sp.edge_reference(oracle, case, level)
        gh, gw = r["cells"].shape
        if level == 3:
            cells, want, name = _stages(ctx, d, case.h9s, p, r, f"{tag} level {level}"), r, "the device's cell map"
        else:
            name, c = _foreign_maps(case, r, level)[0]
            cells, want = Cells(gw, gh, c), sc.render(R.maps, R.weights(p["ramp"]), c, level)
        for cut in (1, 7, 100):
            o = Out(d, case.h9s)
            for row0 in range(0, o.ch, cut):
                o.render(ctx, d, case.h9s, p, cells.ptr(), row0=row0, rows=min(cut, o.ch - row0))
            o.check(want, f"{tag} level {level}, {name}, in stripes of {cut}")
        for row0, rows in {(R.ch // 3, max(1, R.ch // 2)), (R.ch - 1, 1), (0, 1)}:
            o = Out(d, case.h9s).render(ctx, d, case.h9s, p, cells.ptr(), row0=row0, rows=rows)
            o.check(want, f"{tag} level {level}, {name}, rows {row0}..{row0 + rows - 1}", rows=(row0, rows))


@pytest.mark.parametrize("tag", COVER_TAGS)
def test_gpu_cover_and_withheld_frames_under_foreign_cell_maps(ctx, oracle, tag):
    case = TAGS[tag]
    R = rp.restate(oracle, case)
    d = _frames(case)
    checked = 0
    for level in LEVELS:
        p, r = sp.edge_reference(oracle, case, level)
        gh, gw = r["cells"].shape
        name, c = _foreign_maps(case, r, level)[0]
        cells, want = Cells(gw, gh, c), sc.render(R.maps, R.weights(p["ramp"]), c, level)
        for row0, rows in ((0, R.ch), (0, 1), (R.ch // 3, max(1, R.ch // 2))):
            what = f"{tag} level {level}, {name}, rows {row0}..{row0 + rows - 1}"
            part = want[1][row0:row0 + rows]
            owners = (np.unique(part[part > 0]).astype(int) - 1).tolist()
            need = ctx.SeamCutCover(d[2], d[3], case.h9s, cells.ptr(), row0, rows, **p)
            assert np.flatnonzero(need).tolist() == owners, (what, np.flatnonzero(need).tolist(), owners)
            assert not any(need[k] for k in rp.skipped(case, R))
            # NULL for every frame the cover does not name: the same bytes
            Out(d, case.h9s).render(ctx, d, case.h9s, p, cells.ptr(), ptrs=_only(d[1], owners), row0=row0, rows=rows).check(want, what + ", the rest withheld", rows=(row0, rows))
            # NULL for one it names: refused, naming it, with nothing written; the ctx goes on working
            for k in (_some(owners) if owners else []):
                bad = Out(d, case.h9s)
                _refused(ctx, lambda: bad.render(ctx, d, case.h9s, p, cells.ptr(), ptrs=_only(d[1], [q for q in owners if q != k]), row0=row0, rows=rows), k)
                assert bad.untouched(), f"{what}: the refused call wrote something"
                checked += 1
        Out(d, case.h9s).render(ctx, d, case.h9s, p, cells.ptr()).check(want, f"{tag} level {level}, {name}, after the refusals")
    assert checked >= 6


def test_gpu_refused_layout_is_refused_by_every_entry(ctx):
    """no frame with m8 != 0: there is no canvas; every entry says so and writes nothing"""
    import torch
    import imagemosaicing_amd as im
    imgs = sp._noise_frames([(16, 12), (16, 12)], 3)
    h9s = sp._translations([(0, 0), (5, 3)])
    h9s[:, 8] = 0
    d = _upload(imgs)
    with pytest.raises(im.Mi355Error):
        im.mosaic_layout(d[2], d[3], h9s)
    p = sc.params(level=2, depth=8)
    cw, ch, cws = 21, 15, 64                                                # what the layout would be with m8 = 1
    canvas = torch.full((ch + 1, cws), SENT8, dtype=torch.uint8, device="cuda")
    owner = torch.full((ch * cw + GUARD,), FILL["owner"], dtype=torch.int16, device="cuda")
    d_cand = torch.full((6 * 4 * 32,), SENT_REC, dtype=torch.uint8, device="cuda")
    cells = Cells(6, 4)
    given = Cells(6, 4, np.ones((4, 6), np.uint16))
    for call in (lambda: ctx.SeamCandidatesDev(d[1], d[2], d[3], d[4], h9s, d_cand.data_ptr(), 6, 4, **p),
                 lambda: ctx.SeamCellsDev(d[1], d[2], d[3], d[4], h9s, cells.ptr(), 6, 4, **p),
                 lambda: ctx.MosaicSeamCutDev(d[1], d[2], d[3], d[4], h9s, canvas.data_ptr(), cw, ch, cws, d_cells=given.ptr(), d_owner=owner.data_ptr(), **p),
                 lambda: ctx.MosaicSeamCutDev(d[1], d[2], d[3], d[4], h9s, canvas.data_ptr(), cw, ch, cws, d_cells=0, d_owner=owner.data_ptr(), **p),
                 lambda: ctx.MosaicSeamCutDev(None, d[2], d[3], None, h9s, 0, cw, ch, cws, d_cells=given.ptr(), d_owner=owner.data_ptr(), **p),
                 lambda: ctx.SeamCutCover(d[2], d[3], h9s, given.ptr(), **p)):
        with pytest.raises(im.Mi355Error) as e:
            call()
        assert e.value.code != 0 and "h[8]" in str(e.value), str(e.value)
    assert (canvas.cpu().numpy() == SENT8).all() and (owner.cpu().numpy().view(np.uint16) == FILL["owner"]).all() and (d_cand.cpu().numpy() == SENT_REC).all()
    assert (cells.t.cpu().numpy().view(np.uint16) == SENT_CELL).all()


# ---- past a wave of frames, and the probe clamp -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sp.SURVEY_EDGE_CASES))
def test_gpu_wave_and_remainder_cases_equal_restatement(ctx, oracle, name):
    imgs, h9s, p, r = sp.reference(oracle, name)
    d = _upload(imgs)
    cells = _stages(ctx, d, h9s, p, r, name)
    _renders(ctx, d, h9s, p, r, cells, name)
    if name in sp.WAVE_CASES:
        for depth in (4, 1):                                                # the same uploaded frames; the candidates are a prefix
            q, rs = sp.shallower(r, p, depth)
            what = f"{name} depth {depth}"
            cells = _stages(ctx, d, h9s, q, rs, what)
            _renders(ctx, d, h9s, q, sc.render(r["maps"], r["wmaps"], rs["cells"], q["level"]), cells, what)


# ---- records that come from no survey -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sp.RECORD_EDGE_CASES))
def test_gpu_labels_on_records_with_eight_slots(ctx, name):
    import torch
    import imagemosaicing_amd as im
    frame, omega, gray, p, cells, report, _ = sp.record_reference(name)
    gh, gw = cells.shape
    rec = sc.record_bytes(frame, omega, gray)
    d_cand = torch.from_numpy(np.ascontiguousarray(rec).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    out = Cells(gw, gh)
    rep = ctx.SeamLabelsDev(d_cand.data_ptr(), gw, gh, out.ptr(), **p)
    got = out.host(name)
    cells_h, rep_h = im.seam_labels_host(rec.copy().view(im.SEAM_CELL).reshape(gh, gw), **p)
    assert np.array_equal(got, cells) and rep == report, (name, np.argwhere(got != cells)[:5].tolist(), rep, report)
    assert np.array_equal(got, cells_h) and rep == rep_h
    assert np.array_equal(d_cand.cpu().numpy().reshape(rec.shape), rec)     # the label stage reads the records only

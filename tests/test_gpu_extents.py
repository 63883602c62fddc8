"""GPU: renders, statistics, chips and blend, overviews, warps and frame passes where a canvas or frame coordinate passes 65 535, byte for byte
against the references the smaller cases use (tests/extent_patterns.py holds the cases; tests/test_extent_patterns_ref.py shows without a GPU
that each case holds what it is for and would notice a coordinate, a list-block index or a workgroup row cut to 16 bits).

  * canvases 69 172 wide and 69 156 high (plain shifts; a yaw and a projective matrix with a frame of m8 = 0 between; a 69 200-pixel ribbon
    frame; 70 frames on one spot at x = 69 000), 262 221 high and 1 048 653 high: the refined render against the oracle; feathered,
    seamline and median against feather_ref, seamline_ref and median_ref; the optimised seamlines' records, cell map, report and render
    against seamcut_ref; stripes that start past row 65 535 and end on the last row (on the million-row canvas: at row 65 535 * 16); the
    stripe, seamline, median and seamcut covers of such stripes;
  * the gain, block-gain and sharpness statistics of the far pairs;
  * chips and masks and the multiband blend (whole canvas and a stripe above row 65 536) on the 69k cases and on the 262k and million-row
    canvases: blend.hip's launches hold one canvas row per workgroup row, owner_kernel 16; the blend along optimised seams on the 69k cases;
  * every overview level and the preview on the 69k canvases.  The threshold of csrc/overview.hip sits at rows / 128 > 65 535: a canvas of
    8.4 million rows, which is out of scope here;
  * single warps of 3 x 262 200 and (under a quarter turn) 262 200 x 3 sources: results taller than 4 * 65 535 rows;
  * the frame passes on frames 65 537 and 2^20 long, in place and out of place, on the pitches 3 w and 3 w + 5.

The median restatement takes seconds per million pixels, so on canvases above a million pixels it is made on a window only: every line (row of
a tall canvas, column of a wide one) within 40 of a line some frame covers, every 4099th line, and the lines around 65 536 and 65 535 * 4 and
* 16; on the million-row canvas that keeps it under a second per depth where the whole took 15.  All other lines are expected -- and compared
-- as zero with the rest, and once more on the device with a torch reduction.
Every comparison is np.array_equal on bytes or integers; outputs are pre-filled with a sentinel and carry a guard beyond their end.
"""
import numpy as np
import pytest

from tests import block_gain_ref as br
from tests import extent_patterns as ep
from tests import gain_ref as gr
from tests import median_ref as mr
from tests import overview_ref as ovr
from tests import render_patterns as rp
from tests import seamcut_patterns as scp
from tests import seamcut_ref as sc
from tests import sharp_ref as shr
from tests.test_gpu_render_edges import RENDERS, Out, _frames, check_canvas, check_records

pytestmark = pytest.mark.gpu

CASES = ep.canvas_cases()
IDS = [c.tag for c in CASES]
TAGS = {c.tag: c for c in CASES}
TALL = [c for c in CASES if c.axis == 0]
BLEND = [c for c in CASES if c.blend]
TALLEST = [c for c in CASES if c.tag in ("tall_262k", "tall_1m")]           # chips and blend only: the blend-seam restatement walks every cell
MEDIAN_DEPTHS = (1, 5, 9)
WINDOW_ABOVE = 1 << 20                                                      # pixels of a canvas above which the median is restated on a window
MARGIN, EVERY = 40, 4099
BAND = 5


def _ids(cases):
    return [c.tag for c in cases]


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    from tests import test_gpu_render_edges as tre
    c = im.Context(0)
    yield c
    c.close()
    for case in CASES:                                                      # a million-row case holds gigabytes of maps: not for the rest of the session
        rp._RESTATED.pop(case.tag, None)
        tre._DEV.pop(case.tag, None)
    _MEDIAN.clear()
    _CUT.clear()


def _R(oracle, case):
    return rp.restate(oracle, case.render)


def _D(case):
    return _frames(case.render)


def _far_stripe(case, r):
    """a stripe that starts past row 65 535 and ends on the last row; on the million-row canvas it starts at 65 535 * 16"""
    row0 = 65535 * 16 if r.ch > 65535 * 16 else (65535 * 4 + 1 if r.ch > 65535 * 4 else 65536 + 7)
    return row0, r.ch - row0


# ---- the median on a window -------------------------------------------------------------------------------------------------------------------
_MEDIAN = {}


def _lines(case, r):
    """(the window's line indices along the case's axis, the lines nobody covers)"""
    n = r.ch if case.axis == 0 else r.cw
    covered = np.zeros(n, bool)
    for m in r.maps:
        if m is not None:
            covered |= m[1].any(axis=1 - case.axis)
    near = np.convolve(covered, np.ones(2 * MARGIN + 1), "same") > 0
    near[::EVERY] = True
    for t in (65536,) + tuple(65535 * k for k in ep.ROWS_PER_WORKGROUP):
        if t < n:
            near[max(0, t - 2):t + 2] = True
    return np.flatnonzero(near), np.flatnonzero(~covered)


def _median(case, r, ramp, depth):
    """({canvas, spread, count} of the whole canvas, selected [depth, ch, cw] or -- on a window -- None with the window's own selected set)"""
    key = (case.tag, ramp, depth)
    if key not in _MEDIAN:
        if r.cw * r.ch <= WINDOW_ABOVE:
            m = r.median(ramp, depth)
            _MEDIAN[key] = (dict(canvas=m[0], spread=m[1], count=m[2]), m[3], None)
        else:
            idx, _ = _lines(case, r)
            cut = lambda mm: [None if m is None else tuple(np.take(a, idx, axis=case.axis) for a in m) for m in mm]
            m = mr.pick(cut(r.maps), cut(r.weights(ramp)), depth)
            full = dict(canvas=np.zeros((r.ch, r.cw, 3), np.uint8), spread=np.zeros((r.ch, r.cw), np.uint8), count=np.zeros((r.ch, r.cw), np.uint16))
            for k, a in zip(("canvas", "spread", "count"), m[:3]):
                if case.axis == 0:
                    full[k][idx] = a
                else:
                    full[k][:, idx] = a
            _MEDIAN[key] = (full, m[3], idx)
    return _MEDIAN[key]


def _uncovered_is_zero(case, r, o, what):
    """on the device: every line nobody covers is zero in every output"""
    import torch
    _, empty = _lines(case, r)
    if not len(empty):
        return
    e = torch.from_numpy(empty).cuda()
    for k, t in o.t.items():
        if k == "canvas":
            a = t[:r.ch]
            bad = a.index_select(0, e).any() if case.axis == 0 else a[:, :3 * r.cw].reshape(r.ch, r.cw, 3).index_select(1, e).any()
        else:
            a = t[:r.ch * r.cw].reshape(r.ch, r.cw)
            bad = a.index_select(case.axis, e).any()
        assert not bool(bad), f"{what} {k}: a line nobody covers is not zero"


# ---- renders ------------------------------------------------------------------------------------------------------------------------------------
def _refined(ctx, d, case, o, row0=0, rows=-1):
    ctx.MosaicImagesRefinedDev(d[1], d[2], d[3], d[4], case.render.h9s, o.ptr("canvas"), o.cw, o.ch, o.cws, row0, rows)
    ctx.synchronize()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_refined_equals_oracle(ctx, oracle, case):
    r, d = _R(oracle, case), _D(case)
    want = np.ascontiguousarray(r.refined[:, :3 * r.cw]).reshape(r.ch, r.cw, 3)
    o = Out(r, ("canvas",))
    _refined(ctx, d, case, o)
    check_canvas(o.host("canvas"), want, r.cw, r.ch, f"{case.tag} refined")
    if case.axis == 0:
        row0, rows = _far_stripe(case, r)
        o = Out(r, ("canvas",))
        _refined(ctx, d, case, o, row0, rows)
        check_canvas(o.host("canvas"), want, r.cw, r.ch, f"{case.tag} refined rows {row0}..", rows=(row0, rows))
        assert want[row0:].any(), case.tag
        exact = ctx.StripeCover(d[2], d[3], case.render.h9s, row0, rows, exact=True)
        top = r.top[row0:]
        assert np.flatnonzero(exact).tolist() == np.unique(top[top >= 0]).tolist(), case.tag


@pytest.mark.parametrize("ramp", rp.RAMPS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_feathered_equals_restatement(ctx, oracle, case, ramp):
    r, d = _R(oracle, case), _D(case)
    kinds, call, ref = RENDERS["feathered"]
    o = Out(r, kinds)
    call(ctx, d, case.render, o, ramp, 0)
    o.check(ref(r, ramp, 0), f"{case.tag} feathered ramp {ramp}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_seamline_equals_restatement(ctx, oracle, case):
    """the canvas with the owner and count maps; ramp 0, and 3 where the canvas is below a million rows"""
    r, d = _R(oracle, case), _D(case)
    kinds, call, ref = RENDERS["seamline"]
    for ramp in rp.RAMPS if r.ch < (1 << 20) else (0,):
        o = Out(r, kinds)
        call(ctx, d, case.render, o, ramp, 0)
        o.check(ref(r, ramp, 0), f"{case.tag} seamline ramp {ramp}")


@pytest.mark.parametrize("depth", MEDIAN_DEPTHS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_median_equals_restatement(ctx, oracle, case, depth):
    r, d = _R(oracle, case), _D(case)
    kinds, call, _ = RENDERS["median"]
    want, _, idx = _median(case, r, 0, depth)
    o = Out(r, kinds)
    call(ctx, d, case.render, o, 0, depth)
    o.check(want, f"{case.tag} median depth {depth}")
    _uncovered_is_zero(case, r, o, f"{case.tag} median depth {depth}")
    assert (depth == 1 or want["spread"].any()) and int(want["count"].max()) >= 2, case.tag


@pytest.mark.parametrize("case", TALL, ids=_ids(TALL))
def test_gpu_far_stripes_equal_the_whole(ctx, oracle, case):
    """feathered, seamline and median (depths 1 and 5: two rows and one row per lane) on the stripe that starts past row 65 535 -- on the
    million-row canvas at 65 535 * 16 -- and ends on the last row: the whole render's rows, nothing outside them written; and the covers of
    that stripe name the frames that own or are selected in it"""
    r, d = _R(oracle, case), _D(case)
    row0, rows = _far_stripe(case, r)
    h9s = case.render.h9s
    for render, depth in (("feathered", 0), ("seamline", 0), ("median", 1), ("median", 5)):
        kinds, call, ref = RENDERS[render]
        want = _median(case, r, 0, depth)[0] if render == "median" else ref(r, 0, 0)
        o = Out(r, kinds)
        call(ctx, d, case.render, o, 0, depth, row0=row0, rows=rows)
        o.check(want, f"{case.tag} {render} depth {depth} rows {row0}..{row0 + rows - 1}", rows=(row0, rows))
        assert want["canvas"][row0:].any(), case.tag
    part = r.seamline(0)[1][row0:]
    owners = (np.unique(part[part > 0]).astype(int) - 1).tolist()
    assert owners and np.flatnonzero(ctx.SeamlineCover(d[2], d[3], h9s, row0, rows, ramp=0)).tolist() == owners, case.tag
    box = [k for k, m in enumerate(r.maps) if m is not None and m[1][row0:].any()]
    assert np.flatnonzero(ctx.StripeCover(d[2], d[3], h9s, row0, rows)).tolist() == box, case.tag
    for depth in (1, 5):
        _, sel, idx = _median(case, r, 0, depth)
        part = sel[:, row0:] if idx is None else sel[:, idx >= row0]
        inside = (np.unique(part[part > 0]).astype(int) - 1).tolist()
        assert inside and np.flatnonzero(ctx.MedianCover(d[2], d[3], h9s, row0, rows, depth=depth)).tolist() == inside, (case.tag, depth)


# ---- optimised seamlines --------------------------------------------------------------------------------------------------------------------------
_CUT = {}
LABELS_LEAVE_SLOT_0 = ("wide_69k", "tall_69k", "ribbon_x", "ribbon_y")      # there the label stage names a frame in a far cell


def _cut_settings(case, r):
    """the label stage's restatement walks the cells one by one.  Level 3 (data_weight 0, so that the labels leave slot 0 in far cells) on the
    69k canvases and the ribbons; level 5 at depth 8 on the 70 frames and on the 262k canvas; none on the million rows"""
    if r.ch >= (1 << 20):
        return ()
    if case.tag in ("far_many", "tall_262k"):
        return (sc.params(level=5, depth=8, data_weight=0),)
    return (sc.params(level=3, depth=4, data_weight=0),)


def _cut_reference(oracle, case, r, p):
    key = (case.tag, p["level"])
    if key not in _CUT:
        _CUT[key] = sc.seamcut_ref(oracle, case.render.imgs, case.render.h9s, p, maps=r.maps, wmaps=r.weights(p["ramp"]))
    return _CUT[key]


def _far_cells(case, a, level):
    return a[65536 >> level:] if case.axis == 0 else a[:, 65536 >> level:]


def _cut_records(case, r, p):
    """seamcut_ref.candidates; some far cell holds two candidates or more"""
    frame, omega, gray = sc.candidates(r.maps, r.weights(p["ramp"]), p["level"], p["depth"])
    assert _far_cells(case, frame, p["level"])[..., 1].any(), case.tag
    return frame, omega, gray


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_seamcut_equals_restatement(ctx, oracle, case):
    """records, cell map, report and render (at level 3: cell indices cy * gw + cx up to 52 000, and the labels name a frame in some far
    cell); the render under a random cell map, whole and on the far stripe, with the cover of that stripe.  On the million-row canvas the
    label stage's restatement would take a minute: there, and on the other canvases whose labels are compared at level 5 only, the records of
    level 3 at depth 8 are compared on their own"""
    from tests.test_gpu_seamcut_edges import Cells, Out as CutOut, _renders, _stages
    r, d = _R(oracle, case), _D(case)
    h9s = case.render.h9s
    for p in _cut_settings(case, r):
        ref = _cut_reference(oracle, case, r, p)
        what = f"{case.tag} level {p['level']}"
        cells = _stages(ctx, d, h9s, p, ref, what)
        _renders(ctx, d, h9s, p, ref, cells, what)
        assert case.tag not in LABELS_LEAVE_SLOT_0 or (_far_cells(case, ref["cells"], p["level"]) > 0).any(), (what, ref["report"])
        assert p["level"] == 5 or _far_cells(case, ref["frame"], p["level"])[..., 1].any(), what
    if not any(p["level"] == 3 for p in _cut_settings(case, r)):            # stage 1 alone at level 3: at level 5 no far probe pixel of these small frames is covered
        import torch
        p = sc.params(level=3, depth=8)
        gw, gh = sc.grid_of(r.cw, r.ch, p["level"])
        frame, omega, gray = _cut_records(case, r, p)
        d_cand = torch.full(((gh * gw + 2) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.SeamCandidatesDev(d[1], d[2], d[3], d[4], h9s, d_cand.data_ptr(), gw, gh, **p)
        rec = d_cand.cpu().numpy()
        assert (rec[gh * gw * 32:] == 0xAB).all() and np.array_equal(rec[:gh * gw * 32].reshape(gh, gw, 32), sc.record_bytes(frame, omega, gray)), case.tag
    level = 5
    p = scp.edge_params(level)
    gw, gh = sc.grid_of(r.cw, r.ch, level)
    given = scp.random_cells(len(case.render.imgs), gw, gh, 77)
    far = [k + 1 for k in case.far]
    if case.axis == 0:
        given[65536 >> level:] = np.where(given[65536 >> level:] % 2, far[0], far[1])          # the far cells name the far frames: they are followed there
    else:
        given[:, 65536 >> level:] = np.where(given[:, 65536 >> level:] % 2, far[0], far[1])
    want = sc.render(r.maps, r.weights(p["ramp"]), given, level)
    assert not np.array_equal(want[1], r.seamline(p["ramp"])[1]), case.tag
    dc = Cells(gw, gh, given)
    CutOut(d, h9s).render(ctx, d, h9s, p, dc.ptr()).check(want, f"{case.tag} under a random cell map")
    if case.axis == 0:
        row0, rows = _far_stripe(case, r)
        CutOut(d, h9s).render(ctx, d, h9s, p, dc.ptr(), row0=row0, rows=rows).check(want, f"{case.tag} under a random cell map, rows {row0}..", rows=(row0, rows))
        part = want[1][row0:]
        owners = (np.unique(part[part > 0]).astype(int) - 1).tolist()
        assert owners and np.flatnonzero(ctx.SeamCutCover(d[2], d[3], h9s, dc.ptr(), row0, rows, **p)).tolist() == owners, case.tag


# ---- statistics -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ep.GAIN_STEPS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_gain_stats_equal_restatement(ctx, oracle, case, step):
    r, d = _R(oracle, case), _D(case)
    pairs = ep.pairs_of(case, r, reverse=step == 3)
    st, cover = ctx.GainStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, pairs, step)
    recs, cov_ref = gr.stats_ref(r.maps, pairs, step)
    check_records(st, cover, recs, cov_ref, pairs, f"{case.tag} step {step}")
    assert cov_ref.any() and (step == 64 or any(n > 0 for n, _, _ in recs)), case.tag


@pytest.mark.parametrize("grid,step", [((4, 3), 3), ((16, 16), 1)])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_block_gain_stats_equal_restatement(ctx, oracle, case, grid, step):
    """grids 4 x 3 and 16 x 16, cut down to the smallest frame that takes part (a finer grid is refused)"""
    from tests.test_gpu_block_gain import _identities, _same_records
    r, d = _R(oracle, case), _D(case)
    pairs = ep.pairs_of(case, r)
    gx, gy = rp.fitted_grid(case.render, r, *grid)
    st, cover = ctx.BlockGainStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, pairs, step, gx, gy)
    ref, cov_ref = br.stats_ref(r.stats_maps, r.coords, r.sizes, pairs, step, gx, gy)
    assert np.array_equal(cover, cov_ref) and len(ref) > 0, (case.tag, grid)
    _same_records(st, ref)
    _identities(ctx, st, cover, d[1], d[2], d[3], d[4], case.render.h9s, pairs, step)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_sharp_stats_equal_restatement(ctx, oracle, case):
    """with and without per-frame tiles, at steps 1 and 3"""
    from tests.test_gpu_sharp import _same
    r, d = _R(oracle, case), _D(case)
    pairs = ep.pairs_of(case, r)
    lm = shr.lap_maps(r.maps)
    for step in (1, 3):
        want = shr.stats_ref(lm, pairs, step)
        st, fs = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, pairs, step)
        _same(st, fs, want[0], want[1], f"{case.tag} step {step}")
        st2, none = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, pairs, step, frames=False)
        assert none is None and st2.tobytes() == st.tobytes(), case.tag
        assert step != 1 or int(want[0]["n"][pairs.index(case.far)]) > 0, case.tag


# ---- chips, blend, blend along optimised seams ---------------------------------------------------------------------------------------------------------
def _same_chips(got, ref, what):
    assert (got["cw"], got["ch"], len(got["chips"])) == (ref["cw"], ref["ch"], len(ref["chips"])), what
    for k in range(len(ref["chips"])):
        for f in ("x0", "y0", "w", "h", "img"):
            assert int(got["chips"][k][f]) == int(ref["chips"][k][f]), (what, k, f)
        assert np.array_equal(got["chips"][k]["quad"].view(np.uint32), ref["chips"][k]["quad"].view(np.uint32)), (what, k)
        assert np.array_equal(got["chip_imgs"][k], ref["chip_imgs"][k]), f"{what}: chip {k} pixels"
        assert np.array_equal(got["masks"][k], ref["masks"][k]), f"{what}: chip {k} mask"


@pytest.mark.parametrize("case", BLEND + TALLEST, ids=_ids(BLEND + TALLEST))
def test_gpu_chips_and_blend_equal_oracle(ctx, oracle, case):
    """chips (x0 or y0 above 65 535), validity and ownership masks; the multiband blend in one call, from device frames, and -- on the tall
    canvases, where blend.hip's launches run one workgroup row per canvas row and owner_kernel one per 16 -- the far stripe to the last row"""
    imgs, h9s = case.render.imgs, case.render.h9s
    ref = oracle.chips_and_masks(imgs, h9s, find_masks=True)
    assert max(int(c["x0"]) for c in ref["chips"]) > 65535 or max(int(c["y0"]) for c in ref["chips"]) > 65535
    assert sum(int((m[:, :int(c["w"])] != 0).any()) for m, c in zip(ref["masks"], ref["chips"])) >= 3, case.tag
    _same_chips(ctx.ChipsAndMasks(imgs, h9s, find_masks=True), ref, case.tag)
    valid = ctx.ChipsAndMasks(imgs, h9s, find_masks=False)
    assert all(np.array_equal(a, b) for a, b in zip(valid["masks"], ref["valid"])), case.tag
    want, _ = oracle.multiband_blend(ref["chips"], ref["chip_imgs"], ref["masks"], ref["cw"], ref["ch"], band=BAND)
    got, ow, oh, _ = ctx.MosaicBlended(imgs, h9s, band=BAND)
    far = (slice(65536, None), slice(None)) if case.axis == 0 else (slice(None), slice(3 * 65536, None))
    assert want[far].any(), case.tag
    assert (ow, oh) == (ref["cw"], ref["ch"]) and got.shape == want.shape, case.tag
    bad = got != want
    assert not bad.any(), f"{case.tag} blended: {int(bad.sum())} bytes differ, first {np.argwhere(bad)[:5].tolist()}"
    d = _D(case)
    dev, cw, ch, cws = ctx.MosaicBlendedDev(d[1], d[2], d[3], d[4], h9s, band=BAND)
    assert np.array_equal(dev.cpu().numpy(), want), case.tag
    if case.axis == 0:
        row0 = 65535 * 16 if ch > 65535 * 16 else (65535 * 4 + 1 if ch > 65535 * 4 else 65536 + 7)
        part, _, _, _ = ctx.MosaicBlendedDev(d[1], d[2], d[3], d[4], h9s, band=BAND, row0=row0, rows=ch - row0)
        assert np.array_equal(part.cpu().numpy(), want[row0:]), f"{case.tag} blended rows {row0}.."


@pytest.mark.parametrize("case", BLEND, ids=_ids(BLEND))
def test_gpu_blend_seam_equals_restatement(ctx, oracle, case):
    """the cell map on the blend's grid and the canvas blended along it, against blend_seam_ref"""
    import torch
    import imagemosaicing_amd as im
    from tests import blend_seam_ref as bs
    imgs, h9s = case.render.imgs, case.render.h9s
    p = sc.params(level=3, depth=4)
    ref = bs.blend_seam_ref(oracle, imgs, h9s, p, band=BAND)
    d = _D(case)
    gw, gh = im.blend_seam_grid(d[2], d[3], h9s, p["level"])
    assert ref["cells"].shape == (gh, gw), case.tag
    cells = torch.full((gh * gw + 64,), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rep = ctx.BlendSeamCellsDev(d[1], d[2], d[3], d[4], h9s, cells.data_ptr(), gw, gh, **p)
    got = cells.cpu().numpy().view(np.uint16)
    assert (got[gh * gw:] == 0x7777).all() and np.array_equal(got[:gh * gw].reshape(gh, gw), ref["cells"]) and rep == ref["report"], (case.tag, rep, ref["report"])
    canvas, cw, ch, cws = ctx.MosaicBlendedSeam(imgs, h9s, band=BAND, **p)
    bad = canvas != ref["canvas"]
    assert not bad.any(), f"{case.tag} blended along seams: {int(bad.sum())} bytes differ, first {np.argwhere(bad)[:5].tolist()}"


# ---- overviews and the preview ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BLEND, ids=_ids(BLEND))
def test_gpu_overview_levels_and_preview_equal_restatement(ctx, oracle, case):
    """levels 1 .. 7 of the seamline canvas with its count map, in the three no-data modes, whole and -- on the tall canvases -- from stripes
    cut at 65 536 + 128; the level-3 seamline preview.  (csrc/overview.hip changes its launch where rows / 128 passes 65 535: a canvas of 8.4
    million rows, out of scope here.)"""
    import torch
    from tests.test_gpu_overview import Levels, _run, _same
    r, d = _R(oracle, case), _D(case)
    h9s = case.render.h9s
    o = Out(r, ("canvas", "count"))
    ctx.MosaicSeamlineDev(d[1], d[2], d[3], d[4], h9s, o.ptr("canvas"), o.cw, o.ch, o.cws, d_count=o.ptr("count"), ramp=0)
    ctx.synchronize()
    canvas_t, count_t = o.t["canvas"][:r.ch], o.t["count"][:r.ch * r.cw].reshape(r.ch, r.cw)
    pix, cnt = r.seamline(0)[0], r.seamline(0)[2]
    for nodata in (0, 1, 2):
        ref = ovr.overview_ref(pix, r.cw, 7, nodata, cnt)
        _same(_run(ctx, torch, canvas_t, r.cw, 7, nodata, count_t).host(), ref, f"{case.tag} nodata {nodata}")
        if case.axis == 0 and nodata == 2:
            out = Levels(torch, r.cw, r.ch, 7)
            cut = 65536 + 128
            _run(ctx, torch, canvas_t, r.cw, 7, nodata, count_t, row0=0, rows=cut, out=out)
            _run(ctx, torch, canvas_t, r.cw, 7, nodata, count_t, row0=cut, rows=r.ch - cut, out=out)
            _same(out.host(), ref, f"{case.tag} nodata {nodata} in two stripes")
    level = 3
    ow, oh, ows = ovr.layout(r.cw, r.ch, level)[-1]
    for nodata in (0, 2):
        ref, rcov = ovr.overview_ref(pix, r.cw, level, nodata, cnt)[level - 1]
        out, gw, gh, cover = ctx.MosaicPreviewInto(case.render.imgs, None, h9s, want_cover=True, render=2, ramp=0, level=level, nodata=nodata)
        assert (gw, gh) == (ow, oh) and np.array_equal(out[:, :3 * ow], ref[:, :3 * ow]) and np.array_equal(cover, rcov), (case.tag, nodata)


# ---- single warps -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,h9", [("shift", 3, 262200, ep.wp.shift(0.5, 0.25)), ("turn90", 262200, 3, ep.wp.turn(90))])
def test_gpu_warp_taller_than_four_times_65535_rows_equals_oracle(ctx, oracle, name, w, h, h9):
    """mi355_warp_image's launch holds 4 result rows per workgroup row: a 3 x 262 200 source under a shift and a 262 200 x 3 source under a
    quarter turn both give a result 262 200 rows high"""
    img = ep.wp.noise(w, h, 21)
    rc, ref = oracle.image_projection_transform(img, h9)
    assert rc == 0 and ref[2] > 65535 * 4 and ref[0][65535 * 4:].any(), (name, ref[1:])
    buf, dw, dh, dws = ctx.ImageProjectionTransform(img, h9)
    assert (dw, dh, dws) == ref[1:], name
    bad = buf != ref[0]
    assert not bad.any(), f"{name}: {int(bad.sum())} bytes differ, rows {np.argwhere(bad)[:, 0].min()}..{np.argwhere(bad)[:, 0].max()}"


# ---- frame passes on frames 65 537 and 2^20 long ------------------------------------------------------------------------------------------------------
FRAMES = [(w, h, pad) for w, h in ep.FRAME_SIZES for pad in ep.FRAME_PADS]
FRAME_IDS = ["%dx%d+%d" % f for f in FRAMES]
SRC_PAD, DST_FILL = 0xEE, 0x99


def _through(call, img, pad, want, what):
    """one frame through a pass, out of place and in place, on the pitch 3 w + pad with a guard row behind each buffer: the destination holds
    `want`, its padding and guard row and the source are as they were; returns what the two calls returned"""
    import torch
    h, w = img.shape[:2]
    buf, pitch = ep.padded(img, pad)
    buf = np.concatenate([buf, np.full((1, pitch), SRC_PAD, np.uint8)])
    rets = []
    for in_place in (False, True):
        src = torch.from_numpy(buf).cuda()
        dst = src if in_place else torch.full_like(src, DST_FILL)
        torch.cuda.synchronize()
        rets.append(call([src.data_ptr()], [dst.data_ptr()], [w], [h], [pitch]))
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        pix = got[:h, :3 * w].reshape(h, w, 3)
        bad = (pix != want).any(axis=2)
        if bad.any():
            ys, xs = np.nonzero(bad)
            raise AssertionError(f"{what}{' in place' if in_place else ''}: {int(bad.sum())} pixels differ, columns {xs.min()}..{xs.max()}, rows {ys.min()}..{ys.max()}")
        fill = SRC_PAD if in_place else DST_FILL
        assert (got[:h, 3 * w:] == fill).all() and (got[h] == fill).all(), f"{what}: padding or guard row written"
        assert in_place or np.array_equal(src.cpu().numpy(), buf), f"{what}: source changed"
    return rets


def _long_camera(w, h):
    """a barrel camera that moves the ends of the long side by a few pixels (tests/undistort_ref.cameras_for would push most of a 2-pixel-wide
    frame outside)"""
    from tests import undistort_ref as ur
    L = max(w, h)
    return ur.camera(0.8 * L, 0.8 * L, (w - 1) / 2.0 + 0.3, (h - 1) / 2.0 - 0.2, -6e-5 * (1 << 20) / L, 0.0, 1e-7, -2e-7)


@pytest.mark.parametrize("w,h,pad", FRAMES, ids=FRAME_IDS)
def test_gpu_undistort_long_frames(ctx, w, h, pad):
    import imagemosaicing_amd as im
    from tests import undistort_ref as ur
    img, cam = ep.frame(w, h, 31), _long_camera(w, h)
    want, n_out = ur.undistort(img, cam, None, 200)
    assert (want != img).any(axis=2).mean() > 0.5 and n_out < w * h // 2, (n_out, w * h)
    a, b = _through(lambda sp, dp, ww, hh, ws: ctx.UndistortFramesDev(sp, dp, ww, hh, ws, ws, im.Camera(**cam), fill=200), img, pad, want, f"undistort {w}x{h}")
    assert int(a[0]) == int(b[0]) == n_out


@pytest.mark.parametrize("w,h,pad", FRAMES, ids=FRAME_IDS)
def test_gpu_local_warps_long_frames(ctx, w, h, pad):
    """a 16-cell grid along the long side with shifts of up to 3 pixels along it and 0.4 across"""
    from tests import local_warp_ref as lr
    img = ep.frame(w, h, 32)
    gx, gy = (16, 1) if w > h else (1, 16)
    g = np.random.default_rng(33).uniform(-1, 1, (gy + 1, gx + 1, 2)).astype(np.float32) * np.array([3.0, 0.4] if w > h else [0.4, 3.0], np.float32)
    want, n = lr.apply(img, g)
    assert (want != img).any(axis=2).mean() > 0.5
    a, b = _through(lambda sp, dp, ww, hh, ws: ctx.ApplyLocalWarpsDev(sp, dp, ww, hh, ws, ws, g[None]), img, pad, want, f"local warp {w}x{h}")
    assert int(a[0]) == int(b[0]) == n


@pytest.mark.parametrize("w,h,pad", FRAMES, ids=FRAME_IDS)
def test_gpu_gains_long_frames(ctx, w, h, pad):
    """the per-frame LUT and a 16-cell gain map along the long side"""
    img = ep.frame(w, h, 34)
    g = np.array([[1.1, 0.9, 1.3]], np.float32)
    _through(lambda sp, dp, ww, hh, ws: ctx.ApplyGainsDev(sp, dp, ww, hh, ws, g), img, pad, gr.apply_lut(img, g[0]), f"gains {w}x{h}")
    gx, gy = (16, min(h, 2)) if w > h else (min(w, 2), 16)
    bg = np.random.default_rng(35).uniform(0.5, 1.7, (1, gy, gx, 3)).astype(np.float32)
    _through(lambda sp, dp, ww, hh, ws: ctx.ApplyBlockGainsDev(sp, dp, ww, hh, ws, bg), img, pad, br.apply_ref(img, bg[0]), f"block gains {w}x{h}")


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------------------
LONG = 1 << 20


def _smooth_noise(w, h, seed):
    """seeded noise under a 3 x 3 box: unlike in every block, smooth enough for a correlation peak to have neighbours"""
    a = np.random.default_rng(seed).integers(0, 256, (h + 2, w + 2, 3), dtype=np.uint8).astype(np.uint16)
    a = a[:-2] + a[1:-1] + a[2:]
    a = a[:, :-2] + a[:, 1:-1] + a[:, 2:]
    return np.ascontiguousarray((a // 9).astype(np.uint8))


def test_gpu_refine_ties_on_frames_2_20_long(ctx):
    """frame j 24 x 2^20, frame i 2^20 x 24: frame j under a quarter turn.  Ties around row 65 536 of frame j and around column 65 536 of
    frame i, and a sixteenth of a pixel apart (the float's step there) across the last rows of frame j and the last columns of frame i, so
    that the step from REFINED to EDGE falls between two neighbouring floats; radius 3, search 2"""
    import torch
    from tests import tie_refine_cases as tc
    from tests import tie_refine_ref as tr
    from tests.test_gpu_tie_refine import check
    fj = _smooth_noise(24, LONG, 41)
    fi = np.ascontiguousarray(fj.transpose(1, 0, 2)[:, ::-1])               # (x, y) of frame j at (LONG - 1 - y, x) of frame i
    H = np.array([0, -1, LONG - 1, 1, 0, 0, 0, 0, 1], np.float64)
    rng = np.random.default_rng(42)
    ramp = np.arange(3.0, 9.0, 0.0625)
    ys = np.concatenate([65536 + rng.uniform(-1.5, 1.5, 24), LONG - 1 - 65536 + rng.uniform(-1.5, 1.5, 24), LONG - 1 - ramp, ramp, rng.uniform(100, LONG - 100, 40)])
    b = np.stack([rng.uniform(7, 16, len(ys)), ys], 1).astype(np.float32).astype(np.float64)
    ax, ay = tc.project(H.reshape(3, 3), b[:, 0], b[:, 1])
    a = np.stack([ax, ay], 1) + rng.normal(0, 0.3, b.shape)
    assert len(b) == 280 and np.float32(LONG - 4) + np.float32(0.0625) != np.float32(LONG - 4)
    want = check(ctx, torch, tc.records(tc.record(0, 1, a, b, H)), [fi, fj], radius=3, search=2)
    status = want[1][0, :len(b)]
    for part in (slice(0, 24), slice(24, 48), slice(240, 280)):
        assert (status[part] == tr.REFINED).sum() > len(status[part]) // 2, status[part].tolist()
    for part in (slice(48, 144), slice(144, 240)):                          # both statuses along each ramp
        assert {tr.REFINED, tr.EDGE} <= set(status[part].tolist()), status[part].tolist()


def test_gpu_tie_residual_stats_on_frames_2_20_wide(ctx):
    """two frames 2^20 wide, a 16 x 2 grid: ties in the last grid cell (columns from 983 040 on) and around column 65 536"""
    import torch
    import imagemosaicing_amd as im
    from tests import local_warp_cases as lc
    from tests import local_warp_ref as lr
    from tests.test_gpu_local_warp import stats_dev
    w, h = [LONG, LONG], [24, 24]
    h9s = np.stack([ep.wp.shift(0, 0), ep.wp.shift(12.5, 3.25)])
    rng = np.random.default_rng(43)
    bx = np.concatenate([rng.uniform(LONG - 65536, LONG - 14, 150), 65536 + rng.uniform(-30, 30, 100), rng.uniform(0, LONG - 14, 100)])
    b = np.stack([bx, rng.uniform(0, 19, len(bx))], 1)
    a = b + np.array([12.5, 3.25]) + rng.normal(0, 0.6, b.shape)
    rec = lc.records([(0, 1, a.astype(np.float32), b.astype(np.float32))])
    p = dict(grid_x=16, grid_y=2)
    want = lr.stats(rec, w, h, h9s, **p)
    sd, NN = lr.stride(16, 2), 17 * 3
    nodes = want[:-8].reshape(2, sd)[:, :7 * NN].reshape(2, 7, NN)
    assert nodes[:, 0].reshape(2, 3, 17)[:, :, 15:].all() and int(want[-8]) == 0, "the last cell's nodes hold no tie"
    got = stats_dev((torch, im, ctx), rec, w, h, h9s, **p)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert np.array_equal(got, im.tie_residual_stats_host(rec, w, h, h9s, **p))


# ---- features ---------------------------------------------------------------------------------------------------------------------------------------------
def _keepall_ctx():
    import imagemosaicing_amd as im
    p = im.default_params()
    p.nfeatures = 0
    return im.Context(0, p)


@pytest.mark.parametrize("w,h", [(70000, 16), (16, 70000)])
def test_gpu_sift_70000_long_equals_oracle(ctx, oracle, w, h):
    """nfeatures = 2000: more than a hundred keypoints lie past coordinate 65 536.  Keep-all frames are at most 16384 x 16384
    (include/mi355_mosaic.h): at this size the keep-all mode refuses, naming the limit, and goes on working -- its comparison with the oracle
    is test_gpu_sift_keepall_16384_long_equals_oracle's, at that limit"""
    import imagemosaicing_amd as im
    from tests.synth_frames import terrain
    from tests.test_gpu_sift import _check
    from tests.test_gpu_sift_edges import _check_keepall
    img = terrain(w, h, seed=3)
    kp, _ = _check(ctx, oracle, img, f"terrain {w}x{h}")
    assert int((kp["x" if w > h else "y"] > 65536).sum()) > 100 and len(kp) == 2000
    c = _keepall_ctx()
    try:
        with pytest.raises(im.Mi355Error) as e:
            c.SiftExtract(8, img, max_kp=32768)
        assert e.value.code == -1 and "keep-all frames are at most 16384 x 16384" in str(e.value), str(e.value)
        small = img[:, :4000] if w > h else img[:4000]
        _check_keepall(c, oracle, np.ascontiguousarray(small), f"terrain {w}x{h} cut to 4000 after the refusal")
    finally:
        c.close()


@pytest.mark.parametrize("w,h", [(16384, 16), (16, 16384)])
def test_gpu_sift_keepall_16384_long_equals_oracle(oracle, w, h):
    from tests.synth_frames import terrain
    from tests.test_gpu_sift_edges import _check_keepall
    img = terrain(w, h, seed=5)
    assert len(oracle.sift(img, 0, 32768)[0]) > 300
    c = _keepall_ctx()
    try:
        _check_keepall(c, oracle, img, f"terrain {w}x{h}")
    finally:
        c.close()


@pytest.mark.parametrize("w,h", [(16383, 16), (16, 16383), (16383, 48), (48, 16383)])
def test_gpu_surf_16383_long_equals_oracle(ctx, oracle, w, h):
    """SURF's largest side.  A frame 16 pixels across is SURF's smallest too and holds no maximum: the 48-pixel ones hold keypoints along
    the whole length"""
    from tests import surf_patterns as su
    from tests.synth_frames import terrain
    from tests.test_gpu_surf_edges import _same
    img = terrain(w, h, seed=6)
    want = oracle.surf(img, su.THR_SHAPE, su.KEEP_ALL)
    if min(w, h) > 16:
        assert len(want[0]) > 100 and float(want[0]["x" if w > h else "y"].max()) > 16300, len(want[0])
    _same(ctx.SurfExtract(7, img, su.THR_SHAPE, su.KEEP_ALL), want, f"terrain {w}x{h}")

"""The blended one-pass renders and the gain statistics at the warp stage's edges, on the GPU: feather_tile_kernel, seamline_tile_kernel,
median_tile_kernel<K, SAMPLE> (csrc/feather.hip, seamline.hip, median.hip), the gain and block-gain statistics (csrc/gain.hip) and the striped
preview (csrc/overview.hip, frames.hip) against the numpy restatements (tests/feather_ref.py, seamline_ref.py, median_ref.py, gain_ref.py,
block_gain_ref.py, overview_ref.py) on the cases of tests/render_patterns.py -- quarter turns, mirrors, m8 = 2, -1 and 0, a frame without
an inverse, 40 frames on one tile, canvas widths 1 .. 257, canvas heights 1 .. 257, overlap across a list-block corner.  Every comparison
is np.array_equal on output bytes or integer sums; there are no tolerances and nothing is filtered at run time.  Output buffers are
pre-filled with a sentinel and carry a guard (a canvas row, 64 map entries) beyond their end that must stay as it was.
(tests/test_render_patterns_oracle.py checks the cases and the restatements themselves, without a GPU.)
"""
import numpy as np
import pytest

from tests import block_gain_ref as br
from tests import gain_ref as gr
from tests import overview_ref as ovr
from tests import render_patterns as rp

pytestmark = pytest.mark.gpu

CASES = rp.cases()
IDS = [c.tag for c in CASES]
TAGS = {c.tag: c for c in CASES}
NEW = [c for c in CASES if c.new]
SENT8, SENT16, SENT_SPREAD = 0xA5, 0x5555, 0x33
GUARD = 64                                                                  # map entries beyond ch * cw
FILL = {"canvas": SENT8, "owner": SENT16, "count": SENT16, "spread": SENT_SPREAD}
MEDIAN_DEPTHS = rp.DEPTHS + (0,)
COVER_TAGS = ("twins", "hidden", "forty", "rank_deficient", "m8_zero_ends")
HOST_TAGS = ("twins", "turns", "canvas_w1", "canvas_h1", "straddle_overlap")
PREVIEW = {1: ("canvas_w1", "canvas_w2", "canvas_w3", "canvas_h1", "canvas_h2", "straddle_overlap"),
           3: ("canvas_w7", "canvas_w8", "canvas_h7", "canvas_h8", "canvas_h9", "straddle_overlap")}


def _pick(tags):
    return [TAGS[t] for t in tags]


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


# ---- comparison helpers: numpy only (a CPU script can hand them a wrong expectation and see them object) ---------------------------------
def _rows(ch, rows):
    return (0, ch) if rows is None else rows


def check_canvas(got, ref, cw, ch, what, rows=None):
    """got [ch + 1, cws] (the last row is the guard), ref [ch, cw, 3]: the rows [row0, row0 + n) hold ref's bytes and zeroed padding
    [3 cw, cws), every other row and the guard row the sentinel"""
    row0, n = _rows(ch, rows)
    assert got.shape[0] == ch + 1 and got.shape[1] >= 3 * cw and ref.shape == (ch, cw, 3), f"{what}: shapes {got.shape} {ref.shape}"
    inside = got[row0:row0 + n]
    pix = np.ascontiguousarray(inside[:, :3 * cw]).reshape(n, cw, 3)
    bad = (pix != ref[row0:row0 + n]).any(axis=2)
    if bad.any():
        y, x = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what} canvas: {int(bad.sum())} pixels differ, first at x {x} y {y + row0}: got {pix[y, x].tolist()}, expected "
                             f"{ref[y + row0, x].tolist()}; rows {int(np.argwhere(bad)[:, 0].min()) + row0}..{int(np.argwhere(bad)[:, 0].max()) + row0}, "
                             f"columns {int(np.argwhere(bad)[:, 1].min())}..{int(np.argwhere(bad)[:, 1].max())}")
    assert not inside[:, 3 * cw:].any(), f"{what} canvas: row padding [3 cw, cws) not cleared"
    assert (got[:row0] == SENT8).all() and (got[row0 + n:ch] == SENT8).all(), f"{what} canvas: rows outside {row0}..{row0 + n - 1} were written"
    assert (got[ch] == SENT8).all(), f"{what} canvas: the guard row after the canvas was written"


def check_map(got, ref, cw, ch, fill, what, rows=None):
    """got: flat [ch * cw + GUARD], ref [ch, cw]: the rows of the call hold ref, every other entry and the guard the fill"""
    row0, n = _rows(ch, rows)
    assert got.shape == (ch * cw + GUARD,) and ref.shape == (ch, cw), f"{what}: shapes {got.shape} {ref.shape}"
    body = got[:ch * cw].reshape(ch, cw)
    bad = body[row0:row0 + n] != ref[row0:row0 + n]
    if bad.any():
        y, x = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} entries differ, first at x {x} y {y + row0}: got {int(body[y + row0, x])}, expected "
                             f"{int(ref[y + row0, x])}; columns {int(np.argwhere(bad)[:, 1].min())}..{int(np.argwhere(bad)[:, 1].max())}")
    assert (body[:row0] == fill).all() and (body[row0 + n:] == fill).all(), f"{what}: rows outside {row0}..{row0 + n - 1} were written"
    assert (got[ch * cw:] == fill).all(), f"{what}: entries beyond ch * cw were written"


def check_records(st, cover, recs, cov_ref, pairs, what):
    """GainStatsDev's answer against gain_ref.stats_ref's"""
    assert np.array_equal(cover, cov_ref), f"{what}: cover {cover.tolist()} != {cov_ref.tolist()}"
    assert len(st) == len(pairs) == len(recs)
    for i, ((a, b), (nn, sa, sb)) in enumerate(zip(pairs, recs)):
        assert (int(st[i]["a"]), int(st[i]["b"])) == (a, b), (what, i)
        assert int(st[i]["n"]) == nn and np.array_equal(st[i]["sum_a"], sa) and np.array_equal(st[i]["sum_b"], sb), \
            f"{what}: pair {i} ({a}, {b}): got n {int(st[i]['n'])} sums {st[i]['sum_a'].tolist()} {st[i]['sum_b'].tolist()}, expected n {nn} sums {sa.tolist()} {sb.tolist()}"


# ---- device frames and output buffers --------------------------------------------------------------------------------------------------------
_DEV = {}


def _frames(case):
    """the case's frames on the device, uploaded once: (tensors, ptrs, w, h, ws)"""
    if case.tag not in _DEV:
        import torch
        ts = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in case.imgs]
        torch.cuda.synchronize()
        _DEV[case.tag] = (ts, [t.data_ptr() for t in ts], [a.shape[1] for a in case.imgs], [a.shape[0] for a in case.imgs], [3 * a.shape[1] for a in case.imgs])
    return _DEV[case.tag]


def _only(ptrs, keep):
    return [p if k in keep else 0 for k, p in enumerate(ptrs)]


class Out:
    """sentinel-filled device outputs of a cw x ch canvas: "canvas" [ch + 1, cws] uint8, "owner" / "count" [ch * cw + GUARD] uint16 (int16
    storage), "spread" [ch * cw + GUARD] uint8"""
    def __init__(self, r, kinds, cws=None):
        import torch
        import imagemosaicing_amd as im
        self.cw, self.ch, self.cws = r.cw, r.ch, cws or r.cws
        c = r.case
        assert tuple(im.mosaic_layout([a.shape[1] for a in c.imgs], [a.shape[0] for a in c.imgs], c.h9s)[:3]) == (r.cw, r.ch, r.cws), c.tag
        self.t = {}
        for k in kinds:
            if k == "canvas":
                self.t[k] = torch.full((self.ch + 1, self.cws), SENT8, dtype=torch.uint8, device="cuda")
            elif k == "spread":
                self.t[k] = torch.full((self.ch * self.cw + GUARD,), SENT_SPREAD, dtype=torch.uint8, device="cuda")
            else:
                self.t[k] = torch.full((self.ch * self.cw + GUARD,), SENT16, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()                                            # the fills run on torch's stream, the library on the ctx's own

    def ptr(self, k):
        return self.t[k].data_ptr() if k in self.t else 0

    def host(self, k):
        a = self.t[k].cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a

    def untouched(self):
        return all((self.host(k) == FILL[k]).all() for k in self.t)

    def check(self, ref, what, rows=None):
        """ref: {kind: expected array}"""
        for k in self.t:
            if k == "canvas":
                check_canvas(self.host(k), ref[k], self.cw, self.ch, what, rows)
            else:
                check_map(self.host(k), ref[k], self.cw, self.ch, FILL[k], f"{what} {k}", rows)


# the three renders behind one call: (kinds of output, the call, the restatement as {kind: array})
def _feather_call(ctx, d, case, o, ramp, depth, ptrs=None, row0=0, rows=-1):
    ctx.MosaicFeatheredDev(d[1] if ptrs is None else ptrs, d[2], d[3], d[4], case.h9s, o.ptr("canvas"), o.cw, o.ch, o.cws, row0, rows, ramp=ramp)


def _seamline_call(ctx, d, case, o, ramp, depth, ptrs=None, row0=0, rows=-1):
    ctx.MosaicSeamlineDev(d[1] if ptrs is None else ptrs, d[2], d[3], d[4], case.h9s, o.ptr("canvas"), o.cw, o.ch, o.cws, row0, rows,
                          d_owner=o.ptr("owner"), d_count=o.ptr("count"), ramp=ramp)


def _median_call(ctx, d, case, o, ramp, depth, ptrs=None, row0=0, rows=-1):
    ctx.MosaicMedianDev(d[1] if ptrs is None else ptrs, d[2], d[3], d[4], case.h9s, o.ptr("canvas"), o.cw, o.ch, o.cws, row0, rows,
                        d_spread=o.ptr("spread"), d_count=o.ptr("count"), ramp=ramp, depth=depth)


def _feather_ref(r, ramp, depth):
    return {"canvas": r.feather(ramp)[0]}


def _seamline_ref(r, ramp, depth):
    s = r.seamline(ramp)
    return {"canvas": s[0], "owner": s[1], "count": s[2]}


def _median_ref(r, ramp, depth):
    m = r.median(ramp, depth)
    return {"canvas": m[0], "spread": m[1], "count": m[2]}


RENDERS = {"feathered": (("canvas",), _feather_call, _feather_ref),
           "seamline": (("canvas", "owner", "count"), _seamline_call, _seamline_ref),
           "median": (("canvas", "spread", "count"), _median_call, _median_ref)}


# ---- the whole canvas -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ramp", rp.RAMPS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_feathered_equals_restatement(ctx, oracle, case, ramp):
    r = rp.restate(oracle, case)
    o = Out(r, ("canvas",))
    _feather_call(ctx, _frames(case), case, o, ramp, 0)
    o.check(_feather_ref(r, ramp, 0), f"{case.tag} feathered ramp {ramp}")
    wide = Out(r, ("canvas",), cws=r.cws + 12)                              # a caller's wider row: the padding is cleared up to cws
    _feather_call(ctx, _frames(case), case, wide, ramp, 0)
    wide.check(_feather_ref(r, ramp, 0), f"{case.tag} feathered ramp {ramp} row stride {wide.cws}")


@pytest.mark.parametrize("ramp", rp.RAMPS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_seamline_equals_restatement(ctx, oracle, case, ramp):
    r = rp.restate(oracle, case)
    kinds, call, ref = RENDERS["seamline"]
    o = Out(r, kinds)
    call(ctx, _frames(case), case, o, ramp, 0)
    o.check(ref(r, ramp, 0), f"{case.tag} seamline ramp {ramp}")
    wide = Out(r, kinds, cws=r.cws + 12)
    call(ctx, _frames(case), case, wide, ramp, 0)
    wide.check(ref(r, ramp, 0), f"{case.tag} seamline ramp {ramp} row stride {wide.cws}")


@pytest.mark.parametrize("depth", MEDIAN_DEPTHS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_median_equals_restatement(ctx, oracle, case, depth):
    r = rp.restate(oracle, case)
    kinds, call, ref = RENDERS["median"]
    for ramp in rp.RAMPS:
        o = Out(r, kinds)
        call(ctx, _frames(case), case, o, ramp, depth)
        o.check(ref(r, ramp, depth), f"{case.tag} median ramp {ramp} depth {depth}")
    wide = Out(r, kinds, cws=r.cws + 12)
    call(ctx, _frames(case), case, wide, 0, depth)
    wide.check(ref(r, 0, depth), f"{case.tag} median depth {depth} row stride {wide.cws}")


# ---- stripes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("render,depth", [("feathered", 0), ("seamline", 0), ("median", 1), ("median", 5)])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_stripes_equal_the_whole(ctx, oracle, case, render, depth):
    """stripes of 1 row and of 7 rows, side by side in one sentinel-filled set of outputs, are the whole canvas and its maps; one stripe call
    writes its own rows only.  median at depth 1 (two rows per lane) and 5 (one)."""
    r = rp.restate(oracle, case)
    kinds, call, ref = RENDERS[render]
    d, want = _frames(case), ref(r, 3, depth)
    for cut in (1, 7):
        o = Out(r, kinds)
        for row0 in range(0, r.ch, cut):
            call(ctx, d, case, o, 3, depth, row0=row0, rows=min(cut, r.ch - row0))
        o.check(want, f"{case.tag} {render} depth {depth} in stripes of {cut}")
    for row0, rows in {(r.ch // 3, max(1, r.ch // 2)), (r.ch - 1, 1), (0, 1)}:
        o = Out(r, kinds)
        call(ctx, d, case, o, 3, depth, row0=row0, rows=rows)
        o.check(want, f"{case.tag} {render} depth {depth} rows {row0}..{row0 + rows - 1}", rows=(row0, rows))


# ---- covers and withheld frames -----------------------------------------------------------------------------------------------------------------
def _refused(ctx, fn, k):
    import imagemosaicing_amd as im
    with pytest.raises(im.Mi355Error) as e:
        fn()
    assert e.value.code == -1 and "image %d " % k in str(e.value), str(e.value)


def _some(cover):
    return sorted({cover[0], cover[len(cover) // 2], cover[-1]})


@pytest.mark.parametrize("ramp", rp.RAMPS)
@pytest.mark.parametrize("case", _pick(COVER_TAGS), ids=COVER_TAGS)
def test_gpu_seamline_cover_and_withheld_frames(ctx, oracle, case, ramp):
    r = rp.restate(oracle, case)
    kinds, call, ref = RENDERS["seamline"]
    d, want = _frames(case), ref(r, ramp, 0)
    owners = (np.unique(want["owner"][want["owner"] > 0]).astype(int) - 1).tolist()
    need = ctx.SeamlineCover(d[2], d[3], case.h9s, ramp=ramp)
    assert np.flatnonzero(need).tolist() == owners, (case.tag, np.flatnonzero(need).tolist(), owners)
    assert not any(need[k] for k in rp.skipped(case, r))
    for row0, rows in ((0, 1), (r.ch // 3, max(1, r.ch // 2))):
        part = want["owner"][row0:row0 + rows]
        assert np.flatnonzero(ctx.SeamlineCover(d[2], d[3], case.h9s, row0, rows, ramp=ramp)).tolist() == (np.unique(part[part > 0]).astype(int) - 1).tolist()
    o = Out(r, kinds)
    call(ctx, d, case, o, ramp, 0, ptrs=_only(d[1], owners))
    o.check(want, f"{case.tag} seamline ramp {ramp}, every frame outside the cover withheld")
    for k in _some(owners):
        bad = Out(r, kinds)
        _refused(ctx, lambda: call(ctx, d, case, bad, ramp, 0, ptrs=_only(d[1], [q for q in owners if q != k])), k)
        assert bad.untouched(), f"{case.tag}: the refused call wrote something"
        o = Out(r, kinds)
        call(ctx, d, case, o, ramp, 0, ptrs=_only(d[1], owners))            # the ctx goes on working
        o.check(want, f"{case.tag} seamline ramp {ramp} after the refusal for frame {k}")


@pytest.mark.parametrize("depth", MEDIAN_DEPTHS)
@pytest.mark.parametrize("case", _pick(COVER_TAGS), ids=COVER_TAGS)
def test_gpu_median_cover_and_withheld_frames(ctx, oracle, case, depth):
    r = rp.restate(oracle, case)
    kinds, call, ref = RENDERS["median"]
    d, want = _frames(case), ref(r, 0, depth)
    sel = r.median(0, depth)[3]
    inside = (np.unique(sel[sel > 0]).astype(int) - 1).tolist()
    need = ctx.MedianCover(d[2], d[3], case.h9s, depth=depth)
    assert np.flatnonzero(need).tolist() == inside, (case.tag, depth, np.flatnonzero(need).tolist(), inside)
    assert not any(need[k] for k in rp.skipped(case, r))
    for row0, rows in ((0, 1), (r.ch // 3, max(1, r.ch // 2))):
        part = sel[:, row0:row0 + rows]
        assert np.flatnonzero(ctx.MedianCover(d[2], d[3], case.h9s, row0, rows, depth=depth)).tolist() == (np.unique(part[part > 0]).astype(int) - 1).tolist()
    o = Out(r, kinds)
    call(ctx, d, case, o, 0, depth, ptrs=_only(d[1], inside))
    o.check(want, f"{case.tag} median depth {depth}, every frame outside the cover withheld")
    for k in _some(inside):
        bad = Out(r, kinds)
        _refused(ctx, lambda: call(ctx, d, case, bad, 0, depth, ptrs=_only(d[1], [q for q in inside if q != k])), k)
        assert bad.untouched(), f"{case.tag}: the refused call wrote something"
        o = Out(r, kinds)
        call(ctx, d, case, o, 0, depth, ptrs=_only(d[1], inside))           # the ctx goes on working
        o.check(want, f"{case.tag} median depth {depth} after the refusal for frame {k}")


@pytest.mark.parametrize("case", _pick(COVER_TAGS), ids=COVER_TAGS)
def test_gpu_feathered_withheld_frames(ctx, oracle, case):
    """every frame whose box meets the rows is read: withholding one is MI355_ERR_ARG; the frames the render skips (m8 = 0, no inverse) may
    be withheld"""
    r = rp.restate(oracle, case)
    d, want = _frames(case), _feather_ref(r, 0, 0)
    sk = rp.skipped(case, r)
    live = [k for k in range(len(case.imgs)) if k not in sk]
    assert len(sk) == {"m8_zero_ends": 2, "rank_deficient": 1}.get(case.tag, 0)
    assert np.flatnonzero(ctx.StripeCover(d[2], d[3], case.h9s, 0, r.ch)).tolist() == live          # the box cover is this render's cover
    o = Out(r, ("canvas",))
    _feather_call(ctx, d, case, o, 0, 0, ptrs=_only(d[1], live))
    o.check(want, f"{case.tag} feathered, skipped frames withheld")
    for k in _some(live):
        bad = Out(r, ("canvas",))
        _refused(ctx, lambda: _feather_call(ctx, d, case, bad, 0, 0, ptrs=_only(d[1], [q for q in live if q != k])), k)
        assert bad.untouched(), f"{case.tag}: the refused call wrote something"
    o = Out(r, ("canvas",))
    _feather_call(ctx, d, case, o, 0, 0)                                    # the ctx goes on working
    o.check(want, f"{case.tag} feathered after the refusals")


# ---- gain statistics ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", (1, 3))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_gain_stats_equal_restatement(ctx, oracle, case, step):
    """all pairs i < j (the first 60 of the forty frames' 780); at step 3 one of them the other way round"""
    r = rp.restate(oracle, case)
    d = _frames(case)
    pairs = rp.gain_pairs(case, r, reverse=step == 3)
    st, cover = ctx.GainStatsDev(d[1], d[2], d[3], d[4], case.h9s, pairs, step)
    recs, cov_ref = gr.stats_ref(r.maps, pairs, step)
    check_records(st, cover, recs, cov_ref, pairs, f"{case.tag} step {step}")
    sk = rp.skipped(case, r)
    assert all(cover[k] == 0 for k in sk) and all(int(st[i]["n"]) == 0 for i, (a, b) in enumerate(pairs) if a in sk or b in sk)
    if min(r.cw, r.ch) == 1:                                                # the lattice is a single line
        assert int(cover.max()) <= (max(r.cw, r.ch) + step - 1) // step
    # the skipped frames' pointers may be withheld
    st2, cover2 = ctx.GainStatsDev(_only(d[1], [k for k in range(len(d[1])) if k not in sk]), d[2], d[3], d[4], case.h9s, pairs, step)
    assert st2.tobytes() == st.tobytes() and np.array_equal(cover2, cover)


@pytest.mark.parametrize("step", (1, 3))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_block_gain_stats_equal_restatement(ctx, oracle, case, step):
    """grids 1 x 1 and 4 x 3; where a frame that takes part is smaller than 4 x 3 the call is refused, naming it, and the grid cut down to
    the smallest frame is compared in its place"""
    import imagemosaicing_amd as im
    from tests.test_gpu_block_gain import _identities, _same_records
    r = rp.restate(oracle, case)
    d = _frames(case)
    pairs = rp.gain_pairs(case, r, reverse=step == 3)
    grids = [(1, 1), (4, 3)]
    fit = rp.fitted_grid(case, r, 4, 3)
    if fit != (4, 3):
        small = next(k for k, (s, c) in enumerate(zip(r.sizes, r.coords)) if c is not None and (s[0] < 4 or s[1] < 3))
        with pytest.raises(im.Mi355Error) as e:
            ctx.BlockGainStatsDev(d[1], d[2], d[3], d[4], case.h9s, pairs, step, 4, 3)
        assert e.value.code == -1 and "frame %d (%dx%d) is smaller than the 4x3 grid" % ((small,) + r.sizes[small]) in str(e.value), str(e.value)
        grids = [(1, 1)] + ([fit] if fit != (1, 1) else [])
    for gx, gy in grids:
        st, cover = ctx.BlockGainStatsDev(d[1], d[2], d[3], d[4], case.h9s, pairs, step, gx, gy)
        ref, cov_ref = br.stats_ref(r.stats_maps, r.coords, r.sizes, pairs, step, gx, gy)
        assert np.array_equal(cover, cov_ref), (case.tag, step, gx, gy)
        _same_records(st, ref)
        _identities(ctx, st, cover, d[1], d[2], d[3], d[4], case.h9s, pairs, step)
    if case.tag == "turns" and step == 1:
        # three quarter turns: along frame 0's columns (cell_a % 4 grows) frame 2's rows (cell_b // 4) change
        p = st[st["pair"] == pairs.index((0, 2))]
        assert (gx, gy) == (4, 3) and len(set((p["cell_a"] % 4).tolist())) > 1 and len(set((p["cell_b"] // 4).tolist())) > 1


# ---- the striped preview ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,tag", [(l, t) for l, ts in PREVIEW.items() for t in ts])
def test_gpu_preview_equals_the_restatement_of_the_full_render(ctx, oracle, level, tag):
    case = TAGS[tag]
    r = rp.restate(oracle, case)
    ramp = 0 if level == 1 else 3
    full = [np.ascontiguousarray(r.refined[:, :3 * r.cw]).reshape(r.ch, r.cw, 3), r.feather(ramp)[0], r.seamline(ramp)[0]]
    cnt = r.seamline(ramp)[2]
    ow, oh, ows = ovr.layout(r.cw, r.ch, level)[-1]
    pitch = 3 * ow + 5
    seen = {}
    for render in (0, 1, 2):
        for nodata in (0, 2):
            ref, rcov = ovr.overview_ref(full[render], r.cw, level, nodata, cnt)[level - 1]
            out = np.full((oh, pitch), 201, np.uint8)
            out, gw, gh, cover = ctx.MosaicPreviewInto(case.imgs, None, case.h9s, out=out, want_cover=True, render=render, ramp=ramp, level=level, nodata=nodata)
            assert (gw, gh) == (ow, oh)
            bad = out[:, :3 * ow] != ref[:, :3 * ow]
            assert not bad.any(), f"{tag} level {level} render {render} nodata {nodata}: {int(bad.sum())} bytes differ, first {np.argwhere(bad)[:5].tolist()}"
            assert np.all(out[:, 3 * ow:] == 201) and np.array_equal(cover, rcov), (tag, level, render, nodata)
            seen[(render, nodata)] = out[:, :3 * ow].copy()
    try:
        for stripe in (1 << level, 1):                                      # the stripe height does not show
            ctx.set_option("preview_stripe_rows", stripe)
            for (render, nodata), want in seen.items():
                out, _, _ = ctx.MosaicPreviewInto(case.imgs, None, case.h9s, render=render, ramp=ramp, level=level, nodata=nodata)
                assert np.array_equal(out[:, :3 * ow], want), (tag, level, stripe, render, nodata)
    finally:
        ctx.set_option("preview_stripe_rows", 1024)                         # the library's default


# ---- the refined render on the cases tests/test_gpu_warp_edges.py does not see ---------------------------------------------------------------
@pytest.mark.parametrize("case", NEW, ids=[c.tag for c in NEW])
def test_gpu_refined_equals_oracle_on_the_new_cases(ctx, oracle, case):
    r = rp.restate(oracle, case)
    d = _frames(case)
    got, cw, ch, cws = ctx.MosaicImagesRefined(case.imgs, case.h9s)
    assert (cw, ch, cws) == (r.cw, r.ch, r.cws) and np.array_equal(got, r.refined), f"{case.tag}: {int((got != r.refined).sum())} bytes differ"
    want = np.ascontiguousarray(r.refined[:, :3 * r.cw]).reshape(r.ch, r.cw, 3)

    def render(o, row0, rows):
        ctx.MosaicImagesRefinedDev(d[1], d[2], d[3], d[4], case.h9s, o.ptr("canvas"), o.cw, o.ch, o.cws, row0, rows)
        ctx.synchronize()

    for cws_ in (r.cws, r.cws + 12):
        o = Out(r, ("canvas",), cws=cws_)
        render(o, 0, r.ch)
        check_canvas(o.host("canvas"), want, r.cw, r.ch, f"{case.tag} refined row stride {cws_}")
    for cut in (1, 7):
        o = Out(r, ("canvas",))
        for row0 in range(0, r.ch, cut):
            render(o, row0, min(cut, r.ch - row0))
        check_canvas(o.host("canvas"), want, r.cw, r.ch, f"{case.tag} refined in stripes of {cut}")
    o = Out(r, ("canvas",))
    render(o, r.ch // 3, max(1, r.ch // 2))
    check_canvas(o.host("canvas"), want, r.cw, r.ch, f"{case.tag} refined, one stripe", rows=(r.ch // 3, max(1, r.ch // 2)))


# ---- host forms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _pick(HOST_TAGS), ids=HOST_TAGS)
def test_gpu_host_forms_give_the_device_forms_bytes(ctx, oracle, case):
    r = rp.restate(oracle, case)
    d = _frames(case)
    geo = (r.cw, r.ch, r.cws)
    for ramp in rp.RAMPS:
        o = Out(r, ("canvas",))
        _feather_call(ctx, d, case, o, ramp, 0)
        host, cw, ch, cws = ctx.MosaicFeathered(case.imgs, case.h9s, ramp=ramp)
        assert (cw, ch, cws) == geo and np.array_equal(host, o.host("canvas")[:r.ch]), (case.tag, "feathered", ramp)
        o = Out(r, RENDERS["seamline"][0])
        _seamline_call(ctx, d, case, o, ramp, 0)
        host, cw, ch, cws, own = ctx.MosaicSeamline(case.imgs, case.h9s, ramp=ramp, want_owner=True)
        assert (cw, ch, cws) == geo and np.array_equal(host, o.host("canvas")[:r.ch]), (case.tag, "seamline", ramp)
        assert np.array_equal(own, o.host("owner")[:r.ch * r.cw].reshape(r.ch, r.cw)), (case.tag, "seamline owner", ramp)
        assert np.array_equal(ctx.MosaicSeamline(case.imgs, case.h9s, ramp=ramp)[0], host)
        for depth in MEDIAN_DEPTHS:
            o = Out(r, RENDERS["median"][0])
            _median_call(ctx, d, case, o, ramp, depth)
            host, cw, ch, cws, spr = ctx.MosaicMedian(case.imgs, case.h9s, ramp=ramp, depth=depth, want_spread=True)
            assert (cw, ch, cws) == geo and np.array_equal(host, o.host("canvas")[:r.ch]), (case.tag, "median", ramp, depth)
            assert np.array_equal(spr, o.host("spread")[:r.ch * r.cw].reshape(r.ch, r.cw)), (case.tag, "median spread", ramp, depth)
            assert np.array_equal(ctx.MosaicMedian(case.imgs, case.h9s, ramp=ramp, depth=depth)[0], host)

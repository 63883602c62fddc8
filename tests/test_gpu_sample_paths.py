"""GPU: the 2 x 2 texel loads every frame-sampling kernel shares (csrc/mosaic_frame.h: load_quad3 -- one 8-byte load per source row where
8 bytes still lie inside the row's pitch, else 4 + 2 bytes -- and the byte-to-float conversions behind it), pinned where the wide / narrow
switch and the byte positions can go wrong, byte for byte against the references the project already has.

  * bytes: every frame is a function of position, (97 (3 x + c) + 57 y + 31 k + 255) mod 256: all 256 values occur, and 255 and values
    >= 128 stand in each of the six byte positions of a texel pair, so a wrong shift, a sign extension or a swapped half shows;
  * the switch: samples at xi = w - 2, w - 3 and w - 4, in the last row pair and elsewhere, on rows of the IplImage pitch (3 w rounded up
    to 4) and on padded rows (3 w + 4, 3 w + 8); from the geometry, both forms are taken (3 xi + 8 <= ws in the renders and statistics,
    xi + 3 <= w in undistortion and the local warp);
  * alignment: device frames at base pointers +0 .. +3 (tests/pitched.py), so that the 8-byte loads start at every residue mod 8;
  * coverage: identity-like and rotated transforms; the refined, feathered, seamline and median (depth 3) renders, the single-image warp,
    undistortion and the local warp, one gain-statistics and one sharpness-statistics call; frame widths 3, 4 and 5.

Frames are at most 64 x 48, the canvas 89 x 69.  Nothing is skipped or filtered at run time."""
import ctypes as C

import numpy as np
import pytest

from tests import gain_ref as gr
from tests import local_warp_ref as lr
from tests import oracle_lib as ol
from tests import pitched as pf
from tests import render_patterns as rp
from tests import sharp_ref as shr
from tests import undistort_ref as ur

pytestmark = pytest.mark.gpu

# the widest first, widths 5, 4 and 3 last: the refined render takes the highest covering frame, so the small frames are read
SIZES = [(64, 48), (48, 31), (37, 29), (35, 21), (26, 17), (5, 9), (4, 6), (3, 7)]
PADS = ("ipl", 4, 8)                                        # the three layouts: ws = (3 w + 3) & ~3, 3 w + 4, 3 w + 8
PAIRS = [(0, 1), (0, 2), (1, 2), (0, 3), (2, 3), (0, 4), (1, 4), (0, 5), (3, 5), (0, 6), (0, 7), (5, 7), (2, 4), (4, 6)]


def pattern(w, h, k):
    y, x, c = np.mgrid[0:h, 0:w, 0:3]
    return ((97 * (3 * x + c) + 57 * y + 31 * k + 255) & 0xff).astype(np.uint8)


def _turn(deg, s, tx, ty, px=0.0, py=0.0):
    a = np.deg2rad(deg)
    return np.array([s * np.cos(a), -s * np.sin(a), tx, s * np.sin(a), s * np.cos(a), ty, px, py, 1.0], np.float32)


def _h9s():
    return np.stack([_turn(0, 1, 0, 0), _turn(0, 1, 40.5, 20.25), _turn(23, 1.1, 34, 24), _turn(0, 1, 10.25, 30.5),
                     _turn(-40, 1.0, 44, 30, 2e-4, -1e-4), _turn(0, 1, 3.5, 2.25), _turn(17, 1.5, 20.3, 8.6), _turn(0, 1, 12.75, 11.5)])


def _pitches(pad):
    return [pf.ipl_pitch(w) if pad == "ipl" else 3 * w + pad for w, _ in SIZES]


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case():
    imgs = [pattern(w, h, k) for k, (w, h) in enumerate(SIZES)]
    return rp.Render("sample_paths", imgs, _h9s(), "the wide / narrow texel loads and their byte positions", lambda c, r: True, new=True)


@pytest.fixture(scope="module")
def rst(oracle, case):
    """the restatements of the case, made once and left as they are"""
    r = rp.restate(oracle, case)
    assert r.cw <= 256 and r.ch <= 256
    return r


@pytest.fixture(scope="module")
def layouts(case):
    """per layout the pitched frames on the device: (PitchedFrames, tensor, ptrs)"""
    import torch
    out = {}
    for i, pad in enumerate(PADS):
        fr = pf.PitchedFrames(case.imgs, _pitches(pad), offsets=[(k + i) % 4 for k in range(len(SIZES))], seed=60 + i)
        t, ptrs = fr.to_device(torch)
        assert t.data_ptr() % 256 == 0
        out[pad] = (fr, t, ptrs)
    yield out
    out.clear()


def _samples(r, mask_of):
    """per frame (xi, yi) of the canvas pixels mask_of(k, ok) keeps: the texel every such sample loads"""
    out = []
    for k, c in enumerate(r.coords):
        xs, ys, ok = c
        m = mask_of(k, ok)
        out.append((xs[m].astype(np.int32), ys[m].astype(np.int32)))
    return out


# ---- the inputs say what the docstring says -------------------------------------------------------------------------------------------------
def test_bytes_take_every_value_in_every_position(case):
    seen = np.zeros(256, bool)
    for img in case.imgs:
        seen[np.unique(img)] = True
        pair = np.concatenate([img[:, :-1], img[:, 1:]], axis=2)             # [h, w - 1, 6]: the six bytes of the texel pair at xi
        for j in range(6):
            col = pair[..., j]
            assert (col == 255).any() or img.shape[1] < 26, (img.shape, j)
            assert (col >= 128).any(), (img.shape, j)
    assert seen.all()
    big = np.concatenate([np.concatenate([i[:, :-1], i[:, 1:]], axis=2).reshape(-1, 6) for i in case.imgs])
    assert all((big[:, j] == 255).any() for j in range(6))


@pytest.mark.parametrize("pad", PADS)
def test_geometry_takes_both_load_forms(rst, layouts, pad):
    """of the samples the refined render loads (a subset of what the blended renders and the statistics load): xi = w - 2, w - 3 and w - 4 occur
    in the last row pair and above it; the wide form is taken, on tight rows the narrow one too, at xi = w - 2 on both sides of the switch;
    and the 8-byte loads start at every residue mod 8"""
    fr = layouts[pad][0]
    loaded = _samples(rst, lambda k, ok: ok & (rst.top == k))
    wide_n = narrow_n = 0
    last_col = set()
    residues = set()
    hit = set()
    for k, (xi, yi) in enumerate(loaded):
        w, h, ws = int(fr.w[k]), int(fr.h[k]), int(fr.ws[k])
        assert len(xi) and xi.min() >= 0 and xi.max() <= w - 2 and yi.max() <= h - 2
        wide = 3 * xi + 8 <= ws
        wide_n += int(wide.sum()); narrow_n += int((~wide).sum())
        assert ((3 * xi + 8)[wide] <= ws).all()                             # the 8 bytes end inside the row's pitch
        edge = xi == w - 2
        if edge.any():
            last_col |= set(np.unique(wide[edge]).tolist())
        addr = fr.base[k] + yi.astype(np.int64) * ws + 3 * xi
        residues |= set(np.unique(addr[wide] % 8).tolist())
        for d in (2, 3, 4):
            for last in (True, False):
                if ((xi == w - d) & ((yi == h - 2) == last)).any():
                    hit.add((d, last, w))
    for d in (2, 3, 4):
        for last in (True, False):
            assert sum(1 for (dd, ll, w) in hit if (dd, ll) == (d, last)) >= 3, (d, last, sorted(hit))
    for w in (3, 4, 5):
        assert (2, True, w) in hit and (2, False, w) in hit, (w, sorted(hit))
    assert residues == set(range(8)), residues
    assert wide_n > 1000
    if pad == "ipl":
        assert narrow_n > 50 and last_col == {True, False}, (narrow_n, last_col)     # w % 4 of 2, 3 leave room for 8 bytes at w - 2; 0, 1 do not
    else:
        assert narrow_n == 0 and last_col == {True}                         # padded rows: 8 bytes from the last texel pair stay inside the pitch


# ---- the canvas renders -----------------------------------------------------------------------------------------------------------------------
def _canvas(rst):
    import torch
    t = torch.full((rst.ch + 1, rst.cws), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _check_canvas(t, want, rst, what):
    got = t.cpu().numpy()
    pix = np.ascontiguousarray(got[:rst.ch, :3 * rst.cw]).reshape(rst.ch, rst.cw, 3)
    bad = (pix != want).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first (y, x) {np.argwhere(bad)[0].tolist()}"
    assert (got[rst.ch] == 0xA5).all(), f"{what}: the guard row was written"


@pytest.mark.parametrize("pad", PADS)
def test_refined_render(ctx, rst, case, layouts, pad):
    fr, t, ptrs = layouts[pad]
    w, h, ws = fr.geom()
    o = _canvas(rst)
    ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, case.h9s, o.data_ptr(), rst.cw, rst.ch, rst.cws)
    ctx.synchronize()
    _check_canvas(o, np.ascontiguousarray(rst.refined[:, :3 * rst.cw]).reshape(rst.ch, rst.cw, 3), rst, f"refined {pad}")
    assert np.array_equal(fr.device_bytes(t), fr.buf)


@pytest.mark.parametrize("pad", PADS)
def test_feathered_seamline_and_median_renders(ctx, rst, case, layouts, pad):
    fr, t, ptrs = layouts[pad]
    w, h, ws = fr.geom()
    assert int(rst.layers.max()) >= 3                                       # the median at depth 3 has three samples to choose from
    o = _canvas(rst)
    ctx.MosaicFeatheredDev(ptrs, w, h, ws, case.h9s, o.data_ptr(), rst.cw, rst.ch, rst.cws, ramp=0)
    _check_canvas(o, rst.feather(0)[0], rst, f"feathered {pad}")
    o = _canvas(rst)
    ctx.MosaicSeamlineDev(ptrs, w, h, ws, case.h9s, o.data_ptr(), rst.cw, rst.ch, rst.cws, ramp=0)
    _check_canvas(o, rst.seamline(0)[0], rst, f"seamline {pad}")
    o = _canvas(rst)
    ctx.MosaicMedianDev(ptrs, w, h, ws, case.h9s, o.data_ptr(), rst.cw, rst.ch, rst.cws, ramp=0, depth=3)
    _check_canvas(o, rst.median(0, 3)[0], rst, f"median depth 3 {pad}")
    assert np.array_equal(fr.device_bytes(t), fr.buf)


# ---- the statistics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", PADS)
def test_gain_and_sharpness_statistics(ctx, rst, case, layouts, pad):
    fr, t, ptrs = layouts[pad]
    w, h, ws = fr.geom()
    st, cover = ctx.GainStatsDev(ptrs, w, h, ws, case.h9s, PAIRS, 1)
    recs, cov_ref = gr.stats_ref(rst.maps, PAIRS, 1)
    assert np.array_equal(cover, cov_ref), (cover, cov_ref)
    for i, (a, b) in enumerate(PAIRS):
        nn, sa, sb = recs[i]
        assert (int(st[i]["a"]), int(st[i]["b"])) == (a, b)
        assert int(st[i]["n"]) == nn and np.array_equal(st[i]["sum_a"], sa) and np.array_equal(st[i]["sum_b"], sb), (i, a, b, st[i], recs[i])
    assert sum(int(rec[0] > 0) for rec in recs) >= 10
    sst, sfs = ctx.SharpStatsDev(ptrs, w, h, ws, case.h9s, PAIRS, 1)
    want_st, want_fs = shr.stats_ref(shr.lap_maps(rst.maps), PAIRS, 1)
    assert sst.tobytes() == want_st.tobytes(), [(tuple(int(v) for v in a), tuple(int(v) for v in b)) for a, b in zip(sst, want_st) if a != b][:3]
    assert sfs.tobytes() == want_fs.tobytes()
    assert sum(int(s["n"] > 0) for s in want_st) >= 6


# ---- the single-image warp (warp_kernel) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", PADS)
def test_single_image_warp(ctx, oracle, case, layouts, pad):
    fr = layouts[pad][0]
    for k in range(len(SIZES)):
        for h9 in (_turn(0, 1, 0.5, 0.25), _turn(31, 1.2, 3, 4, 1e-4, 2e-4)):
            dst = C.c_void_p()
            dw, dh, dws = C.c_int(), C.c_int(), C.c_int()
            rc = ctx.L.mi355_warp_image(ctx._h, C.c_void_p(fr.host_ptrs()[k]), int(fr.w[k]), int(fr.h[k]), int(fr.ws[k]), 3, h9.ctypes.data_as(C.c_void_p),
                                        C.byref(dst), C.byref(dw), C.byref(dh), C.byref(dws))
            assert rc == 0, (rc, (ctx.L.mi355_last_error(ctx._h) or b"").decode())
            buf = np.ctypeslib.as_array(C.cast(dst, ol.u8p), shape=(dh.value, dws.value)).copy()
            ctx.L.mi355_free(dst)
            rc, want = oracle.image_projection_transform(case.imgs[k], h9)
            assert rc == 0 and (dw.value, dh.value, dws.value) == want[1:] and np.array_equal(buf, want[0]), (pad, k, SIZES[k])


# ---- undistortion and the local warp (texel_sample3: xi + 3 <= w) -----------------------------------------------------------------------------
def _texel_forms(xs, ys, w, h, has=None):
    """(wide, narrow) counts of texel_sample3 and the (w - xi, last row pair) classes its samples fall in"""
    has = np.ones(xs.shape, bool) if has is None else has
    xi = np.minimum(xs[has].astype(np.int32), w - 2)
    yi = np.minimum(ys[has].astype(np.int32), h - 2)
    wide = xi + 3 <= w
    return int(wide.sum()), int((~wide).sum()), {(int(w - a), bool(b)) for a, b in zip(xi, yi == h - 2)}


@pytest.mark.parametrize("pad", PADS)
def test_undistortion(ctx, case, layouts, pad):
    import torch
    import imagemosaicing_amd as im
    fr, t, ptrs = layouts[pad]
    w, h, ws = fr.geom()
    fd = pf.PitchedFrames([np.zeros_like(i) for i in case.imgs], [3 * int(x) + 5 for x in w], offsets=[(3 * k) % 4 for k in range(len(SIZES))], seed=7)
    for cam, out in ((ur.camera(64.0, 64.0, 1.0, 1.0), (64.0, 64.0, 0.5, 0.75)),                 # xs = u + 0.5, ys = v + 0.25: identity-like
                     (ur.camera(30.0, 31.0, 1.6, 2.2, 0.2, 0.05, 1e-3, -2e-3, 0.01), None)):
        td, dp = fd.to_device(torch)
        params = im.undistort_params(fill=200) if out is None else im.undistort_params(out_fx=out[0], out_fy=out[1], out_cx=out[2], out_cy=out[3], fill=200)
        cnt = ctx.UndistortFramesDev(ptrs, dp, w, h, fr.ws, fd.ws, im.Camera(**cam), params)
        got = fd.device_bytes(td)
        wide_n = narrow_n = 0
        classes = set()
        for k in range(len(SIZES)):
            want, n_out = ur.undistort(case.imgs[k], cam, out, 200)
            assert np.array_equal(fd.pixels(k, got), want), (pad, k, SIZES[k], int((fd.pixels(k, got) != want).sum()))
            assert cnt[k] == n_out
            xs, ys = ur.source_map(cam, int(w[k]), int(h[k]), out)
            a, b, c = _texel_forms(xs, ys, int(w[k]), int(h[k]), ur.inside(xs, ys, int(w[k]), int(h[k])))
            wide_n += a; narrow_n += b
            classes |= {(d, last, int(w[k])) for d, last in c}
        assert wide_n > 1000 and narrow_n > 50                              # both forms of texel_sample3, many times over
        if out is not None:
            for d in (2, 3, 4):
                for last in (True, False):
                    assert sum(1 for (dd, ll, x) in classes if (dd, ll) == (d, last)) >= 3, (d, last)
            assert {(2, True, 3), (2, True, 4), (2, True, 5), (3, False, 3), (3, False, 4), (3, False, 5)} <= classes
        del td
    assert np.array_equal(fr.device_bytes(t), fr.buf)


@pytest.mark.parametrize("pad", PADS)
def test_local_warp(ctx, case, layouts, pad):
    import torch
    fr, t, ptrs = layouts[pad]
    w, h, ws = fr.geom()
    n = len(SIZES)
    rng = np.random.default_rng(5)
    grids = np.zeros((n, 3, 3, 2), np.float32)
    grids[..., 0], grids[..., 1] = 0.5, 0.25                                 # identity-like: every texel pair of every row pair is read
    grids[1::2] += rng.uniform(-1.5, 1.5, grids[1::2].shape).astype(np.float32)
    fd = pf.PitchedFrames([np.zeros_like(i) for i in case.imgs], [3 * int(x) + 7 for x in w], offsets=[(k + 2) % 4 for k in range(n)], seed=8)
    td, dp = fd.to_device(torch)
    cnt = ctx.ApplyLocalWarpsDev(ptrs, dp, w, h, fr.ws, fd.ws, grids)
    got = fd.device_bytes(td)
    wide_n = narrow_n = 0
    classes = set()
    for k in range(n):
        want, nc = lr.apply(case.imgs[k], grids[k])
        assert np.array_equal(fd.pixels(k, got), want), (pad, k, SIZES[k], int((fd.pixels(k, got) != want).sum()))
        assert cnt[k] == nc
        xs, ys, _ = lr.source_map(int(w[k]), int(h[k]), grids[k])
        a, b, c = _texel_forms(xs, ys, int(w[k]), int(h[k]))
        wide_n += a; narrow_n += b
        classes |= {(d, last, int(w[k])) for d, last in c}
    assert wide_n > 1000 and narrow_n > 100
    for d in (2, 3, 4):
        for last in (True, False):
            assert sum(1 for (dd, ll, x) in classes if (dd, ll) == (d, last)) >= 3, (d, last)
    assert {(2, True, 3), (2, True, 4), (2, True, 5), (3, False, 3), (3, False, 4), (3, False, 5)} <= classes
    assert np.array_equal(fr.device_bytes(t), fr.buf)
    del td

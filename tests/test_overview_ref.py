"""CPU: tests/overview_ref.py, the numpy restatement of the overview levels (include/mi355_mosaic.h), meets the consequences the header
states -- the direct definition equals the sums carried from level to level, every byte lies between the smallest and the largest valid
sample of its block, a constant stays constant up to the edge, n > 0 is the OR of the valid map, stripes equal the whole, the three
no-data modes differ where they should -- and the library's host geometry (mi355_overview_layout) equals the formulas.
"""
import numpy as np
import pytest

from tests import overview_ref as ovr

SIZES = [(1, 1), (2, 2), (3, 3), (127, 129), (128, 128), (129, 127), (1, 300), (300, 1), (1000, 750)]      # (cw, ch)


def _canvas(cw, ch, seed, hole=0.3):
    """random pixels [ch, cw, 3] with zeroed (no-data) patches, and a sparse map that is NOT the non-zero set"""
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)
    pix[rng.random((ch, cw)) < hole] = 0
    pix[: ch // 3, : cw // 4] = 0
    vmap = (rng.random((ch, cw)) < 0.5).astype(np.uint16) * rng.integers(1, 65536, (ch, cw)).astype(np.uint16)
    vmap[ch // 2:, cw // 2:] = 0
    return pix, vmap


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("cw,ch", SIZES)
def test_direct_equals_carried_and_bounds_hold(cw, ch):
    pix, vmap = _canvas(cw, ch, cw * 1000 + ch)
    for nodata in (ovr.NONE, ovr.ZERO, ovr.MAP):
        direct = ovr.overview_ref(pix, cw, 7, nodata, vmap)
        assert _same(direct, ovr.overview_carried(pix, cw, 7, nodata, vmap)), nodata
        V = ovr.valid_map(pix, nodata, vmap)
        for l, ((ow, oh, ows), (lev, cov)) in enumerate(zip(ovr.layout(cw, ch, 7), direct), 1):
            assert lev.shape == (oh, ows) and cov.shape == (oh, ow) and lev.dtype == np.uint8 and cov.dtype == np.uint16
            assert not lev[:, 3 * ow:].any()                                   # padding
            out = lev[:, :3 * ow].reshape(oh, ow, 3)
            lo, hi = ovr.block_min_max(pix, V, l)
            has = cov > 0
            assert np.all(out[has] >= lo[has]) and np.all(out[has] <= hi[has]) and not out[~has].any()
            # n > 0 is the OR of V over the block; n counts it
            b = 1 << l
            for (X, Y) in [(0, 0), (ow - 1, oh - 1), (ow // 2, oh // 2)]:
                blk = V[Y * b:(Y + 1) * b, X * b:(X + 1) * b]
                assert cov[Y, X] == blk.sum() and (cov[Y, X] > 0) == blk.any()
            assert int(cov.sum()) == int(V.sum())


def test_full_blocks_give_the_rounded_box_mean():
    rng = np.random.default_rng(5)
    pix = rng.integers(0, 256, (256, 384, 3), dtype=np.uint8)
    for l, (lev, cov) in enumerate(ovr.overview_ref(pix, 384, 7), 1):
        b = 1 << l
        assert np.all(cov == b * b)
        mean = pix.reshape(256 // b, b, 384 // b, b, 3).astype(np.float64).mean(axis=(1, 3))
        want = np.floor(mean + 0.5).astype(np.uint8)                            # (S + n/2) / n with n even: round half up
        assert np.array_equal(lev[:, :3 * (384 // b)].reshape(256 // b, 384 // b, 3), want)


@pytest.mark.parametrize("cw,ch", [(129, 127), (1000, 750)])
def test_a_constant_stays_constant_up_to_the_edge(cw, ch):
    """a survey of one colour inside an irregular outline, zeros outside: with the coverage known no level shows any other colour"""
    yy, xx = np.mgrid[:ch, :cw]
    inside = ((xx - cw / 2.0) ** 2 / (cw / 2.3) ** 2 + (yy - ch / 2.0) ** 2 / (ch / 2.1) ** 2) < 1
    colour = np.array([13, 200, 255], np.uint8)
    pix = np.where(inside[..., None], colour, 0).astype(np.uint8)
    for nodata, vmap in ((ovr.ZERO, None), (ovr.MAP, inside.astype(np.uint16))):
        for (ow, oh, ows), (lev, cov) in zip(ovr.layout(cw, ch, 7), ovr.overview_ref(pix, cw, 7, nodata, vmap)):
            out = lev[:, :3 * ow].reshape(oh, ow, 3)
            assert np.all(out[cov > 0] == colour) and not out[cov == 0].any()
    # without the coverage the edge is smeared: that is what the modes are for
    lev, cov = ovr.overview_ref(pix, cw, 3)[2]
    out = lev[:, :3 * cov.shape[1]].reshape(cov.shape + (3,))
    assert np.any((out[..., 1] > 0) & (out[..., 1] < 200))


@pytest.mark.parametrize("levels", [1, 3, 7])
def test_stripes_equal_the_whole(levels):
    cw, ch = 301, 1000
    pix, vmap = _canvas(cw, ch, 77)
    u = 1 << levels
    cuts = [0, u, 4 * u] + ([7 * u] if 7 * u < ch else []) + [ch]
    for nodata in (ovr.NONE, ovr.ZERO, ovr.MAP):
        assert _same(ovr.stripes(pix, cw, levels, cuts, nodata, vmap), ovr.overview_ref(pix, cw, levels, nodata, vmap))


def test_the_three_modes_differ_where_they_should():
    pix, vmap = _canvas(208, 160, 9)
    none, zero, bymap = (ovr.overview_ref(pix, 208, 4, m, vmap) for m in (ovr.NONE, ovr.ZERO, ovr.MAP))
    V0, VM = pix.any(axis=2), vmap != 0
    for l in range(1, 5):
        b = 1 << l
        assert np.all(none[l - 1][1] == b * b)                                  # 208 x 160: whole blocks
        for mode, V in ((zero, V0), (bymap, VM)):
            full = ovr.block_sums(V, l) == b * b
            lev, cov = mode[l - 1]
            ow = cov.shape[1]
            a, r = lev[:, :3 * ow].reshape(cov.shape + (3,)), none[l - 1][0][:, :3 * ow].reshape(cov.shape + (3,))
            assert np.array_equal(a[full], r[full])                             # where everything is valid the modes agree
            assert np.any(a[~full] != r[~full])                                 # and elsewhere they do not
        assert not np.array_equal(zero[l - 1][1], bymap[l - 1][1])
    # saturated input at the deepest level: the sum 255 * 16384 + 8192 is carried whole
    lev, cov = ovr.overview_ref(np.full((128, 128, 3), 255, np.uint8), 128, 7)[6]
    assert cov[0, 0] == 16384 and lev[0, :3].tolist() == [255, 255, 255]


# ---- against the library (host geometry: no GPU) ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def im():
    from imagemosaicing_amd import build
    build.build()
    import imagemosaicing_amd
    return imagemosaicing_amd


def test_library_layout_equals_the_formulas(im):
    for cw, ch in SIZES:
        for levels in range(1, 8):
            assert im.overview_layout(cw, ch, levels) == ovr.layout(cw, ch, levels), (cw, ch, levels)
    for bad in (0, 8, -1):
        with pytest.raises(im.Mi355Error) as e:
            im.overview_layout(100, 100, bad)
        assert e.value.code == -1
    with pytest.raises(im.Mi355Error):
        im.overview_layout(0, 100, 3)
    assert im.overview_layout(100, 100, 7)[6] == (1, 1, 4)                       # the refusals leave the call usable


def test_new_symbols_are_exported_and_params_default(im):
    L = im.load_library()
    for name in ("mi355_overview_layout", "mi355_mosaic_overview_dev", "mi355_mosaic_overview", "mi355_default_preview_params",
                 "mi355_mosaic_preview_into"):
        assert hasattr(L, name), name
    p = im.preview_params()
    assert (p.render, p.ramp, p.level, p.nodata) == (0, 0, 3, im.NODATA_MAP) and not any(p.reserved)
    p = im.preview_params(render=2, ramp=16, level=5, nodata=im.NODATA_ZERO)
    assert (p.render, p.ramp, p.level, p.nodata) == (2, 16, 5, 1)
    import ctypes
    assert ctypes.sizeof(im.PreviewParams) == 32

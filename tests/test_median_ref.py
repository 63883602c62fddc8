"""CPU: the median render (include/mi355_mosaic.h, "median render").

  * the numpy restatement (tests/median_ref.py, built from the oracle's refined render) on the reference's committed 20-frame run
    (tests/golden) and on the 10-frame case of tests/test_gpu_gain.py (projective frames, a skipped frame), at ramp 0 and 16: with depth 1 the
    canvas is the seamline restatement's; where one frame covers a pixel the bytes are the refined render's; every byte lies between the
    smallest and the largest selected sample; the spread is 0 where at most one frame is selected; the count is the seamline count;
  * reversing the frame order changes nothing beyond what the index tie-break at the selection boundary dictates;
  * the moving-object property, the point of the render: a block painted into one of five exact looks at a scene drops out wherever the dirty
    looks are a minority of the selected ones, while the feathered mean keeps a ghost of it, and the spread map shows where it was;
  * a built tie at the selection boundary, which the index decides;
  * the new symbols are exported and declared, the parameter struct is 16 bytes, the adaptor's MosaicImagesMedian compiles in both modes, and
    the binding fails loudly without a context.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import feather_ref as fr
from tests import gain_ref as gr
from tests import median_ref as mr
from tests import seamline_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355_default_median_params", "mi355_mosaic_median_dev", "mi355_mosaic_median", "mi355_mosaic_median_into", "mi355_mosaic_median_cover")


@pytest.fixture(scope="module")
def golden(oracle):
    imgs, h9s = sr.golden_survey()
    return imgs, h9s, gr.frame_sample_maps(oracle, imgs, h9s)


@pytest.fixture(scope="module")
def case(oracle):
    from tests.test_gpu_gain import _case
    imgs, h9s, pairs = _case()
    return imgs, h9s, gr.frame_sample_maps(oracle, imgs, h9s)


def _refined(oracle, imgs, h9s):
    rc, (canvas, cw, ch, cws) = oracle.mosaic_images_refined(imgs, h9s)
    assert rc == 0
    return canvas[:, :3 * cw].reshape(ch, cw, 3)


def _check_consequences(oracle, imgs, h9s, maps, ramp, depths):
    wmaps = sr.weight_maps(oracle, imgs, h9s, ramp, maps)
    s_out, s_owner, s_count, _, _ = sr.pick(maps, wmaps)
    refined = _refined(oracle, imgs, h9s)
    # depth 1 is the seamline render
    out, spread, count, sel, tie = mr.pick(maps, wmaps, 1)
    assert np.array_equal(out, s_out) and np.array_equal(sel[0], s_owner) and np.array_equal(count, s_count) and not spread.any()
    single = s_count == 1
    assert single.sum() > 1000
    for depth in depths:
        out, spread, count, sel, tie = mr.pick(maps, wmaps, depth)
        d = depth or mr.DEFAULT_DEPTH
        assert sel.shape[0] == d and out.shape == refined.shape
        assert np.array_equal(count, s_count)
        assert np.array_equal(out[single], refined[single])
        assert np.array_equal(sel[0], s_owner)                              # the deepest frame is always among the selected
        m = np.minimum(count.astype(np.int64), d)
        assert np.array_equal((sel > 0).sum(axis=0), m)
        lo, hi = mr.selected_samples(maps, sel)
        cov = count > 0
        assert (out[cov] >= lo[cov]).all() and (out[cov] <= hi[cov]).all() and not out[~cov].any()
        assert not spread[m <= 1].any()
        assert np.array_equal(spread[cov], (hi - lo).max(axis=2)[cov])
        # every selected frame covers the pixel
        for k, mp in enumerate(maps):
            mine = (sel == k + 1).any(axis=0)
            assert not mine.any() if mp is None else not (mine & ~mp[1]).any()
    return s_count


@pytest.mark.parametrize("ramp", [0, 16])
def test_golden_survey_consequences(golden, oracle, ramp):
    imgs, h9s, maps = golden
    count = _check_consequences(oracle, imgs, h9s, maps, ramp, (0, 2, 9))
    assert (count >= 3).sum() > 10000 and count.max() >= 4                  # not vacuous: medians of three and more


@pytest.mark.parametrize("ramp", [0, 16])
def test_case_consequences(case, oracle, ramp):
    imgs, h9s, maps = case
    count = _check_consequences(oracle, imgs, h9s, maps, ramp, (0, 4, 9))
    assert (count >= 3).sum() > 1000


def test_frame_order_changes_nothing_but_the_boundary_ties(golden, oracle):
    """the selected SET depends on the caller's order only where the depth-th and the (depth + 1)-th weight are equal; a median does not look
    at the order inside the set.  Here: the reversed strip at depth 2, where the 20-frame strip has frames to spare."""
    imgs, h9s, maps = golden
    depth = 2
    out, spread, count, sel, tie = mr.median_ref(oracle, imgs, h9s, 0, depth, maps, full=True)
    perm = list(range(19, -1, -1))
    out2, spread2, count2, sel2, tie2 = mr.median_ref(oracle, [imgs[k] for k in perm], h9s[perm], 0, depth, full=True)
    assert np.array_equal(count, count2) and np.array_equal(tie, tie2)
    back = np.zeros(21, np.int64)
    back[1:] = [perm[q] + 1 for q in range(20)]
    same = ~tie
    assert np.array_equal(np.sort(back[sel2], axis=0)[:, same], np.sort(sel.astype(np.int64), axis=0)[:, same])
    assert np.array_equal(out[same], out2[same]) and np.array_equal(spread[same], spread2[same])
    assert same.mean() > 0.9 and (count > depth).sum() > 10000


def test_a_moving_object_drops_out(oracle):
    clean, dirty, h9s, (bx, by, block) = mr.moving_object_case()
    cmaps = gr.frame_sample_maps(oracle, clean, h9s)
    dmaps = gr.frame_sample_maps(oracle, dirty, h9s)
    c_out, c_spread, count, sel, _ = mr.median_ref(oracle, clean, h9s, 0, 9, cmaps, full=True)
    d_out, d_spread, d_count, d_sel, _ = mr.median_ref(oracle, dirty, h9s, 0, 9, dmaps, full=True)
    assert np.array_equal(count, d_count) and np.array_equal(sel, d_sel)   # selection does not look at texels
    assert not c_spread.any()                                               # five exact looks at one scene agree everywhere
    m = np.minimum(count.astype(np.int64), 9)
    n_dirty = np.zeros(count.shape, np.int64)
    for k in range(len(clean)):
        n_dirty += (dmaps[k][0] != cmaps[k][0]).any(axis=2) & (sel == k + 1).any(axis=0)
    foot = n_dirty > 0
    assert foot.sum() == block * block and foot[by:by + block, bx:bx + block].all() and n_dirty.max() == 1
    assert (m[foot] >= 3).all()
    ok = 2 * n_dirty < m
    assert ok[foot].all()
    assert np.array_equal(d_out[ok], c_out[ok])                             # the block is gone
    assert (d_spread[foot] > 0).all() and not d_spread[~foot].any()        # and the spread map says where it was
    f_clean, _ = fr.feather_ref(oracle, clean, h9s, 0, cmaps)
    f_dirty, _ = fr.feather_ref(oracle, dirty, h9s, 0, dmaps)
    assert np.array_equal(f_clean, c_out)                                   # clean looks: every render gives the scene
    assert (f_dirty[foot] != f_clean[foot]).any(axis=1).all()              # the feathered mean keeps a ghost on every pixel of the block


def test_the_index_decides_a_tie_at_the_selection_boundary(oracle):
    imgs, h9s, col, rows = mr.boundary_tie_case()
    maps = gr.frame_sample_maps(oracle, imgs, h9s)
    out, spread, count, sel, tie = mr.median_ref(oracle, imgs, h9s, 0, 2, maps, full=True)
    assert (count[rows, col] == 3).all() and tie[rows, col].all()           # the case really holds the tie: frames 0 and 1, 13 from their borders
    assert (sel[0, rows, col] == 3).all() and (sel[1, rows, col] == 2).all()            # frame 2 is deepest; of the tied pair the larger index
    a, b = maps[2][0][rows, col], maps[1][0][rows, col]
    assert np.array_equal(out[rows, col], ((a + b + 1) >> 1).astype(np.uint8))
    assert np.array_equal(spread[rows, col], np.abs(a - b).max(axis=1).astype(np.uint8))
    assert (out[rows, col] != ((a + maps[0][0][rows, col] + 1) >> 1)).any()             # and it shows in the bytes
    # the tie is at the boundary only: a column further on frame 1 is strictly deeper than frame 0
    assert not tie[rows, col + 1].any() and (sel[1, rows.start + 8:rows.stop - 8, col + 1] == 2).all()


# ---- the public surface -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def im():
    from imagemosaicing_amd import build
    build.build()
    import imagemosaicing_amd
    return imagemosaicing_amd


def test_new_symbols_are_exported_and_declared(im):
    L = im.load_library()
    hdr = open(os.path.join(ROOT, "include", "mi355_mosaic.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    assert "mi355_median_params" in hdr and "#define MI355_MEDIAN_MAX_DEPTH 9" in hdr
    for name in ("MedianParams", "median_params"):
        assert hasattr(im, name), name
    for name in ("MosaicMedian", "MosaicMedianDev", "MosaicMedianInto", "MedianCover"):
        assert hasattr(im.Context, name), name
    p = im.median_params()
    assert C.sizeof(p) == 16 and p.ramp == 0 and p.depth == 0 and list(p.reserved) == [0, 0]
    p = im.median_params(ramp=12, depth=7)
    assert p.ramp == 12 and p.depth == 7


def test_parameter_struct_is_16_bytes_in_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mi355_mosaic.h"\n'
                   'typedef char size_is_16[sizeof(mi355_median_params) == 16 ? 1 : -1];\n'
                   'typedef char same_as_seamline[sizeof(mi355_median_params) == sizeof(mi355_seamline_params) ? 1 : -1];\n'
                   'typedef char max_depth_is_9[MI355_MEDIAN_MAX_DEPTH == 9 ? 1 : -1];\n'
                   'int main(void) { mi355_median_params p; p.ramp = 0; p.depth = 5; p.reserved[1] = 0; return p.ramp; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("keep", [False, True])
def test_adaptor_median_compiles_as_cxx(tmp_path, keep):
    src = tmp_path / "t.cpp"
    src.write_text('#include "mi355_adaptor.h"\nusing namespace mi355ref;\n'
                   'int f(ImagePoseInfo* p, int n, ImageTransform* t, int mode) {\n'
                   '  IplImage* out = NULL;\n'
                   '  int rc = mode == 4 ? mi355::MosaicImagesMedian(p, n, t, out) : mi355::MosaicImagesSeamline(p, n, t, out);\n'
                   '  cvReleaseImage(&out); return rc; }\n'
                   'int main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-c"] + (["-DMI355_ADAPTOR_KEEP_FRAMES"] if keep else []) +
                       ["-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    syms = subprocess.run(["nm", "-C", str(tmp_path / "t.o")], capture_output=True, text=True).stdout
    for name in ("mi355_mosaic_median_into", "mi355_mosaic_seamline_into"):
        assert name in syms, name


def test_binding_raises_without_a_context(im):
    """a context that does not exist: every new method reaches the C ABI and fails there, loudly (no CPU path answers instead)"""
    ctx = im.Context.__new__(im.Context)
    ctx.L, ctx._h, ctx.device = im.load_library(), C.c_void_p(), 0
    img = np.zeros((32, 32, 3), np.uint8)
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    h9s[1, 2] = 10
    for call in (lambda: ctx.MosaicMedian([img, img], h9s),
                 lambda: ctx.MosaicMedian([img, img], h9s, ramp=4, depth=3, want_spread=True),
                 lambda: ctx.MosaicMedianDev([0, 0], [32, 32], [32, 32], [96, 96], h9s, 0, 42, 32, 128, d_spread=0, d_count=0),
                 lambda: ctx.MosaicMedianInto([img, img], None, h9s),
                 lambda: ctx.MedianCover([32, 32], [32, 32], h9s)):
        with pytest.raises(im.Mi355Error) as e:
            call()
        assert e.value.code == -1

"""The multiband blend along optimised seams on the CPU: tests/blend_seam_ref.py restates the definition in include/mi355_mosaic.h, and every
case of tests/blend_seam_patterns.py holds what its name says.  No GPU: tests/test_gpu_blend_seam.py compares the build with this restatement."""
import numpy as np
import pytest

from tests import blend_seam_patterns as bp
from tests import blend_seam_ref as bs
from tests import oracle_lib as ol
from tests import seamcut_ref as sc


@pytest.fixture(scope="module")
def orc():
    return ol.load_oracle()


def _moved(r):
    return r["best"] != r["set"]["best"]


def _probes(s, level):
    st = 1 << level
    gw, gh = sc.grid_of(s["cw"], s["ch"], level)
    return np.minimum(np.arange(gh) * st + st // 2, s["ch"] - 1), np.minimum(np.arange(gw) * st + st // 2, s["cw"] - 1)


@pytest.mark.parametrize("name", sorted(bp.CASES))
def test_every_case(orc, name):
    """slot 0 is FindMasksByDistMap's owner at every probe, omega does not increase along the slots, the energy does not rise unless the
    fallback says so, a zero map gives the oracle's masks, and the masks partition what `best` says"""
    case, cells, r = bp.reference(orc, name)
    s, p = r["set"], case.p
    py, px = _probes(s, p["level"])
    assert np.array_equal(r["slot0"], s["best"][np.ix_(py, px)]), "slot 0 is not the probe's owner"
    om = r["omega"].astype(int)
    assert (np.diff(om, axis=2) <= 0).all() and ((r["frame"] > 0) == (om > 0)).all()
    filled = (r["frame"] > 0).sum(axis=2)
    assert filled.max() <= p["depth"] and ((r["frame"] > 0) == (np.arange(8)[None, None] < filled[..., None])).all()
    rep = r["report"]
    assert rep["energy_after"] <= rep["energy_before"] or rep["fallback"]
    o = orc.chips_and_masks(case.imgs, case.h9s, keep=case.keep)
    gw, gh = sc.grid_of(s["cw"], s["ch"], p["level"])
    zero, best0 = bs.ownership_under(s, np.zeros((gh, gw), np.uint16), p["level"])
    assert (o["cw"], o["ch"]) == (s["cw"], s["ch"]) and len(zero) == len(o["masks"])
    assert all(np.array_equal(a, b) for a, b in zip(zero, o["masks"])) and np.array_equal(best0, s["best"])
    assert all(np.array_equal(a, b) for a, b in zip(s["chip_imgs"], o["chip_imgs"]))
    total = sum(int((m[:, :int(c["w"])] == 255).sum()) for m, c in zip(r["masks"], s["chips"]))
    assert total == int((r["best"] >= 0).sum())
    # the map moves a pixel only to a chip whose image its cell names and that is valid there
    mv = _moved(r)
    used = r["cells"] if cells is None else cells
    want = np.repeat(np.repeat(used.astype(int), 1 << p["level"], 0), 1 << p["level"], 1)[:s["ch"], :s["cw"]] - 1
    img = np.array([int(c["img"]) for c in s["chips"]] + [-2])
    assert (img[r["best"]][mv] == want[mv]).all()
    assert all(s["cover"][v][mv & (r["best"] == v)].all() for v in range(len(s["chips"])))


@pytest.mark.parametrize("name", sorted(bp.CRAFTED_EXPECT))
def test_crafted_scenes(orc, name):
    """changed > 0, no fallback, the rectangle under one owner afterwards -- and the figures of the prototype this feature was planned on"""
    case, _, r = bp.reference(orc, name)
    x, y, w, h = bp.crafted_rect(name)
    before, after = r["set"]["best"][y:y + h, x:x + w], r["best"][y:y + h, x:x + w]
    rep = r["report"]
    assert rep["changed"] > 0 and not rep["fallback"] and rep["energy_after"] < rep["energy_before"]
    assert len(np.unique(after)) == 1 and len(np.unique(before)) == 2
    got = (rep["energy_before"], rep["energy_after"], rep["changed"], tuple(int((before == k).sum()) for k in (0, 1)),
           tuple(int((after == k).sum()) for k in (0, 1)), int(_moved(r).sum()))
    assert got == bp.CRAFTED_EXPECT[name]


def test_symmetric_stays_cut(orc):
    _, _, r = bp.reference(orc, "symmetric2")
    x, y, w, h = bp.crafted_rect("symmetric2")
    after = r["best"][y:y + h, x:x + w]
    assert [int((after == k).sum()) for k in (0, 1)] == [96, 96] and not r["report"]["fallback"]


def test_holes_and_staircase(orc):
    _, _, r = bp.reference(orc, "holes")
    filled = (r["frame"] > 0).sum(axis=2)
    assert (filled == 0).any() and (filled == 1).any() and (filled == 0)[:, 1:-1].any(axis=0).any() and (filled == 0)[1:-1].any(axis=1).any()
    _, _, r = bp.reference(orc, "staircase")
    row = (r["frame"] > 0).sum(axis=2)[2]
    assert set(row.tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("depth", range(1, 9))
def test_nine_depth(orc, depth):
    case, _, r = bp.reference(orc, "nine_depth%d" % depth)
    assert case.p["depth"] == depth and int((r["frame"] > 0).sum(axis=2).max()) == depth
    if depth == 1:
        assert not _moved(r).any() and r["report"]["changed"] == 0


def test_twins_lower_index_leads(orc):
    _, _, r = bp.reference(orc, "twins")
    s = r["set"]
    assert np.array_equal(s["d"][0], s["d"][1]) and np.array_equal(s["cover"][0], s["cover"][1])
    both = (r["frame"] == 1).any(axis=2) & (r["frame"] == 2).any(axis=2)
    assert both.any()
    i1, i2 = np.argmax(r["frame"] == 1, axis=2), np.argmax(r["frame"] == 2, axis=2)
    assert (i2[both] == i1[both] + 1).all()
    assert (np.take_along_axis(r["omega"], i1[..., None], 2)[..., 0][both] == np.take_along_axis(r["omega"], i2[..., None], 2)[..., 0][both]).all()
    assert not (s["best"] == 1).any()


def test_skipped_dropped_and_foreign_ids(orc):
    _, _, r = bp.reference(orc, "skipped")
    assert len(r["set"]["chips"]) == 3 and not (r["frame"] == 4).any()
    case, cells, r = bp.reference(orc, "keep_drops")
    assert len(r["set"]["chips"]) == 2 and (cells == 2).all() and not (r["frame"] == 2).any() and not _moved(r).any()
    _, cells, r = bp.reference(orc, "above_n")
    assert cells.max() == 65535 and (cells == 4).any() and not _moved(r).any()
    _, cells, r = bp.reference(orc, "random_ids")
    assert _moved(r).sum() > 100 and set(np.unique(cells).tolist()) == {0, 1, 2, 3, 4}
    _, cells, r = bp.reference(orc, "far_ids")
    assert cells.min() >= 1 and not _moved(r).any()                                 # every cell names a frame, none of them covers it


def test_projective_and_big(orc):
    _, _, r = bp.reference(orc, "projective")
    c = r["set"]["chips"]
    assert (c["sx"] != 0).any() and (c["sy"] != 0).any() and _moved(r).any()
    _, _, r = bp.reference(orc, "big")
    s = r["set"]
    assert s["cw"] > 256 and s["ch"] > 256 and _moved(r).any()
    mv = _moved(r)
    assert sum(bool(mv[y:y + 256, x:x + 256].any()) for y in (0, 256) for x in (0, 256)) >= 3      # the map is followed in several ownership blocks


@pytest.mark.parametrize("n", (33, 65, 130))
def test_many_chips_in_one_block(orc, n):
    _, _, r = bp.reference(orc, "many%d" % n)
    s = r["set"]
    assert len(s["chips"]) == n and s["cw"] <= 256 and s["ch"] <= 256
    assert int((r["frame"] > 0).sum(axis=2).max()) == 8 and _moved(r).any()
    assert int(s["cover"].sum(axis=0).max()) > min(n // 2, 64)                      # far more covering chips than slots in the central cells
    assert (np.unique(r["frame"])[-1] > 64) == (n > 64)                             # candidates from beyond one chip per lane


def test_chips_without_a_distance_own_through_the_map(orc):
    _, _, r1 = bp.reference(orc, "thin_named1")
    s = r1["set"]
    with np.errstate(invalid="ignore"):
        assert all(not (s["d"][v] > 0).any() for v in (1, 2, 3)) and s["cover"][1].sum() == 39 and s["cover"][3].sum() == 1
    assert not np.isin(r1["frame"], (2, 3, 4)).any() and not np.isin(s["best"], (1, 2, 3)).any()
    assert int(_moved(r1).sum()) == 39 and (r1["best"][_moved(r1)] == 1).all()
    _, _, r3 = bp.reference(orc, "thin_named3")
    assert int(_moved(r3).sum()) == 1 and (r3["best"][_moved(r3)] == 3).all()
    _, _, r0 = bp.reference(orc, "no_valid_named")
    assert r0["set"]["cover"][1].sum() == 0 and not _moved(r0).any()


@pytest.mark.parametrize("name", sorted(bp.sp.REM_CASES))
def test_remainders(orc, name):
    case, _, r = bp.reference(orc, name)
    s, level = r["set"], case.p["level"]
    st = 1 << level
    rx, ry = s["cw"] % st, s["ch"] % st
    assert 0 < rx < st and 0 < ry < st
    gw, gh = sc.grid_of(s["cw"], s["ch"], level)
    clamped_x, clamped_y = (gw - 1) * st + st // 2 > s["cw"] - 1, (gh - 1) * st + st // 2 > s["ch"] - 1
    assert clamped_x == (rx <= st // 2) and clamped_y == (ry <= st // 2)
    assert clamped_x != clamped_y                                                   # one axis clamped, the other not
    py, px = _probes(s, level)
    assert px[-1] <= s["cw"] - 1 and py[-1] <= s["ch"] - 1 and (px[-1] == s["cw"] - 1) >= clamped_x


@pytest.mark.parametrize("name", ("crafted3", "nine_depth4", "projective", "many65"))
def test_consequences(orc, name):
    """an all-zero map, depth = 1, and diff_weight = seam_penalty = 0 each give the masks of chips_and_masks and the canvas of the blend"""
    case, _, r = bp.reference(orc, name)
    o = orc.chips_and_masks(case.imgs, case.h9s, keep=case.keep)
    canvas = orc.multiband_blend(o["chips"], o["chip_imgs"], o["masks"], o["cw"], o["ch"], 5)[0]
    gw, gh = sc.grid_of(o["cw"], o["ch"], case.p["level"])
    for what, p, cells in (("zero map", case.p, np.zeros((gh, gw), np.uint16)), ("depth 1", dict(case.p, depth=1), None),
                           ("free seams", dict(case.p, diff_weight=0, seam_penalty=0), None)):
        q = bs.blend_seam_ref(orc, case.imgs, case.h9s, p, keep=case.keep, cells=cells, chips=r["set"])
        assert all(np.array_equal(a, b) for a, b in zip(q["masks"], o["masks"])), what
        assert np.array_equal(q["canvas"], canvas), what
        if cells is None:
            assert not q["cells"].any() and q["report"]["changed"] == 0, what
    assert not np.array_equal(r["canvas"], canvas)                                  # while the case's own map moves the seam


@pytest.mark.parametrize("mutate", bs.MUTATIONS)
def test_each_mutation_shows(orc, mutate):
    """every rule the restatement can get wrong changes the records, the masks or the canvas of at least one case"""
    seen = []
    for name in ("twins", "thin_named1", "crafted2", "nine_depth4", "many65"):
        case, cells, r = bp.reference(orc, name)
        q = bs.blend_seam_ref(orc, case.imgs, case.h9s, case.p, keep=case.keep, cells=cells, chips=r["set"], mutate=mutate, blend=False)
        if not np.array_equal(q["records"], r["records"]) or not np.array_equal(q["best"], r["best"]):
            seen.append(name)
    assert seen, mutate
    expect = {"tie": "twins", "dpos": "thin_named1", "round": "crafted2", "probe": "crafted2"}[mutate]
    assert expect in seen


def test_quality_file_matches_the_restatement(orc):
    """profiles/blend_seam_quality.json records seam_disagreement before and after on the crafted scenes: the figures are this restatement's"""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "blend_seam_quality.json")
    rec = json.load(open(path))["cases"]
    for name in sorted(bp.CRAFTED):
        case, _, r = bp.reference(orc, name)
        maps = bs.sample_maps(r["set"], len(case.imgs))
        before = sc.seam_disagreement(maps, bs.owner_frames(r["set"], r["set"]["best"]))
        after = sc.seam_disagreement(maps, bs.owner_frames(r["set"], r["best"]))
        assert (rec[name]["disagreement_before"], rec[name]["disagreement_after"]) == (before, after), name


def test_python_surface():
    import ctypes as C
    import imagemosaicing_amd as im
    for name in ("BlendSeamCellsDev", "ChipsAndMasksSeam", "MosaicBlendedSeamDev", "MosaicBlendedSeam", "MosaicBlendedSeamInto"):
        assert callable(getattr(im.Context, name)), name
    assert callable(im.blend_seam_grid)
    L = im.load_library()
    for sym in ("mi355_blend_seam_cells_dev", "mi355_chips_and_masks_seam", "mi355_mosaic_blended_seam_dev", "mi355_mosaic_blended_seam",
                "mi355_mosaic_blended_seam_into"):
        assert isinstance(getattr(L, sym), C._CFuncPtr), sym

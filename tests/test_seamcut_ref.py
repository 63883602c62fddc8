"""CPU: the optimised seamlines (include/mi355_mosaic.h, "optimised seamlines") on the numpy restatement alone (tests/seamcut_ref.py), and the
one stage that needs no GPU, mi355_seam_labels_host, against it.

  * identities: an all-zero cell map, depth = 1, and diff_weight = seam_penalty = 0 give the seamline restatement's bytes, owner and count; the
    returned labelling never costs more than the seamline's own on any case;
  * the crafted scenes (tests/seamcut_patterns.py: crafted): a rectangle astride the geometric mid-seam, a quarter (moved object) or half
    (relief) of its columns on frame 0's side; the seamline owner map's boundary crosses it top to bottom, the seamcut owner map has one owner
    on every pixel of it, and the full-resolution seam disagreement is strictly lower.  A moved object placed symmetrically stays cut: the
    known limit, asserted;
  * every edge the cases are named for occurs in its case;
  * each of the five mutations of the label stage changes some case's cell map;
  * the host twin gives the reference's cell map and report on every case; the C surface.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import seamcut_patterns as sp
from tests import seamcut_ref as sc
from tests import seamline_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355_default_seamcut_params", "mi355_seam_candidates_dev", "mi355_seam_labels_dev", "mi355_seam_labels_host", "mi355_seam_cells_dev",
       "mi355_mosaic_seamcut_dev", "mi355_mosaic_seamcut", "mi355_mosaic_seamcut_into", "mi355_mosaic_seamcut_cover")


def _m(r):
    return (r["frame"] > 0).sum(axis=2)


@pytest.mark.parametrize("name", sorted(sp.CASES))
def test_identities_and_energy(oracle, name):
    imgs, h9s, p, r = sp.reference(oracle, name)
    s_out, s_owner, s_count, _, _ = sr.pick(r["maps"], r["wmaps"])
    # an all-zero cell map is the seamline render
    z = sc.render(r["maps"], r["wmaps"], np.zeros_like(r["cells"]), p["level"])
    assert np.array_equal(z[0], s_out) and np.array_equal(z[1], s_owner) and np.array_equal(z[2], s_count)
    assert np.array_equal(r["count"], s_count)
    # depth 1, and no seam cost at all: nothing moves
    for kw in (dict(depth=1), dict(diff_weight=0, seam_penalty=0)):
        q = dict(p, **kw)
        f, o, g = sc.candidates(r["maps"], r["wmaps"], q["level"], q["depth"])
        cells, rep = sc.labels(f, o, g, q)
        assert not cells.any() and rep["changed"] == 0 and rep["fallback"] == 0, kw
        assert np.array_equal(f[..., 0], r["frame"][..., 0])                # slot 0 does not depend on depth
    # slot 0 is the seamline owner of the probe
    s = 1 << p["level"]
    ch, cw = s_owner.shape
    py = np.minimum(np.arange(r["cells"].shape[0]) * s + s // 2, ch - 1); px = np.minimum(np.arange(r["cells"].shape[1]) * s + s // 2, cw - 1)
    assert np.array_equal(r["frame"][..., 0], s_owner[np.ix_(py, px)])
    # never worse than the seamline labelling by its own measure
    rep = r["report"]
    assert sc.energy(r["frame"], r["omega"], r["gray"], r["slot"], p) <= rep["energy_before"]
    assert rep["fallback"] == int(rep["energy_after"] > rep["energy_before"])
    assert rep["changed"] == int((r["cells"] > 0).sum())


def _rect_owners(oracle, name, rect):
    imgs, h9s, p, r = sp.reference(oracle, name)
    x, y, rw, rh = rect
    assert p == sc.params(level=2)                                          # the defaults, at level 2
    s_owner = sr.pick(r["maps"], r["wmaps"])[1]
    assert (r["count"][y:y + rh, x:x + rw] >= 2).all()                      # the rectangle lies inside the overlap
    assert x < sp.SEAM_X < x + rw - 1                                       # and the geometric mid-seam runs through it
    before, after = sc.seam_disagreement(r["maps"], s_owner), sc.seam_disagreement(r["maps"], r["owner"])
    print("seam disagreement %s: seamline %d, seamcut %d" % (name, before, after))
    return r, s_owner[y:y + rh, x:x + rw], r["owner"][y:y + rh, x:x + rw], before, after


@pytest.mark.parametrize("frames,relief", [(2, False), (3, False), (2, True), (3, True)])
def test_the_seam_goes_round_the_rectangle(oracle, frames, relief):
    """the rectangle is astride the mid-seam: the seamline render gives frame 0 every pixel of it left of x = 43.5 -- a quarter of the moved
    object, half of the relief one -- and frame 1 the rest; the seamcut render gives all of it to one frame"""
    name = ("relief" if relief else "crafted") + str(frames)
    rect = sp.crafted(frames, relief)[3]
    r, cut, whole, before, after = _rect_owners(oracle, name, rect)
    left = int(sp.SEAM_X) + 1 - rect[0]                                     # its columns on frame 0's side
    assert left * 4 >= rect[2]
    assert (cut[:, :left] == 1).all() and (cut[:, left:] == 2).all()        # the seamline boundary crosses it top to bottom
    assert len(np.unique(whole)) == 1
    assert after < before
    assert r["report"]["fallback"] == 0 and r["report"]["changed"] > 0


def test_known_limit_a_symmetric_rectangle_stays_cut(oracle):
    """a moved object with as many columns on either side of the mid-seam: moving the seam left or right of it costs the same, the rows'
    min-marginals tie, every cell keeps slot 0 and the rectangle stays cut.  Pinned so that nobody takes the test above to cover it."""
    rect = sp.crafted(2, symmetric=True)[3]
    r, cut, whole, before, after = _rect_owners(oracle, "symmetric2", rect)
    assert rect[0] + rect[2] / 2.0 - 0.5 == sp.SEAM_X
    assert np.array_equal(whole, cut) and len(np.unique(whole)) == 2 and after == before


def test_the_edges_occur_in_their_cases(oracle):
    ref = lambda name: sp.reference(oracle, name)[3]
    assert ref("grid_1x1")["cells"].shape == (1, 1) and _m(ref("grid_1x1")).max() == 1
    assert ref("grid_1xN")["cells"].shape == (1, 7) and ref("grid_Nx1")["cells"].shape == (7, 1)
    for name, cells in (("strip_63", 63), ("strip_64", 64), ("strip_65", 65), ("strip_255", 255), ("strip_256", 256), ("strip_257", 257)):
        assert ref(name)["cells"].shape == (1, cells), name
    assert ref("strip_65_v")["cells"].shape == (65, 1) and ref("strip_257_v")["cells"].shape == (257, 1)
    # a canvas that is no multiple of the cell, in both axes
    r = ref("projective")
    assert r["owner"].shape[0] % 8 and r["owner"].shape[1] % 8 and sp.reference(oracle, "projective")[2]["level"] == 3
    # holes in the middle of a path: a run of empty cells with candidates on both sides, along a row and along a column (each is walked both ways)
    m = _m(ref("holes"))
    row, col = m[2], m[:, 2]
    for line in (row, col):
        z = np.flatnonzero(line == 0)
        assert len(z) and line[:z[0]].any() and line[z[-1] + 1:].any()
    # m from 0 to depth along one path
    r = ref("staircase")
    assert any(set(range(5)) <= set(line.tolist()) for line in _m(r))
    # nine contributors over a cell, at depth 4 and 8
    for name, depth in (("nine_depth4", 4), ("nine_depth8", 8)):
        r = ref(name)
        assert r["count"].max() == 9 and _m(r).max() == depth
    # twins: equal omega in every cell that has both, the larger index first
    r = ref("twins")
    f, o = r["frame"].astype(int), r["omega"]
    both = (f == 1).any(axis=2) & (f == 2).any(axis=2)
    s1, s2 = np.argmax(f == 1, axis=2), np.argmax(f == 2, axis=2)
    assert both.sum() > 50 and (s2[both] + 1 == s1[both]).all()
    assert (np.take_along_axis(o, s1[..., None], 2)[..., 0][both] == np.take_along_axis(o, s2[..., None], 2)[..., 0][both]).all()
    # an argmin tie between two filled slots
    S = np.where(r["frame"] > 0, r["S"], sc.INF)
    srt = np.sort(S, axis=2)
    assert ((srt[..., 0] == srt[..., 1]) & (srt[..., 1] < sc.INF)).sum() > 10
    # a label that is a candidate in p and not in its neighbour q
    r = ref("crafted3")
    lab = np.take_along_axis(r["frame"], r["slot"][..., None], 2)[..., 0]
    miss = (lab[:, :-1] > 0) & (r["frame"][:, 1:, 0] > 0) & ~(r["frame"][:, 1:] == lab[:, :-1, None]).any(axis=2)
    assert miss.any()
    # the energy fallback
    r = ref("twins_differ")
    assert r["report"]["fallback"] == 1 and r["report"]["energy_after"] > r["report"]["energy_before"] and not r["cells"].any()
    # levels 2 and 5, a skipped frame
    imgs, h9s, p, r = sp.reference(oracle, "level5")
    assert p["level"] == 5 and h9s[3, 8] == 0 and r["maps"][3] is None and not (r["frame"] == 4).any() and r["cells"].shape == (4, 5)
    assert sp.reference(oracle, "crafted2")[2]["level"] == 2
    # the record cases: one frame on both sides of an empty cell ...
    f = sp.record_reference("records_holes")[0]
    m = (f > 0).sum(axis=2)
    assert any(m[y, x] == 0 and np.intersect1d(f[y, x - 1][f[y, x - 1] > 0], f[y, x + 1][f[y, x + 1] > 0]).size for y in range(7) for x in range(1, 8))
    # ... and a path whose costs, were the minimum not subtracted at every step, would leave the 16 bits the sums are kept in
    f, o, g, p = sp.record_reference("records_dear")[:4]
    D = p["data_weight"] * (o[..., :1].astype(np.int64) - o) * (f > 0)
    grown = sc._sweep(f, g, D, p, "nosub")
    assert grown.max() > 65535 and sc._sweep(f, g, D, p, None).max() <= 12479


def test_each_mutation_is_seen(oracle):
    seen = {mu: [] for mu in sc.MUTATIONS}
    for name in sorted(sp.CASES):
        imgs, h9s, p, r = sp.reference(oracle, name)
        for mu in sc.MUTATIONS:
            if (sc.labels(r["frame"], r["omega"], r["gray"], p, mu)[0] != r["cells"]).any():
                seen[mu].append(name)
    for name in sorted(sp.RECORD_CASES):
        f, o, g, p, cells = sp.record_reference(name)[:5]
        for mu in sc.MUTATIONS:
            if (sc.labels(f, o, g, p, mu)[0] != cells).any():
                seen[mu].append(name)
    print(seen)
    for mu in sc.MUTATIONS:
        assert seen[mu], mu
    # on surveys the path restart and the subtraction change no label (frames are convex; the sums stay small): only the record cases see them
    assert seen["restart"] == ["records_holes"] and "records_dear" in seen["nosub"]


# ---- the host twin and the public surface ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def im():
    from imagemosaicing_amd import build
    build.build()
    import imagemosaicing_amd
    return imagemosaicing_amd


def _records(im, frame, omega, gray):
    rec = np.zeros(frame.shape[:2], im.SEAM_CELL)
    rec["frame"], rec["omega"], rec["gray"] = frame, omega, gray
    assert np.array_equal(rec.view(np.uint8).reshape(frame.shape[:2] + (32,)), sc.record_bytes(frame, omega, gray))
    return rec


@pytest.mark.parametrize("name", sorted(sp.CASES) + sorted(sp.RECORD_CASES))
def test_host_twin_equals_restatement(im, oracle, name):
    if name in sp.CASES:
        imgs, h9s, p, r = sp.reference(oracle, name)
        frame, omega, gray, cells, report = r["frame"], r["omega"], r["gray"], r["cells"], r["report"]
    else:
        frame, omega, gray, p, cells, report, _ = sp.record_reference(name)
    kw = {k: v for k, v in p.items()}
    got, rep = im.seam_labels_host(_records(im, frame, omega, gray), **kw)
    assert np.array_equal(got, cells) and rep == report, (rep, report)


def test_host_twin_refuses_every_range_error(im):
    rec = np.zeros((2, 3), im.SEAM_CELL)
    for k, (lo, hi) in sc.RANGES.items():
        for v in ([lo - 1] if hi is None else [lo - 1, hi + 1]):
            with pytest.raises(im.Mi355Error) as e:
                im.seam_labels_host(rec, **{k: v})
            assert e.value.code == -1, (k, v)
    cells, rep = im.seam_labels_host(rec)
    assert not cells.any() and rep == dict(energy_before=0, energy_after=0, changed=0, fallback=0)


def test_new_symbols_are_exported_and_declared(im):
    L = im.load_library()
    hdr = open(os.path.join(ROOT, "include", "mi355_mosaic.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    for name in ("SeamCutParams", "SeamReport", "SEAM_CELL", "seamcut_params", "seam_grid", "seam_labels_host"):
        assert hasattr(im, name), name
    for name in ("SeamCandidatesDev", "SeamLabelsDev", "SeamCellsDev", "MosaicSeamCutDev", "MosaicSeamCut", "MosaicSeamCutInto", "SeamCutCover"):
        assert hasattr(im.Context, name), name
    p = im.seamcut_params()
    assert C.sizeof(p) == 32 and im.SEAM_CELL.itemsize == 32 and C.sizeof(im.SeamReport) == 24
    assert {k: getattr(p, k) for k in sc.DEFAULTS} == sc.DEFAULTS and p.reserved == 0


def test_structs_in_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "mi355_mosaic.h"\n'
                   'typedef char params_32[sizeof(mi355_seamcut_params) == 32 ? 1 : -1];\n'
                   'typedef char cell_32[sizeof(mi355_seam_cell) == 32 && offsetof(mi355_seam_cell, omega) == 16 && offsetof(mi355_seam_cell, gray) == 24 ? 1 : -1];\n'
                   'typedef char report_24[sizeof(mi355_seam_report) == 24 ? 1 : -1];\n'
                   'typedef char slots_8[MI355_SEAMCUT_MAX_DEPTH == 8 ? 1 : -1];\n'
                   'int main(void) { mi355_seamcut_params p; p.level = 3; return p.level; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_binding_raises_without_a_context(im):
    """a context that does not exist: every new method reaches the C ABI and fails there, loudly (no CPU path answers instead)"""
    ctx = im.Context.__new__(im.Context)
    ctx.L, ctx._h, ctx.device = im.load_library(), C.c_void_p(), 0
    img = np.zeros((32, 32, 3), np.uint8)
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    h9s[1, 2] = 10
    for call in (lambda: ctx.MosaicSeamCut([img, img], h9s),
                 lambda: ctx.MosaicSeamCutDev([0, 0], [32, 32], [32, 32], [96, 96], h9s, 0, 42, 32, 128, d_count=0),
                 lambda: ctx.MosaicSeamCutInto([img, img], None, h9s),
                 lambda: ctx.SeamCandidatesDev([0, 0], [32, 32], [32, 32], [96, 96], h9s, 0, 6, 4),
                 lambda: ctx.SeamLabelsDev(0, 6, 4, 0),
                 lambda: ctx.SeamCellsDev([0, 0], [32, 32], [32, 32], [96, 96], h9s, 0, 6, 4),
                 lambda: ctx.SeamCutCover([32, 32], [32, 32], h9s, 0)):
        with pytest.raises(im.Mi355Error) as e:
            call()
        assert e.value.code == -1

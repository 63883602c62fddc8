"""CPU: the edge cases of the optimised seamlines (tests/seamcut_patterns.py: WAVE_CASES, REM_CASES, RECORD_EDGE_CASES, and the cases of
tests/render_patterns.py at seamcut_patterns.EDGE_SETTINGS) hold what they are for, on the numpy restatement alone (tests/seamcut_ref.py);
tests/test_gpu_seamcut_edges.py compares the HIP kernels with the same restatement on the same cases.

  * wave*: more covering frames at one probe than a wave has lanes, so that a lane of seam_candidates_kernel holds 2, 3 and more than 8 keys; a
    cell whose eight winners come out of one lane, and cells whose winners come out of seven lanes or more;
  * rem_*: per level, the probe of the partial cell is clamped to the canvas and is not, in x and in y;
  * the cases of tests/render_patterns.py: what the seamcut stages see on them (filled slots, partial cells, changed cells) is recorded and
    the few things the GPU tests rely on are asserted;
  * the record cases with up to 8 filled slots, and the host twin on all of the new records.
"""
import numpy as np
import pytest

from tests import render_patterns as rp
from tests import seamcut_patterns as sp
from tests import seamcut_ref as sc
from tests.test_seamcut_ref import _m, _records, im  # noqa: F401  (im: the module-scope fixture that builds the library)

RENDER_CASES = rp.cases()
LEVELS = tuple(l for l, _, _ in sp.EDGE_SETTINGS)


def _lane_census(imgs, r, p):
    """(the largest number of frames that cover one probe and go to one lane, per cell with 8 winners the number of lanes they come from)"""
    n = len(imgs)
    ch, cw = r["owner"].shape
    assert max(cw, ch) <= 256 and all(m is not None for m in r["maps"])     # one list block, no frame skipped: lane_of holds
    s = 1 << p["level"]
    gh, gw = r["cells"].shape
    py = np.minimum(np.arange(gh) * s + s // 2, ch - 1); px = np.minimum(np.arange(gw) * s + s // 2, cw - 1)
    lanes = np.array([sp.lane_of(n, k) for k in range(n)])
    at_probe = np.stack([m[1][np.ix_(py, px)] for m in r["maps"]])           # [n, gh, gw]
    share = max(int(at_probe[lanes == l].sum(axis=0).max()) for l in range(sp.WAVE))
    full = (r["frame"] > 0).all(axis=2)
    from_lanes = {(int(y), int(x)): len(set(lanes[r["frame"][y, x].astype(int) - 1].tolist())) for y, x in np.argwhere(full)}
    return share, from_lanes


@pytest.mark.parametrize("name,share", [("wave65", 2), ("wave130", 3), ("wave600", 9), ("wave600_one_lane", 9)])
def test_wave_cases_fill_the_lanes(oracle, name, share):
    imgs, h9s, p, r = sp.reference(oracle, name)
    assert p["depth"] == 8 and h9s[:, [0, 4, 8]].min() == 1 and np.array_equal(h9s[:, [2, 5]], np.round(h9s[:, [2, 5]]))
    assert 0 <= h9s[:, [2, 5]].min() and h9s[:, [2, 5]].max() <= 8
    for axis in (2, 5):                                                     # not monotone in k: keys reach a lane in mixed order
        d = np.diff(h9s[:, axis])
        assert (d > 0).any() and (d < 0).any()
    got, from_lanes = _lane_census(imgs, r, p)
    print("%s: %d frames, canvas %s, at most %d covering frames of one lane at a probe; lanes of the 8 winners per cell %s"
          % (name, len(imgs), r["owner"].shape, got, sorted(from_lanes.values())))
    assert got == share if name == "wave65" else got >= share
    assert from_lanes and max(from_lanes.values()) >= 7                     # the pop of one lane's head leaves the other lanes' heads alone
    if name == "wave130":
        # the first six winners of one cell come three each out of lanes 0 and 1, and neither lane was handed its three in sorted order
        c = sp.STACK_PROBE >> p["level"]
        assert tuple(r["frame"][c, c, :6].astype(int) - 1) == sp.STACK_ORDER and len(set(r["omega"][c, c, :6].tolist())) == 3
        for lane in (0, 1):
            arrive = [sp.STACK_ORDER.index(k) for k in sorted((k for k in sp.STACK if sp.lane_of(len(imgs), k) == lane), reverse=True)]
            assert len(arrive) == 3 and arrive != sorted(arrive) and arrive != sorted(arrive, reverse=True), (lane, arrive)
    if name == "wave600_one_lane":
        c = sp.ONE_LANE_PROBE >> p["level"]
        assert from_lanes[(c, c)] == 1 and sp.lane_of(len(imgs), int(r["frame"][c, c, 0]) - 1) == sp.ONE_LANE
        assert len(set(r["omega"][c, c].tolist())) == 1                     # equal omega: the index alone orders them
        assert (np.diff(r["frame"][c, c].astype(int)) < 0).all()
    # a smaller depth is a prefix of the records
    for depth in (1, 4):
        f, o, g = sc.candidates(r["maps"], r["wmaps"], p["level"], depth)
        q, rs = sp.shallower(r, p, depth)
        assert np.array_equal(f, rs["frame"]) and np.array_equal(o, rs["omega"]) and np.array_equal(g, rs["gray"]) and q["depth"] == depth


def _clamped(size, s):
    """per cell along an axis of `size` pixels: the probe x0 + s / 2 lies beyond the canvas and is clamped to size - 1"""
    return np.arange((size + s - 1) // s) * s + s // 2 > size - 1


@pytest.mark.parametrize("level", (2, 3, 4, 5))
def test_rem_cases_clamp_the_probe_and_do_not(oracle, level):
    s = 1 << level
    seen = {"x": set(), "y": set()}
    names = ["rem_L%d_%dx%d%s" % (level, rx, ry, t) for rx, ry in sp.rem_pairs(level) for t in ("", "_turned")]
    assert sorted(names) == sorted(k for k in sp.REM_CASES if k.startswith("rem_L%d_" % level))
    for name in names:
        imgs, h9s, p, r = sp.reference(oracle, name)
        ch, cw = r["owner"].shape
        rx, ry = cw % s, ch % s
        assert p["level"] == level and name.startswith("rem_L%d_%dx%d" % (level, rx, ry)) and len(imgs) == 2
        m = _m(r)
        cx, cy = _clamped(cw, s), _clamped(ch, s)
        # the partial cell's probe is clamped exactly for a remainder of at most s / 2; every whole cell's probe is not
        assert cx[-1] == (rx <= s // 2) and cy[-1] == (ry <= s // 2) and not cx[:-1].any() and not cy[:-1].any() and len(cx) > 1 and len(cy) > 1
        assert cx[-1] != cy[-1]                                             # within a case one axis is clamped, the other is not
        if name.endswith("_turned"):
            # both frames give the canvas's last column and row samples: every partial cell has a candidate, the corner cell both
            assert m[-1, -1] == 2 and (m[:, -1] >= 1).all() and (m[-1, :] >= 1).all() and m[0, 0] == 1 and m[1, 1] >= 1
        else:
            # no frame gives the canvas's last column or row a sample: a partial cell has candidates exactly where its probe lies before them
            for line, size, rem in ((m[:-1, -1], cw, rx), (m[-1, :-1], ch, ry)):
                probe = min((size // s) * s + s // 2, size - 1)
                assert (line >= 1).all() if probe < size - 1 else not line.any(), (name, line, probe)
            assert m[0, 0] == 1 and (m[1, 1] == 2 or level == 2)
        seen["x"].add((rx, bool(cx[-1]))); seen["y"].add((ry, bool(cy[-1])))
    want = {(1, True), (s // 2, True), (s // 2 + 1, False), (s - 1, False)}
    assert seen["x"] == want and seen["y"] == want                          # clamped and not clamped, in both axes, at this level


def test_render_pattern_cases_as_the_seamcut_stages_see_them(oracle):
    """a record of what the cases of tests/render_patterns.py give stages 1 and 2, and the assertions the GPU tests lean on"""
    seen = {}
    for case in RENDER_CASES:
        n_live = sum(m is not None for m in rp.restate(oracle, case).maps)
        for level in LEVELS:
            p, r = sp.edge_reference(oracle, case, level)
            s = 1 << level
            ch, cw = r["owner"].shape
            seen[(case.tag, level)] = dict(m=int(_m(r).max()), partial=bool(cw % s or ch % s), narrow=cw < s, changed=r["report"]["changed"],
                                           fallback=r["report"]["fallback"])
            assert _m(r).max() <= min(p["depth"], n_live)
            assert set(np.unique(r["frame"]).tolist()) <= {0} | {k + 1 for k, m in enumerate(r["maps"]) if m is not None}     # a skipped frame is nobody's candidate
    for key in sorted(seen):
        print(key, seen[key])
    tags = {c.tag for c in RENDER_CASES}
    assert len(RENDER_CASES) == 36 and {"turns", "forty", "scaled_matrices", "m8_zero_ends", "rank_deficient", "straddle_overlap", "canvas_w1", "canvas_w3"} <= tags
    # more than four filled slots on the 40 frames, at both depth-8 levels; depth 4 caps level 3
    assert seen[("forty", 2)]["m"] == 8 and seen[("forty", 5)]["m"] == 8 and seen[("forty", 3)]["m"] == 4
    # partial cells at every level, canvases narrower than a lane's four pixels and than one cell
    for level in LEVELS:
        assert sum(v["partial"] for (t, l), v in seen.items() if l == level) >= 30
        assert seen[("canvas_w1", level)]["narrow"] and seen[("canvas_w3", level)]["narrow"]
    # cells on both sides of the list-block boundary at level 5: the 291 x 281 canvas has 10 x 9 cells, the ninth column and row start at 256
    p, r = sp.edge_reference(oracle, next(c for c in RENDER_CASES if c.tag == "straddle_overlap"), 5)
    assert r["cells"].shape == (9, 10) and (_m(r)[8, 8:] >= 2).any() and (_m(r)[7, :8] >= 1).all()
    # the label stage moves cells on the turned and mirrored frames and on the scaled matrices.  On the forty it moves none at any level (at
    # level 2 its labelling costs more than the seamline's and the fallback returns that); there stage 3 is exercised by the random cell
    # maps of tests/test_gpu_seamcut_edges.py alone (test_random_cell_maps_name_every_kind_of_frame below)
    assert any(seen[("turns", l)]["changed"] > 0 for l in LEVELS) and any(seen[("scaled_matrices", l)]["changed"] > 0 for l in LEVELS)
    assert seen[("forty", 2)]["fallback"] == 1 and not any(seen[("forty", l)]["changed"] for l in LEVELS)


def test_random_cell_maps_name_every_kind_of_frame(oracle):
    """the random cell maps of the GPU tests name, on some case, a skipped frame, a frame without an inverse, a frame that does not touch
    the cell and a frame that covers part of it; where they name a frame that gives the cell samples the render follows them"""
    kinds = dict(skipped=0, no_inverse=0, away=0, part=0, whole=0)
    for case in RENDER_CASES:
        R = rp.restate(oracle, case)
        n = len(case.imgs)
        for level in LEVELS:
            p, r = sp.edge_reference(oracle, case, level)
            gh, gw = r["cells"].shape
            s = 1 << level
            for seed in (0, 1):
                cells = sp.random_cells(n, gw, gh, 1000 * level + seed)
                assert cells.max() <= n
                for (y, x), k in np.ndenumerate(cells):
                    if k == 0:
                        continue
                    if R.maps[k - 1] is None:
                        kinds["skipped"] += 1
                        continue
                    cov = R.maps[k - 1][1][y * s:(y + 1) * s, x * s:(x + 1) * s]
                    if not R.maps[k - 1][1].any():
                        kinds["no_inverse"] += 1
                    elif not cov.any():
                        kinds["away"] += 1
                    else:
                        kinds["whole" if cov.all() else "part"] += 1
    print(kinds)
    assert all(v > 0 for v in kinds.values()), kinds
    # the render follows such a map: not the seamline owner map, and the named frame wherever it gives a sample
    case = next(c for c in RENDER_CASES if c.tag == "turns")
    R = rp.restate(oracle, case)
    p, r = sp.edge_reference(oracle, case, 2)
    cells = sp.random_cells(len(case.imgs), r["cells"].shape[1], r["cells"].shape[0], 2000)
    out, owner, count = sc.render(R.maps, R.weights(0), cells, 2)
    assert (owner != R.seamline(0)[1]).any() and np.array_equal(count, R.seamline(0)[2])
    beyond = sc.render(R.maps, R.weights(0), np.full_like(cells, len(case.imgs) + 1), 2)
    assert np.array_equal(beyond[0], R.seamline(0)[0]) and np.array_equal(beyond[1], R.seamline(0)[1])


def test_record_cases_fill_eight_slots_and_see_the_mutations():
    seen = {mu: [] for mu in sc.MUTATIONS}
    filled = set()
    for name in sorted(sp.RECORD_EDGE_CASES):
        f, o, g, p, cells, report, slot = sp.record_reference(name)
        m = (f > 0).sum(axis=2)
        filled |= set(m.ravel().tolist())
        fi = f.astype(int)
        for y, x in np.ndindex(m.shape):                                    # what the header defines the stage on: distinct frames, omega descending
            k = int(m[y, x])
            assert len(set(fi[y, x, :k].tolist())) == k and not fi[y, x, k:].any() and (np.diff(o[y, x, :k].astype(int)) <= 0).all() and (o[y, x, :k] > 0).all()
        for mu in sc.MUTATIONS:
            if (sc.labels(f, o, g, p, mu)[0] != cells).any():
                seen[mu].append(name)
        # the picked slot reaches beyond the first four somewhere
        print(name, "filled", sorted(set(m.ravel().tolist())), "largest picked slot", int(slot.max()), report)
    print(seen)
    assert {5, 6, 7, 8} <= filled and 0 in filled
    for mu in ("tie", "miss", "dir"):
        assert seen[mu], mu
    f = sp.record_reference("records8_ids")[0]
    assert {65535, 65534, 32768, 256, 255} <= set(np.unique(f).tolist())
    assert {sp.record_reference(n)[0].shape[:2] for n in sp.RECORD_EDGE_CASES} >= {(5, 70), (70, 5), (9, 33), (7, 9)}
    p = sp.record_reference("records8_dear")[3]
    assert (p["depth"], p["data_weight"], p["diff_weight"], p["seam_penalty"], p["miss_cost"]) == (8, 16, 16, 255, 255)
    assert (sp.record_reference("records8_dear")[0][..., 0] > 0).all() and sp.record_reference("records8_holes_free")[3]["miss_cost"] == 0
    assert max(int(sp.record_reference(n)[6].max()) for n in sp.RECORD_EDGE_CASES) >= 5


@pytest.mark.parametrize("name", sorted(sp.SURVEY_EDGE_CASES) + sorted(sp.RECORD_EDGE_CASES))
def test_host_twin_equals_restatement_on_the_edge_cases(im, oracle, name):
    if name in sp.SURVEY_EDGE_CASES:
        imgs, h9s, p, r = sp.reference(oracle, name)
        sets = [(r["frame"], r["omega"], r["gray"], p, r["cells"], r["report"])]
        if name in sp.WAVE_CASES:
            for depth in (1, 4):
                q, rs = sp.shallower(r, p, depth)
                sets.append((rs["frame"], rs["omega"], rs["gray"], q, rs["cells"], rs["report"]))
    else:
        sets = [sp.record_reference(name)[:6]]
    for frame, omega, gray, p, cells, report in sets:
        got, rep = im.seam_labels_host(_records(im, frame, omega, gray), **p)
        assert np.array_equal(got, cells) and rep == report, (rep, report)


@pytest.mark.parametrize("level", LEVELS)
def test_host_twin_equals_restatement_on_the_render_pattern_cases(im, oracle, level):
    for case in RENDER_CASES:
        p, r = sp.edge_reference(oracle, case, level)
        got, rep = im.seam_labels_host(_records(im, r["frame"], r["omega"], r["gray"]), **p)
        assert np.array_equal(got, r["cells"]) and rep == r["report"], (case.tag, rep, r["report"])

"""GPU: the pair stage (csrc/match.hip: match -> sort -> ratio filter -> grid select; csrc/ransac.hip: device-built draw tables, RANSAC, accept)
against the oracle, bit for bit, at parameter and keypoint edges.  tests/test_match_patterns_oracle.py shows on the oracle alone that the inputs of
tests/match_patterns.py hold what they are for, and that the composed oracle (oracle_pair_record, which takes the parameters) equals the oracle's
own entry points.  Every comparison is exact; floats are compared by bit pattern.

mi355_params is fixed when a context is created, so every parameter set is a context of its own: five that run pairs, one more with min_inliers 10
at the default 1000 samples (the inlier-count cases are exact at 1000 samples, not at the 77 of the min_inliers / sample_times context), and three
that only show the refusal and never launch anything.  Each is closed where it was made."""
import contextlib

import numpy as np
import pytest

from tests import match_patterns as mp
from tests import oracle_lib as ol
from tests.golden_util import bits

pytestmark = pytest.mark.gpu
SEED = 3


@pytest.fixture(scope="module")
def orc():
    return ol.load_oracle_fast()


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _context(**params):
    """a context with mi355_params fields changed; `gx` / `gy` as oracle_pair_record names them"""
    import imagemosaicing_amd as im
    p = im.default_params()
    for k, v in params.items():
        setattr(p, {"gx": "grid_x", "gy": "grid_y"}.get(k, k), v)
    c = im.Context(0, p)
    try:
        yield c
    finally:
        c.close()


def _set(c, img_id, xy, d, w, h):
    c.SetFeatures(img_id, mp.keypoints(xy), np.ascontiguousarray(d, np.uint8).astype(np.float32).reshape(-1, 128), w, h)


def _set_pair(c, k, p):
    _set(c, 2 * k, p["xy1"], p["d1"], p["w"], p["h"])
    _set(c, 2 * k + 1, p["xy2"], p["d2"], p["w"], p["h"])
    return (2 * k, 2 * k + 1)


def _same_record(r, o, tag):
    """a whole mi355_pair_result against oracle_pair_record's: the counts, the inlier lists (zero beyond n_in) and, for an accepted pair, H and ok;
    a rejected record keeps its real n_in and inlier lists, H is all zero and ok is 0 (the closing refinement is skipped: mi355_mosaic.h)"""
    got = (int(r["n_selected"]), int(r["n_in"]), int(r["accepted"]))
    assert got == (o["n_selected"], o["n_in"], o["accepted"]), (tag, got, (o["n_selected"], o["n_in"], o["accepted"]))
    n = o["n_in"]
    assert np.array_equal(r["a"][:n], o["a"]) and np.array_equal(r["b"][:n], o["b"]), (tag, "inlier lists")
    assert not np.frombuffer(r["a"][n:].tobytes(), np.uint8).any() and not np.frombuffer(r["b"][n:].tobytes(), np.uint8).any(), (tag, "beyond n_in")
    if o["accepted"]:
        assert int(r["ok"]) == o["ok"] == 1 and np.array_equal(bits(r["H"]), bits(o["H"])), (tag, "H", r["H"], o["H"])
    else:
        assert int(r["ok"]) == 0 and not bits(r["H"]).any(), (tag, "rejected record", int(r["ok"]), r["H"])


def _run_pairs(c, orc, pairs, seed=SEED, tag="", **params):
    """the pairs in ONE MatchPairs call against the composed oracle under the same parameters"""
    ids = [_set_pair(c, k, p) for k, p in enumerate(pairs)]
    want = ol.parallel_map(lambda p: mp.record_of(orc, p, mp.DIST, seed, **params), pairs)
    res = c.MatchPairs(ids, mp.DIST, seed)
    for k, (r, o, ij) in enumerate(zip(res, want, ids)):
        assert (int(r["i"]), int(r["j"])) == ij
        _same_record(r, o, (tag, k))
    c.DropFeatures(-1)
    return res, want


def _small_pairs(s):
    """four small pairs (M <= 1400): related, mostly outliers, a train image over 2048 keypoints (the large-pair path), unrelated"""
    a, b, c = mp.make_pair(s, 1400, 1400, outliers=0.3), mp.make_pair(s + 1, 500, 900, outliers=0.75), mp.make_pair(s + 2, 700, 2100)
    return [a, b, c, dict(a, xy2=b["xy2"], d2=b["d2"])]


# ---- stand-alone SelectMatchPairs -------------------------------------------------------------------------------------------------------------
def test_select_cell_edges_and_cell_filling(ctx, orc):
    """every cell-edge pattern (clamped cells and far-outside points included) on grids 3x3, 1x1, 5x5, 8x8, 7x9 and 1x64, every cell-filling
    pattern.  nMatch > 400 never reaches the kernel: mi355_select_grid refuses it (and MatchPairs a max_selected > 400), so the walk's cut at
    MI355_MAX_SELECTED entries cannot be taken -- per_grid * nGrids <= nMatch <= 400; the refusal is what is pinned here, and nMatch = 400 on 5x5
    (exactly 400 selected) is the largest list"""
    import imagemosaicing_amd as im
    pats = mp.edge_select_patterns() + mp.fill_patterns()
    assert {(p["gx"], p["gy"]) for p in pats} >= set(mp.EDGE_GRIDS)
    longest = 0
    for p in pats:
        args = (p["matches"], p["kp1"], p["kp2"], p["nMatch"], p["w"], p["h"], p["gx"], p["gy"])
        if p["nMatch"] > 400:
            with pytest.raises(im.Mi355Error, match="nMatch"):
                ctx.SelectMatchPairs(*args)
            continue
        o1, o2 = orc.select(*args)
        a1, a2 = ctx.SelectMatchPairs(*args)
        assert len(a1) == len(o1), (p["tag"], len(a1), len(o1))
        assert np.array_equal(a1, o1) and np.array_equal(a2, o2), (p["tag"], int((a1["id"] != o1["id"]).argmax()))
        longest = max(longest, len(a1))
    assert longest == 400 and any(p["nMatch"] > 400 for p in pats)
    p = pats[0]
    for (gx, gy, w, h) in [(9, 8, p["w"], p["h"]), (0, 3, p["w"], p["h"]), (3, 0, p["w"], p["h"]), (3, 3, 2, p["h"]), (3, 3, p["w"], 2)]:
        with pytest.raises(im.Mi355Error):
            ctx.SelectMatchPairs(p["matches"], p["kp1"], p["kp2"], p["nMatch"], w, h, gx, gy)


# ---- MatchPairs ---------------------------------------------------------------------------------------------------------------------------------
def test_match_pairs_keypoints_on_cell_edges(ctx, orc):
    """default parameters, 4001x2999: the edge points are the first queries of the sorted list (exact descriptor copies)"""
    res, want = _run_pairs(ctx, orc, [mp.edge_pair()], seed=7, tag="edge_pair")
    assert want[0]["n_selected"] == 396 and want[0]["accepted"] == 1


def test_match_pairs_guard_image_smaller_than_grid(ctx, orc):
    """an image i narrower or lower than the grid is refused (stepX = 0: the cell would come from x / 0); a 3x3 image stays legal"""
    import imagemosaicing_amd as im
    p = mp.make_pair(41, 60, 80, w=3, h=3)
    p["xy1"] = mp.edge_points(3, 3)[:60].copy()
    _run_pairs(ctx, orc, [p], tag="3x3 image")
    for (w, h) in [(2, 3), (3, 2), (1, 1)]:
        _set(ctx, 0, p["xy1"], p["d1"], w, h)
        _set(ctx, 1, p["xy2"], p["d2"], 3, 3)
        with pytest.raises(im.Mi355Error, match="grid"):
            ctx.MatchPairs([(1, 0), (0, 1)], mp.DIST, SEED)
        r = ctx.MatchPairs([(1, 0)], mp.DIST, SEED)        # the train image may be as small as it likes: the cell comes from image i
        assert int(r[0]["n_selected"]) == mp.record_of(orc, dict(p, xy1=p["xy2"], d1=p["d2"], xy2=p["xy1"], d2=p["d1"]), mp.DIST, SEED)["n_selected"]
    ctx.DropFeatures(-1)


PARAM_SETS = {"grid_8x8_max_384": dict(gx=8, gy=8, max_selected=384), "fraction_0.1_max_100": dict(select_fraction=0.1, max_selected=100),
              "min_inliers_10_samples_77": dict(min_inliers=10, sample_times=77)}


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_parameter_context(orc, name):
    params = PARAM_SETS[name]
    with _context(**params) as c:
        res, want = _run_pairs(c, orc, _small_pairs(200 + 10 * list(PARAM_SETS).index(name)), tag=name, **params)
    assert any(o["accepted"] for o in want) and not all(o["accepted"] for o in want)
    if name == "grid_8x8_max_384":
        assert want[0]["n_selected"] == 384
    if name == "fraction_0.1_max_100":
        assert [o["n_selected"] for o in want[:3]] == [99, 45, 63]                 # 9 * int(min(100, 0.1 M) / 9)


def test_refused_parameters():
    """a grid over 64 cells, grid_x < 1 and max_selected > 400: MI355_ERR_ARG from MatchPairs, nothing launched"""
    import imagemosaicing_amd as im
    p = mp.make_pair(51, 50, 60)
    for bad in (dict(gx=9, gy=8), dict(gx=0), dict(max_selected=401)):
        with _context(**bad) as c:
            ids = _set_pair(c, 0, p)
            with pytest.raises(im.Mi355Error):
                c.MatchPairs([ids], mp.DIST, SEED)


def test_grid_1x1_context_and_n_selected_sweep(orc):
    """grid 1x1: n_selected = int(min(400, 0.3 M)).  All twenty pairs of the sweep in one call: the tables draw_tables_kernel built for n = 4 .. 400
    give the oracle's records, and the same selected points through Ransac2D -- whose tables are built on the host -- give the same inliers and H"""
    with _context(gx=1, gy=1) as c:
        _run_pairs(c, orc, _small_pairs(300), tag="1x1", gx=1, gy=1)
        res, want = _run_pairs(c, orc, mp.sweep_pairs(), tag="sweep", gx=1, gy=1)
        assert [int(r["n_selected"]) for r in res] == list(mp.SWEEP_N)
        for n, r, o in zip(mp.SWEEP_N, res, want):
            ok, i1, i2, H = c.Ransac2D(o["sel1"], o["sel2"], mp.DIST, 1000, SEED)
            assert ok == o["ok"] and np.array_equal(i1, o["a"]) and np.array_equal(i2, o["b"]), n
            assert np.array_equal(i1, r["a"][:len(i1)]) and len(i1) == int(r["n_in"]), n
            if len(i1) >= 4:
                assert np.array_equal(bits(H), bits(o["H"])), n
            if int(r["accepted"]):
                assert np.array_equal(bits(H), bits(r["H"])), n


def test_six_seeds_through_four_table_slots(ctx, orc):
    """four slots hold the draw tables of the latest seeds: six seeds in turn, twice over, then the first again -- every table set is evicted and
    rebuilt -- and every record is the oracle's for its seed"""
    p = mp.make_pair(31, 600, 700, outliers=0.5, noise=1.5)      # 1.5 px of noise: the inlier set depends on the winning draw
    ids = _set_pair(ctx, 0, p)
    seeds = [11, 12, 13, 14, 15, 16]
    want = {s: mp.record_of(orc, p, mp.DIST, s) for s in seeds}
    assert len({o["H"].tobytes() for o in want.values()}) == len(seeds) and all(o["accepted"] for o in want.values())
    for s in seeds + seeds + seeds[:1]:
        _same_record(ctx.MatchPairs([ids], mp.DIST, s)[0], want[s], ("seed", s))
    ctx.DropFeatures(-1)


def _threshold(c, orc, cases, min_inliers):
    pairs = [mp.inlier_case(K, ds) for K, ds in cases.items()]
    ids = [_set_pair(c, k, p) for k, p in enumerate(pairs)]
    want = [mp.record_of(orc, p, mp.DIST, mp.INLIER_SEED, min_inliers=min_inliers) for p in pairs]
    assert [o["n_in"] for o in want] == list(cases) and [o["accepted"] for o in want] == [int(K > min_inliers) for K in cases]
    recs = []
    try:
        for S in (0, 2):
            c.set_option("ransac_split", S)
            res = c.MatchPairs(ids, mp.DIST, mp.INLIER_SEED)
            for K, r, o in zip(cases, res, want):
                _same_record(r, o, ("K", K, "split", S))
            recs.append(res.tobytes())
    finally:
        c.set_option("ransac_split", -1)
        c.DropFeatures(-1)
    assert recs[0] == recs[1]


def test_accept_threshold(ctx, orc):
    """n_in == min_inliers is rejected, min_inliers + 1 accepted; a rejected record carries its real n_in and inlier lists, H = 0 and ok = 0, in
    both forms of the RANSAC (one workgroup per pair, split)"""
    _threshold(ctx, orc, mp.INLIER_CASES_30, 30)
    with _context(min_inliers=10) as c:
        _threshold(c, orc, mp.INLIER_CASES_10, 10)


def test_ratio_context_and_ratio_corners(orc):
    R = mp.ratio_pairs()
    with _context(ratio=0.8) as c:
        _run_pairs(c, orc, _small_pairs(400), tag="ratio", ratio=0.8)
        names = ["duplicated_train_rows", "one_train_row", "no_train_row", "duplicate_across_chunks"]
        res, want = _run_pairs(c, orc, [R[n] for n in names], tag="ratio corners", ratio=0.8)
    by = dict(zip(names, want))
    assert by["one_train_row"]["n_kept"] == 200 and by["no_train_row"]["n_selected"] == 0
    for n in ("duplicated_train_rows", "duplicate_across_chunks"):
        assert not np.isin(R[n]["dropped"], by[n]["kept"][:, 0]).any() and by[n]["n_selected"] > 0


# ---- descriptor content -------------------------------------------------------------------------------------------------------------------------
def test_bf_match_descriptor_content(ctx, orc):
    """rows that look like padding (all 128) up to the last valid train row, all 0 against all 255, all rows equal, duplicated train rows (also
    across the 2048-row chunk boundary), one train row, none"""
    for name, (d1, d2) in mp.content_patterns().items():
        _set(ctx, 100, np.zeros((len(d1), 2)), d1, 1000, 750)
        _set(ctx, 101, np.zeros((len(d2), 2)), d2, 1000, 750)
        m, g1, g2 = ctx.BFMatch(100, 101, sorted_=False)
        if len(d2) == 0:
            assert len(m) == 0, name
            continue
        idx, b1, b2 = orc.bf_match(d1, d2)
        assert np.array_equal(m["trainIdx"], idx) and np.array_equal(g1, b1) and np.array_equal(g2, b2), name
        ms, s1, s2 = ctx.BFMatch(100, 101, sorted_=True)
        want = orc.sort_matches(idx, b1)
        assert np.array_equal(np.stack([ms["queryIdx"], ms["trainIdx"]], 1), want) and np.array_equal(s1, b1[want[:, 0]]) and np.array_equal(s2, b2[want[:, 0]]), name
    ctx.DropFeatures(-1)


def test_set_features_clamps_and_rounds(ctx):
    """desc_f32_to_u8_kernel: floor(clip(v, 0, 255) + 0.5)"""
    desc = np.zeros((3, 128), np.float32)
    desc[0, :10], desc[1, 118:], desc[2, 5:125] = mp.FLOAT_DESC, mp.FLOAT_DESC[::-1], np.tile(mp.FLOAT_DESC, 12)
    ctx.SetFeatures(7, mp.keypoints(np.zeros((3, 2))), desc, 640, 480)
    kp, got = ctx.GetFeatures(7)
    assert np.array_equal(got, mp.float_desc_expected(desc).astype(np.float32))
    ctx.DropFeatures(7)


# ---- run splitting ------------------------------------------------------------------------------------------------------------------------------
def test_large_pair_runs_split_by_sub_pair_count(ctx, orc):
    """option big_subpairs_max = 2: a 2049 x 300 pair is two sub-pairs, a 2049 x 2049 pair four (a run always takes one pair at least).  Every
    record of a mixed batch equals the one the pair gives alone and the one given with the option at its default"""
    a, b = mp.make_pair(61, 1500, 1500), mp.make_pair(62, 300, 2049)
    A1, A2 = _set_pair(ctx, 0, a)
    C, B = _set_pair(ctx, 1, b)
    mixed = [(A1, A2), (C, B), (B, C), (A2, A1), (B, B), (B, C), (C, B), (C, A1)]
    try:
        default = ctx.MatchPairs(mixed, mp.DIST, 5)
        ctx.set_option("big_subpairs_max", 2)
        together = ctx.MatchPairs(mixed, mp.DIST, 5)
        alone = [ctx.MatchPairs([p], mp.DIST, 5)[0] for p in mixed]
    finally:
        ctx.set_option("big_subpairs_max", 65536)
    for p, r, s, d in zip(mixed, together, alone, default):
        assert r.tobytes() == s.tobytes() == d.tobytes(), p
    _same_record(together[0], mp.record_of(orc, a, mp.DIST, 5), "1500 x 1500")
    _same_record(together[1], mp.record_of(orc, b, mp.DIST, 5), "300 x 2049")
    ctx.DropFeatures(-1)


# ---- one context through every entry point ------------------------------------------------------------------------------------------------------
def test_workspaces_shared_across_entry_points(orc):
    """MatchPairs, BFMatch, SelectMatchPairs and SurfMatchPairs share workspaces (the pair table, the 1-NN arrays, sel1 / sel2 / nsel, the
    records) and each sizes them for itself: a 300 x 300 pair, a 2049 x 300 pair (the smallest large pair: two query chunks), lists of 2049
    and 100 matches and two SURF pairs, one after the other in ONE context, then the first two again.  Every output is, byte for byte, what
    the same call gives in a context of its own, and the oracle's (the SURF records against surf -> surf_match_pair, as tests/test_gpu_surf_edges.py
    checks them).  On the oracle: 90 and 396 selected, 37 and 211 inliers; 396 and 27 of the lists selected; 124 and 198 SURF correspondences
    selected, 121 and 186 of them inliers"""
    from tests import surf_patterns as su
    a, b = mp.make_pair(71, 300, 300), mp.make_pair(72, 2049, 300)
    sel = {p["tag"]: p for p in mp.fill_patterns()}["size_2049"]
    frames = su.dup_pair()

    def select_args(n):
        return (sel["matches"][:n], sel["kp1"], sel["kp2"], int(min(400.0, 0.3 * n)), sel["w"], sel["h"], 3, 3)

    def install(c):
        assert (_set_pair(c, 0, a), _set_pair(c, 1, b)) == ((0, 1), (2, 3))
        for k, f in enumerate(frames):
            c.SurfExtract(10 + k, f, su.THR, su.KEEP_ALL)

    calls = {"match small": lambda c: (c.MatchPairs([(0, 1)], mp.DIST, SEED),), "match large": lambda c: (c.MatchPairs([(2, 3)], mp.DIST, SEED),),
             "bf large": lambda c: c.BFMatch(2, 3, True, 4096), "bf small": lambda c: c.BFMatch(0, 1, True, 4096),
             "select 2049": lambda c: c.SelectMatchPairs(*select_args(2049)), "select 100": lambda c: c.SelectMatchPairs(*select_args(100)),
             "surf": lambda c: (c.SurfMatchPairs([(10, 11), (11, 10)], mp.DIST, SEED),)}
    order = ["match small", "match large", "bf large", "bf small", "select 2049", "select 100", "surf", "match small", "match large"]
    assert set(order) == set(calls)

    def as_bytes(out):
        return [np.ascontiguousarray(x).tobytes() for x in out]

    alone = {}
    for name, call in calls.items():
        with _context() as c:
            install(c)
            alone[name] = as_bytes(call(c))
    got = {}
    with _context() as c:
        install(c)
        for k, name in enumerate(order):
            got[name] = calls[name](c)
            assert as_bytes(got[name]) == alone[name], (k, name)
    for name, p in (("match small", a), ("match large", b)):
        _same_record(got[name][0][0], mp.record_of(orc, p, mp.DIST, SEED), name)
    for name, p in (("bf small", a), ("bf large", b)):
        idx, b1, b2 = orc.bf_match(p["d1"], p["d2"])
        want = orc.sort_matches(idx, b1)
        ms, s1, s2 = got[name]
        assert len(ms) == len(p["d1"]), name
        assert np.array_equal(np.stack([ms["queryIdx"], ms["trainIdx"]], 1), want) and np.array_equal(s1, b1[want[:, 0]]) and np.array_equal(s2, b2[want[:, 0]]), name
    for n, kept in ((2049, 396), (100, 27)):
        o1, o2 = orc.select(*select_args(n))
        a1, a2 = got["select %d" % n]
        assert len(o1) == kept and np.array_equal(a1, o1) and np.array_equal(a2, o2), n
    F = [orc.surf(f, su.THR, su.KEEP_ALL) for f in frames]
    for r, (i, j) in zip(got["surf"][0], ((0, 1), (1, 0))):
        n_in, i1, i2, H, n_sel = orc.surf_match_pair(F[i], F[j], mp.DIST, SEED)
        assert n_sel > 100 and n_in > 18, (i, j, n_sel, n_in)
        assert (int(r["i"]), int(r["j"]), int(r["n_selected"]), int(r["n_in"]), int(r["accepted"])) == (10 + i, 10 + j, n_sel, n_in, 1), (i, j)
        assert np.array_equal(r["a"][:n_in], i1[:n_in]) and np.array_equal(r["b"][:n_in], i2[:n_in]) and np.array_equal(bits(r["H"]), bits(H)), (i, j)

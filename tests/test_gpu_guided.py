"""GPU: guided matching (include/mi355_mosaic.h, "guided matching"; csrc/guided.hip) against the numpy restatement tests/guided_ref.py, byte for
byte: selection lists, counts, distances and whole records (the diagnostic word _pad apart), with guard bytes behind every output.  The inputs are
the crafted features of tests/guided_cases.py (tests/test_guided_ref.py shows on the CPU what each holds), installed with SetFeatures."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from tests import guided_cases as gc
from tests import guided_ref as gr
from tests import oracle_lib as ol
from tests.golden_util import GOLD
from tests.match_patterns import keypoints

pytestmark = pytest.mark.gpu
SEED = 12345
DIST = 2.5
GUARD = 0xCD


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
    import imagemosaicing_amd as im
    p = im.default_params()
    for k, v in params.items():
        setattr(p, k, v)
    c = im.Context(0, p)
    try:
        yield c
    finally:
        c.close()


def _install(c, img_id, xy, d, w=gc.W, h=gc.H):
    c.SetFeatures(img_id, keypoints(xy), np.ascontiguousarray(d, np.uint8).astype(np.float32).reshape(-1, 128), w, h)


def _install_case(c, k, case):
    _install(c, 2 * k, case["xy_i"], case["d_i"])
    _install(c, 2 * k + 1, case["xy_j"], case["d_j"])
    return (2 * k, 2 * k + 1)


def _select_dev(c, pairs, guides, want_dist=True, **params):
    """GuidedSelectDev into guarded device buffers -> (a [n, 400] SFPOINT, b, nsel [n], dist [n, 400] or None)"""
    import torch
    n = len(pairs)
    d_a = torch.full((n * 400 + 8, 12), GUARD, dtype=torch.uint8, device="cuda")
    d_b = torch.full((n * 400 + 8, 12), GUARD, dtype=torch.uint8, device="cuda")
    d_n = torch.full((n + 8, 4), GUARD, dtype=torch.uint8, device="cuda")
    d_d = torch.full((n * 400 + 8, 4), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.GuidedSelectDev(pairs, guides, d_a.data_ptr(), d_b.data_ptr(), d_n.data_ptr(), d_d.data_ptr() if want_dist else 0, **params)
    c.synchronize()
    a, b, ns, dd = d_a.cpu().numpy(), d_b.cpu().numpy(), d_n.cpu().numpy(), d_d.cpu().numpy()
    for buf, used in ((a, n * 400), (b, n * 400), (ns, n), (dd, n * 400 if want_dist else 0)):
        assert (buf[used:] == GUARD).all(), "guard bytes"
    return (a[:n * 400].copy().view(gr.SFPOINT).reshape(n, 400), b[:n * 400].copy().view(gr.SFPOINT).reshape(n, 400), ns[:n].copy().view(np.int32).reshape(n),
            dd[:n * 400].copy().view(np.int32).reshape(n, 400) if want_dist else None)


def _match_dev(c, pairs, guides, **params):
    """GuidedMatchDev into a guarded device buffer -> PAIR_RESULT [n]"""
    import torch
    n = len(pairs)
    size = gr.PAIR_RESULT.itemsize
    d_o = torch.full((n + 1, size), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.GuidedMatchDev(pairs, guides, d_o.data_ptr(), DIST, SEED, **params)
    c.synchronize()
    o = d_o.cpu().numpy()
    assert (o[n] == GUARD).all(), "guard record"
    return o[:n].copy().view(gr.PAIR_RESULT).reshape(n)


def _check_select(c, cases, max_selected=400, want_dist=True):
    """the cases grouped by their parameters, every group in ONE call, lists / counts / distances against the restatement"""
    groups = {}
    for k, case in enumerate(cases):
        groups.setdefault(tuple(sorted(case["params"].items())), []).append(k)
    ids = [_install_case(c, k, case) for k, case in enumerate(cases)]
    for key, ks in groups.items():
        a, b, ns, dd = _select_dev(c, [ids[k] for k in ks], [cases[k]["G"] for k in ks], want_dist, **dict(key))
        for r, k in enumerate(ks):
            wa, wb, wd = gc.ref_select(cases[k], max_selected)
            tag = cases[k]["tag"]
            assert int(ns[r]) == len(wa), (tag, int(ns[r]), len(wa))
            A, B, D = gr.lists_400(wa, wb, wd)
            assert a[r].tobytes() == A.tobytes() and b[r].tobytes() == B.tobytes(), (tag, "lists")
            assert dd is None or dd[r].tobytes() == D.tobytes(), (tag, "distances")
    c.DropFeatures(-1)


def _want_record(orc, ij, case, max_selected=400, min_inliers=30):
    return gr.record(orc, ij[0], ij[1], case["xy_i"], case["d_i"], case["xy_j"], case["d_j"], case["G"], DIST, SEED, max_selected=max_selected,
                     min_inliers=min_inliers, **dict(gr.DEFAULTS, **case["params"]))


def _check_records(c, orc, cases, **ctx_params):
    ids = [_install_case(c, k, case) for k, case in enumerate(cases)]
    out = {}
    for k, case in enumerate(cases):                        # a call per case: the parameters differ
        got = _match_dev(c, [ids[k]], [case["G"]], **case["params"])[0]
        want = _want_record(orc, ids[k], case, **ctx_params)
        assert (int(got["n_selected"]), int(got["n_in"]), int(got["accepted"])) == (int(want["n_selected"]), int(want["n_in"]), int(want["accepted"])), case["tag"]
        assert gr.record_bytes(got) == gr.record_bytes(want), case["tag"]
        out[case["tag"]] = got
    c.DropFeatures(-1)
    return out


# ---- the selection --------------------------------------------------------------------------------------------------------------------------------
def test_select_crafted_cases(ctx):
    """the radius edge, the lane and LDS strides, equal d at two k and equal d1 from two q, max_dist2 and the ratio at equality, all 0 against all
    255, 401 and 500 survivors with equal d1 across the cut, n_sel 3 and 4"""
    _check_select(ctx, gc.crafted_cases())


def test_select_keypoint_counts(ctx):
    """0, 1, 3, 4, 255, 256, 257, 2047 and 2048 keypoints on either side"""
    _check_select(ctx, gc.size_cases())


def test_select_guides(ctx):
    """identity, non-integer shift, similarity, mild projective, a zero denominator at one keypoint, all zero, NaN and inf entries"""
    _check_select(ctx, gc.guide_cases())


def test_select_without_distances(ctx):
    _check_select(ctx, gc.cut_cases()[:2], want_dist=False)


def test_max_selected_below_400(orc):
    with _context(max_selected=100) as c:
        _check_select(c, [gc.survivor_case(500), gc.survivor_case(99), gc.scene(31, 700, 700, gc.SHIFT)], max_selected=100)
        _check_records(c, orc, [gc.scene(31, 700, 700, gc.SHIFT)], max_selected=100)
    with _context(max_selected=0) as c:
        _check_select(c, [gc.survivor_case(4)], max_selected=0)


# ---- whole records --------------------------------------------------------------------------------------------------------------------------------
def test_records_of_crafted_and_planted_pairs(ctx, orc):
    """n_sel 3 and 4 (Ransac2D's smallest lists), the cut cases, full frames, a guide that finds nothing, and the planted planar pair: 300 true ties
    plus 100 wrong ones inside the radius"""
    cases = gc.cut_cases() + [gc.scene(301, 2048, 2048, gc.SHIFT), gc.scene(41, 90, 80, gc.SIMILARITY), gc.guide_cases()[-1], gc.planted_case()]
    got = _check_records(ctx, orc, cases)
    p = got["planted planar pair"]
    assert int(p["accepted"]) == 1 and int(p["n_selected"]) == 400 and int(p["n_in"]) >= 280
    assert int(got["n_sel 3"]["n_selected"]) == 3 and int(got["n_sel 4"]["n_selected"]) == 4
    rejected = got[gc.guide_cases()[-1]["tag"]]
    assert int(rejected["accepted"]) == 0 and not np.frombuffer(gr.record_bytes(rejected)[8:], np.uint8).any()


@pytest.mark.parametrize("n_pairs", [1, 256, 257])
def test_many_pairs_in_one_call(ctx, orc, n_pairs):
    """1, 256 and 257 pairs in one call, the same pair several times among them"""
    scenes = [gc.scene(500 + k, 80 + 9 * k, 120 - 5 * k, G) for k, G in enumerate((gc.SHIFT, gc.IDENTITY, gc.PROJECTIVE, gc.SIMILARITY, gc.SHIFT, gc.ZERO_DEN))]
    ids = [_install_case(ctx, k, s) for k, s in enumerate(scenes)]
    which = [(5 * p + p // 7) % len(scenes) for p in range(n_pairs)]
    pairs, guides = [ids[k] for k in which], [scenes[k]["G"] for k in which]
    sel = [gr.lists_400(*gc.ref_select(s)) for s in scenes]
    nsel = [len(gc.ref_select(s)[0]) for s in scenes]
    a, b, ns, dd = _select_dev(ctx, pairs, guides)
    for p, k in enumerate(which):
        assert int(ns[p]) == nsel[k] and a[p].tobytes() == sel[k][0].tobytes() and b[p].tobytes() == sel[k][1].tobytes() and dd[p].tobytes() == sel[k][2].tobytes(), p
    want = [_want_record(orc, ids[k], s) for k, s in enumerate(scenes)]
    dev = _match_dev(ctx, pairs, guides)
    host = ctx.GuidedMatch(pairs, guides, DIST, SEED)
    for p, k in enumerate(which):
        assert gr.record_bytes(dev[p]) == gr.record_bytes(want[k]) == gr.record_bytes(host[p]), p
    assert any(int(r["accepted"]) for r in dev) or max(nsel) <= 30
    ctx.DropFeatures(-1)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable(ctx, orc):
    import imagemosaicing_amd as im
    import torch
    s = gc.scene(600, 50, 50, gc.SHIFT)
    ij = _install_case(ctx, 0, s)
    rng = np.random.default_rng(0)
    _install(ctx, 7, rng.uniform(0, 700, (2049, 2)), gc.rand_desc(rng, 2049))
    d_o = torch.zeros((2, gr.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    d_l = torch.zeros((2 * 400, 12), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(2, dtype=torch.int32, device="cuda")

    def all_three(pairs, guides, msg, **kw):
        with pytest.raises(im.Mi355Error, match=msg):
            ctx.GuidedSelectDev(pairs, guides, d_l.data_ptr(), d_l.data_ptr(), d_n.data_ptr(), **kw)
        with pytest.raises(im.Mi355Error, match=msg):
            ctx.GuidedMatchDev(pairs, guides, d_o.data_ptr(), DIST, SEED, **kw)
        with pytest.raises(im.Mi355Error, match=msg):
            ctx.GuidedMatch(pairs, guides, DIST, SEED, **kw)

    for r in (0.0, -1.0, 64.5, np.nan, np.inf):
        all_three([ij], [s["G"]], "radius=", radius=r)
    for m in (-1, 8323201):
        all_three([ij], [s["G"]], "max_dist2=%d" % m, max_dist2=m)
    for r in (-0.1, 1.5, np.nan, np.inf):
        all_three([ij], [s["G"]], "ratio=", ratio=r)
    all_three([ij], [s["G"]], "reserved=1", reserved=1)
    all_three([ij, (1, 1)], [s["G"], s["G"]], "pair 1: i == j == 1")
    all_three([ij, (0, 99)], [s["G"], s["G"]], "no resident features for image 99")
    all_three([(98, 1)], [s["G"]], "no resident features for image 98")
    all_three([(0, 7)], [s["G"]], "image 7 holds 2049 keypoints")
    all_three([(7, 1)], [s["G"]], "image 7 holds 2049 keypoints")
    # n < 0 and NULL arrays, through the C interface
    pr, gd = np.array([ij], np.int32), np.ascontiguousarray(s["G"], np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
    L, h = ctx.L, ctx._h
    out = np.zeros(1, gr.PAIR_RESULT)
    for n, p, g, o, msg in ((-1, vp(pr), vp(gd), vp(out), "n=-1"), (1, None, vp(gd), vp(out), "NULL pairs_ij"), (1, vp(pr), None, vp(out), "NULL guides"), (1, vp(pr), vp(gd), None, "NULL records")):
        assert L.mi355_guided_match(h, p, n, g, None, C.c_float(DIST), C.c_uint32(SEED), o) < 0
        assert msg in L.mi355_last_error(h).decode()
        assert L.mi355_guided_match_dev(h, p, n, g, None, C.c_float(DIST), C.c_uint32(SEED), C.c_void_p(d_o.data_ptr()) if o else None) < 0
    assert L.mi355_guided_select_dev(h, vp(pr), 1, vp(gd), None, None, C.c_void_p(d_l.data_ptr()), C.c_void_p(d_n.data_ptr()), None) < 0
    assert L.mi355_guided_select_dev(h, vp(pr), -1, vp(gd), None, C.c_void_p(d_l.data_ptr()), C.c_void_p(d_l.data_ptr()), C.c_void_p(d_n.data_ptr()), None) < 0
    # n == 0 is fine and launches nothing (all pointers NULL); params NULL means the defaults
    assert L.mi355_guided_match(h, None, 0, None, None, C.c_float(DIST), C.c_uint32(SEED), None) == 0
    assert L.mi355_guided_match_dev(h, None, 0, None, None, C.c_float(DIST), C.c_uint32(SEED), None) == 0
    assert L.mi355_guided_select_dev(h, None, 0, None, None, None, None, None, None) == 0
    assert L.mi355_guided_match(h, vp(pr), 1, vp(gd), None, C.c_float(DIST), C.c_uint32(SEED), vp(out)) == 0
    with _context(max_selected=401) as c2:
        _install_case(c2, 0, s)
        with pytest.raises(im.Mi355Error, match="max_selected=401"):
            c2.GuidedMatch([ij], [s["G"]], DIST, SEED)
    # the ctx still works
    want = _want_record(orc, ij, s)
    assert gr.record_bytes(out[0]) == gr.record_bytes(want)
    assert gr.record_bytes(ctx.GuidedMatch([ij], [s["G"]], DIST, SEED)[0]) == gr.record_bytes(want)
    ctx.DropFeatures(-1)


# ---- end to end on the reference's frames ---------------------------------------------------------------------------------------------------------
def test_golden_frames_end_to_end(ctx, orc):
    """frames 4..11 of the reference's run: GPU SIFT, match_pairs with window 4, guides chained from the accepted consecutive pairs, GuidedMatchDev on
    spans 2 and 3.  The records equal the restatement on the GPU's own features, and the merged record set has more accepted pairs than the base."""
    import imagemosaicing_amd as im
    from PIL import Image
    n = 8
    for k in range(n):
        img = np.ascontiguousarray(np.array(Image.open(os.path.join(GOLD, "DSC%05d.JPG" % (4 + k))).convert("RGB"))[:, :, ::-1])
        ctx.SiftExtractHost(k, img)
    base = ctx.MatchPairs([(i, j) for i in range(n) for j in range(i + 1, min(n, i + 4))], DIST, SEED)
    chains = gr.chain_guides(base, n)
    pairs = [ij for ij in sorted(chains) if ij[1] - ij[0] in (2, 3)]
    assert len(pairs) >= 8
    guides = [chains[ij] for ij in pairs]
    got = _match_dev(ctx, pairs, guides)
    feats = [ctx.GetFeatures(k) for k in range(n)]
    xy = [np.stack([kp["x"], kp["y"]], 1) for kp, _ in feats]
    ds = [d.astype(np.uint8) for _, d in feats]
    want = ol.parallel_map(lambda t: gr.record(orc, t[0][0], t[0][1], xy[t[0][0]], ds[t[0][0]], xy[t[0][1]], ds[t[0][1]], t[1], DIST, SEED), list(zip(pairs, guides)))
    for ij, g, w in zip(pairs, got, want):
        assert gr.record_bytes(g) == gr.record_bytes(w), (ij, int(g["n_in"]), int(w["n_in"]))
    merged = im.merge_pair_results(base, got)
    assert len(merged) == len(base) and int(merged["accepted"].sum()) > int(base["accepted"].sum()), (int(merged["accepted"].sum()), int(base["accepted"].sum()))
    assert (merged["n_in"] >= base["n_in"]).all()
    ctx.DropFeatures(-1)

"""GPU: mi355_refine_ties_dev / mi355_refine_ties (csrc/tie_refine.hip) against the numpy restatement of the header's definition
(tests/tie_refine_ref.py): records, status, ncc2 and report byte for byte, out of place and in place, with guard bytes behind every output
and the frames' own bytes (padding included) unchanged.  The quality bounds are asserted on the reference by tests/test_tie_refine_ref.py and
hold here through byte equality; the quality test repeats them on the library's own output."""
import numpy as np
import pytest

from tests import tie_refine_cases as tc
from tests import tie_refine_ref as tr
from tests.pitched import PitchedFrames, ipl_pitch, pitch_kinds

pytestmark = pytest.mark.gpu
REC = tr.PAIR_RESULT.itemsize
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1]


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


class DevFrames:
    """imgs (None: a frame the caller does not hold) in one pitched device buffer"""

    def __init__(self, torch, imgs, pitches=None, offsets=None):
        self.torch = torch
        real = [k for k, i in enumerate(imgs) if i is not None]
        self.pf = PitchedFrames([imgs[k] for k in real], pitches if pitches is not None else [ipl_pitch(imgs[k].shape[1]) for k in real], offsets, seed=7)
        self.t, ptrs = self.pf.to_device(torch)
        n = len(imgs)
        self.ptrs, self.w, self.h, self.ws = [0] * n, np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        for q, k in enumerate(real):
            self.ptrs[k], self.w[k], self.h[k], self.ws[k] = ptrs[q], self.pf.w[q], self.pf.h[q], self.pf.ws[q]

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.pf.buf)


def run_dev(ctx, torch, recs, fr, inplace=False, want_outputs=True, **params):
    n = len(recs)
    guard = lambda nbytes: torch.full((nbytes + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    d_in = guard(n * REC)
    if n:
        d_in[:n * REC] = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = d_in if inplace else guard(n * REC)
    d_st, d_nc, d_rep = guard(n * 400), guard(n * 1600), guard(n * 64)
    torch.cuda.synchronize()
    if want_outputs:
        ctx.RefineTiesDev(d_in.data_ptr(), n, fr.ptrs, fr.w, fr.h, fr.ws, d_out.data_ptr(), d_st.data_ptr(), d_nc.data_ptr(), d_rep.data_ptr(), **params)
    else:
        ctx.RefineTiesDev(d_in.data_ptr(), n, fr.ptrs, fr.w, fr.h, fr.ws, d_out.data_ptr(), **params)
    ctx.synchronize()
    bufs = [b.cpu().numpy() for b in (d_out, d_st, d_nc, d_rep, d_in)]
    for b, size in zip(bufs, (n * REC, n * 400, n * 1600, n * 64, n * REC)):
        assert (b[size:] == 0xCD).all()
        if not want_outputs and b is not bufs[0] and b is not bufs[4]:
            assert (b == 0xCD).all()
    if not inplace:
        assert bufs[4][:n * REC].tobytes() == recs.tobytes()                  # the input is only read
    return (bufs[0][:n * REC].view(tr.PAIR_RESULT).copy(), bufs[1][:n * 400].reshape(n, 400).copy(), bufs[2][:n * 1600].view(np.float32).reshape(n, 400).copy(),
            bufs[3][:n * 64].view(tr.TIE_REPORT).copy())


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("records", "status", "ncc2", "report")):
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))[0]
            if name == "status":
                idx = np.argwhere(g != w)[:5]
                raise AssertionError("%s %s: %s got %s want %s" % (what, name, idx.tolist(), [g[tuple(i)] for i in idx], [w[tuple(i)] for i in idx]))
            raise AssertionError("%s %s: %d bytes differ, first at %d" % (what, name, len(bad), bad[0]))


def check(ctx, torch, recs, imgs, pitches=None, offsets=None, min_inliers=30, **params):
    want = tr.refine_ties(recs, imgs, min_inliers=min_inliers, **params)
    fr = DevFrames(torch, imgs, pitches, offsets)
    same(run_dev(ctx, torch, recs, fr, **params), want, "out of place")
    same(run_dev(ctx, torch, recs, fr, inplace=True, **params), want, "in place")
    assert fr.unchanged()
    return want


def pair_case(wj, hj, wi, hi, H, n_ties, seed, noise=0.4, margin=-2.0):
    """frame j random, frame i = frame j seen through H; n_ties points b over frame j (margin < 0: also outside it), a = H(b) + noise"""
    rng = np.random.default_rng(seed)
    fj = tc.random_frame(wj, hj, seed)
    fi = tc.warp_frame(fj, H, wi, hi)
    b = np.stack([rng.uniform(margin, wj - 1 - margin, n_ties), rng.uniform(margin, hj - 1 - margin, n_ties)], 1)
    b[::3] = np.rint(b[::3] * 4) / 4                                            # a third on quarter pixels: p, q of 0, 1/4, 1/2, 3/4
    ax, ay = tc.project(np.asarray(H, np.float64).reshape(3, 3), b[:, 0], b[:, 1])
    a = np.stack([ax, ay], 1) + rng.normal(0, noise, b.shape)
    return [fi, fj], tc.record(0, 1, a, b, H)


ROT = tc.similarity(12.0, 1.06, 4.0, -6.0).reshape(9)
PROJ = tc.similarity(-5.0, 0.97, 3.0, 2.0, 3e-4, -2e-4).reshape(9)
SHIFT = [1, 0, 2, 0, 1, 1, 0, 0, 1]


# ---- 1 shapes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(33, 29, 33, 29), (40, 36, 40, 36), (96, 80, 96, 80), (96, 80, 61, 70)])
def test_frame_sizes_pitches_and_offsets(ctx, size):
    import torch
    wj, hj, wi, hi = size
    seen = set()
    for q, (R, S) in enumerate(((2, 1), (7, 3), (1, 4), (10, 4))):
        imgs, rec = pair_case(wj, hj, wi, hi, SHIFT, 48, 10 + q, margin=R + S - 3.0)
        recs = tc.records(rec)
        pitches = [pitch_kinds(wi)[(q + 2) % 5], pitch_kinds(wj)[q % 5]]
        want = check(ctx, torch, recs, imgs, pitches=pitches, offsets=[q % 4, (q + 1) % 4], radius=R, search=S)
        seen |= set(want[1][0, :48].tolist())
    assert tr.EDGE in seen and (tr.REFINED in seen or min(size) < 34), seen


@pytest.mark.parametrize("R,S", [(1, 1), (1, 3), (2, 4), (7, 1), (7, 3), (7, 4), (10, 1), (10, 3), (10, 4)])
def test_radius_and_search(ctx, R, S):
    import torch
    imgs, rec = pair_case(96, 80, 96, 80, ROT, 40, 3, margin=R + S + 1.0)
    want = check(ctx, torch, tc.records(rec), imgs, radius=R, search=S)
    assert want[3]["count"][0][tr.REFINED] >= 1, want[3]["count"][0]                  # the case reaches the last step


def test_tie_counts_record_counts_and_optional_outputs(ctx):
    import torch
    imgs, big = pair_case(96, 80, 96, 80, ROT, 400, 4, margin=9.0)
    recs = []
    for n_in in (1, 63, 64, 65, 399, 400):
        r = big.copy()
        r["n_in"] = n_in
        r["a"][n_in:] = 0
        r["b"][n_in:] = 0
        recs.append(r)
    want = check(ctx, torch, tc.records(*recs), imgs, radius=3, search=2)
    assert want[3]["count"][:, tr.REFINED].tolist() == [int((want[1][5, :n] == tr.REFINED).sum()) for n in (1, 63, 64, 65, 399, 400)]
    assert want[3]["count"][5][tr.REFINED] > 300
    # 70 records of a few ties each, some of them not processed; 3; 1; 0
    many = []
    for k in range(70):
        r = big.copy()
        n_in = 1 + (k * 7) % 11
        r["a"][:n_in], r["b"][:n_in] = big["a"][k * 5:k * 5 + n_in], big["b"][k * 5:k * 5 + n_in]
        r["n_in"] = n_in
        r["a"][n_in:] = 0
        r["b"][n_in:] = 0
        r["accepted"] = 0 if k % 9 == 4 else 1
        many.append(r)
    many = tc.records(*many)
    for n in (70, 3, 1, 0):
        check(ctx, torch, many[:n], imgs, radius=4, search=1)
    # no optional output: the records alone
    fr = DevFrames(torch, imgs)
    got = run_dev(ctx, torch, many[:3], fr, want_outputs=False, radius=4, search=1)
    assert got[0].tobytes() == tr.refine_ties(many[:3], imgs, radius=4, search=1)[0].tobytes()


# ---- 2 content ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [2, 3])
def test_checkers_equal_peaks_and_the_cast_on_its_boundary(ctx, period):
    import torch
    ch = tc.checker(48, 40, period)
    rng = np.random.default_rng(period)
    b = np.rint(rng.uniform(11, 28, (60, 2)) * 4) / 4                           # quarter pixels: samples of 0, 63.75, 127.5, 191.25, 255 before the cast
    a = b + np.rint(rng.uniform(-1, 1, b.shape) * 2) / 2
    recs = tc.records(tc.record(0, 1, a, b, IDENT), tc.record(1, 0, b, b, IDENT))
    for S in (3, 1):
        want = check(ctx, torch, recs, [ch, ch.copy()], radius=3, search=S)
        st, peak = want[1][1, :60], want[2][1, :60]
        live = st != tr.FLAT                                # period 2 sampled at a half pixel is 127 everywhere: FLAT
        assert live.sum() >= 20 and (period == 3 or not live.all())
        # equal patches score exactly 1; where a whole period fits the search range the first of the equal peaks is the corner (-S, -S)
        assert (peak[live] == 1.0).all() and (st[live] == (tr.BORDER if period == 2 or S == 3 else tr.REFINED)).all()


def test_flat_frames_flat_windows_and_min_ncc(ctx):
    import torch
    white = np.full((36, 40, 3), 255, np.uint8)
    b = np.array([[20.0, 18.0], [15.25, 14.5], [12.0, 12.0]])
    want = check(ctx, torch, tc.records(tc.record(0, 1, b, b, IDENT)), [white, white.copy()])
    assert (want[1][0, :3] == tr.FLAT).all()
    imgs, recs, st = tc.status_case()
    for min_ncc in (0.7, 0.0, 1.0):
        want = check(ctx, torch, recs, imgs, min_ncc=min_ncc)
        assert want[1][0, 6] == tr.LOW and want[2][0, 6] == 0                   # every vw = 0: peak 0 is LOW whatever min_ncc says
        if min_ncc == 0.7:
            assert want[1][0, :len(st)].tolist() == st.tolist()
        if min_ncc == 1.0:
            assert want[1][0, 1] == tr.REFINED and want[1][0, 0] == tr.LOW


# ---- 3 geometry --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H", [("identity", IDENT), ("rotation", ROT), ("projective", PROJ)])
def test_maps(ctx, name, H):
    import torch
    imgs, rec = pair_case(96, 80, 110, 90, H, 80, 6, margin=6.0)
    rec["H"][8] = 2.25                                                          # the residual slot must be read as 1
    want = check(ctx, torch, tc.records(rec), imgs, radius=5, search=2)
    assert want[3]["count"][0][tr.REFINED] >= 1, want[3]["count"][0]


def test_bad_coordinates_and_a_denominator_through_zero(ctx):
    import torch
    imgs, rec = pair_case(96, 80, 96, 80, IDENT, 24, 8, margin=12.0)
    for k, (fld, c, v) in enumerate((("a", "x", np.nan), ("a", "y", np.nan), ("b", "x", np.nan), ("b", "y", np.nan), ("a", "x", 1e30), ("b", "y", 1e30),
                                      ("a", "x", -1e30), ("a", "y", -3.0), ("b", "x", -0.5), ("b", "y", -40.0), ("a", "x", np.inf), ("b", "x", -np.inf))):
        rec[fld][c][k] = v
    zero = rec.copy()
    zero["b"]["x"][:4] = [40.0, 36.0, 44.0, 47.0]
    zero["H"] = [1, 0, 0, 0, 1, 0, -0.025, 0, 1]                                # 1 - x / 40: zero at b.x = 40, crossing zero inside the other windows
    nanH = rec.copy()
    nanH["H"][4] = np.nan
    want = check(ctx, torch, tc.records(rec, zero, nanH), imgs, radius=4, search=2)
    assert (want[1][0, :12] == tr.EDGE).all() and (want[1][0, 12:24] != tr.EDGE).all()
    assert (want[1][1, :4] == tr.EDGE).all() and (want[1][2, :24] == tr.EDGE).all()


def test_patches_on_and_one_ulp_beside_the_frame_edges(ctx):
    import torch
    w, h, R, S = 64, 56, 3, 2
    fj = tc.random_frame(w, h, 9)
    imgs = [fj.copy(), fj]
    dn, up = (lambda v: np.nextafter(np.float32(v), np.float32(-1e9))), (lambda v: np.nextafter(np.float32(v), np.float32(1e9)))
    mid = (30.0, 25.0)
    pts, expect = [], []
    # templates: b.x - R >= 0 and b.x + R < w - 1, likewise y; a in the middle, so that only the template decides
    for bx, by, ok in ((R, mid[1], 1), (dn(R), mid[1], 0), (dn(w - 1 - R), mid[1], 1), (w - 1 - R, mid[1], 0),
                       (mid[0], R, 1), (mid[0], dn(R), 0), (mid[0], dn(h - 1 - R), 1), (mid[0], h - 1 - R, 0)):
        pts.append((mid[0], mid[1], bx, by)); expect.append(ok)
    # windows: a.x - (R + S) >= 0 and a.x + (R + S) < w - 1; b in the middle
    RS = R + S
    for ax, ay, ok in ((RS, mid[1], 1), (dn(RS), mid[1], 0), (dn(w - 1 - RS), mid[1], 1), (w - 1 - RS, mid[1], 0),
                       (mid[0], RS, 1), (mid[0], dn(RS), 0), (mid[0], dn(h - 1 - RS), 1), (mid[0], h - 1 - RS, 0), (up(RS), up(RS), 1)):
        pts.append((ax, ay, mid[0], mid[1])); expect.append(ok)
    pts = np.array(pts, np.float32)
    want = check(ctx, torch, tc.records(tc.record(0, 1, pts[:, :2], pts[:, 2:], IDENT)), imgs, radius=R, search=S)
    st = want[1][0, :len(pts)]
    assert ((st != tr.EDGE) == np.array(expect, bool)).all(), st


def test_a_peak_at_each_border_and_corner_of_the_search_range(ctx):
    import torch
    imgs, _, _ = tc.status_case()
    S = 3
    shifts = [(dx, dy) for dy in (-S, 0, S) for dx in (-S, 0, S)] + [(1, -2), (-2, 2)]
    b = np.array([[40.0 + (k % 3), 48.0 + k // 3] for k in range(len(shifts))])
    a = b + [2, 1] - np.array(shifts, np.float64)                               # the true place is a + shift
    want = check(ctx, torch, tc.records(tc.record(0, 1, a, b, SHIFT)), imgs, search=S)
    st = want[1][0, :len(shifts)]
    assert st.tolist() == [tr.REFINED if max(abs(dx), abs(dy)) < S else tr.BORDER for dx, dy in shifts]
    assert (want[2][0, :len(shifts)] == 1.0).all()


# ---- 4 records ---------------------------------------------------------------------------------------------------------------------------
def unprocessed_records():
    imgs, recs, _ = tc.status_case()
    r = [recs[0].copy() for _ in range(9)]
    r[1]["accepted"] = 0
    r[2]["j"] = 2                                           # a frame that is not held
    r[3]["i"] = 1                                           # i == j
    r[4]["i"], r[4]["j"] = 1, 0                             # i > j: processed
    r[5]["j"] = 3                                           # index out of range
    r[6]["i"] = -1
    r[7]["n_in"] = 0
    r[8]["n_in"] = 401
    flags = [0, tr.F_NOT_ACCEPTED, tr.F_NO_FRAME, tr.F_BAD, 0, tr.F_BAD, tr.F_BAD, tr.F_BAD, tr.F_BAD]
    return imgs + [None], tc.records(*r), flags


def test_records_that_are_not_processed_are_copied_bit_for_bit(ctx):
    import torch
    imgs, recs, flags = unprocessed_records()
    want = check(ctx, torch, recs, imgs)
    assert want[3]["flags"].tolist() == flags
    for k, f in enumerate(flags):
        if f:
            assert want[0][k].tobytes() == recs[k].tobytes() and not want[1][k].any()


def test_host_form_equals_the_reference_and_refuses_bad_records(ctx):
    import imagemosaicing_amd as im
    imgs, recs, flags = unprocessed_records()
    good = recs[[0, 1, 2, 4]]
    want = tr.refine_ties(good, imgs)
    same(ctx.RefineTies(good, imgs), want, "host form")
    qc = tc.quality()
    same(ctx.RefineTies(qc["rec"], qc["imgs"], drop_mask=0x30), tr.refine_ties(qc["rec"], qc["imgs"], drop_mask=0x30), "host form, quality")
    for k in (3, 5, 6, 7, 8):
        with pytest.raises(im.Mi355Error, match="record 1") as e:
            ctx.RefineTies(recs[[0, k]], imgs)
        assert e.value.code == -1
    same(ctx.RefineTies(good, imgs), want, "host form after the refusals")
    assert len(ctx.RefineTies(recs[:0], imgs)[0]) == 0


def test_parameter_refusals_leave_the_ctx_usable(ctx):
    import torch
    import imagemosaicing_amd as im
    imgs, recs, _ = tc.status_case()
    fr = DevFrames(torch, imgs)
    bad = [dict(radius=0), dict(radius=11), dict(search=0), dict(search=5), dict(min_ncc=-0.1), dict(min_ncc=1.5), dict(min_ncc=float("nan")),
           dict(min_ncc=float("inf")), dict(drop_mask=1), dict(drop_mask=2), dict(drop_mask=0x40), dict(drop_mask=-1)]
    for kw in bad:
        name = list(kw)[0]
        with pytest.raises(im.Mi355Error, match=name) as e:
            run_dev(ctx, torch, recs, fr, **kw)
        assert e.value.code == -1
        with pytest.raises(im.Mi355Error, match=name):
            ctx.RefineTies(recs, imgs, **kw)
    p = im.tie_params()
    assert (p.radius, p.search, p.drop_mask, p.reserved, p.min_ncc) == (7, 3, 0, 0, np.float32(0.7))
    p.reserved = 1
    with pytest.raises(im.Mi355Error, match="reserved"):
        run_dev(ctx, torch, recs, fr, params=p)
    small = DevFrames(torch, imgs)
    small.w[0] = 1
    with pytest.raises(im.Mi355Error, match="image 0"):
        run_dev(ctx, torch, recs, small)
    same(run_dev(ctx, torch, recs, fr), tr.refine_ties(recs, imgs), "after the refusals")


# ---- 5 dropping --------------------------------------------------------------------------------------------------------------------------
def test_dropping_and_demotion(ctx):
    import torch
    import imagemosaicing_amd as im
    imgs, recs, st = tc.status_case()
    n = len(st)
    for mask in (1 << tr.EDGE, 1 << tr.FLAT, 1 << tr.LOW, 1 << tr.BORDER, 0x3c):
        kept = sum(1 for s in st if not (mask >> s) & 1)
        for min_inliers in (kept - 1, kept):                # demotion exactly at n_out == min_inliers, not at min_inliers + 1
            p = im.default_params()
            p.min_inliers = min_inliers
            c = im.Context(0, p)
            try:
                want = check(c, torch, recs, imgs, min_inliers=min_inliers, drop_mask=mask)
            finally:
                c.close()
            assert want[0]["n_in"][0] == kept and want[3]["flags"][0] == (tr.F_DEMOTED if min_inliers == kept else 0)
            assert want[0]["accepted"][0] == (0 if min_inliers == kept else 1)
            assert want[1][0, :n].tolist() == st.tolist()                       # status stays at the original indices
    # a longer record: chunks of the prefix sum, stable order, zeroed tail
    imgs2, big = pair_case(96, 80, 96, 80, ROT, 400, 12, margin=2.0)
    want = check(ctx, torch, tc.records(big), imgs2, radius=3, search=2, drop_mask=0x3c)
    keep = np.nonzero(want[1][0] == tr.REFINED)[0]
    assert 100 < len(keep) < 400 and want[0]["n_in"][0] == len(keep)
    assert np.array_equal(want[0]["a"]["id"][0, :len(keep)], big["a"]["id"][keep]) and not want[0]["a"]["id"][0, len(keep):].any()


# ---- 6 quality ---------------------------------------------------------------------------------------------------------------------------
def test_quality_against_ground_truth(ctx):
    import torch
    q = tc.quality()
    n = len(q["truth"])
    off = q["rec"].copy()
    off["H"][0, 2] += np.float32(0.5)
    off["H"][0, 5] += np.float32(0.5)
    for name, recs in (("exact H", q["rec"]), ("H off by half a pixel", off)):
        want = check(ctx, torch, recs, q["imgs"])
        fr = DevFrames(torch, q["imgs"])
        got = run_dev(ctx, torch, recs, fr)
        before, after = tc.rms(recs[0], q["truth"]), tc.rms(got[0][0], q["truth"])
        not_refined = int((got[1][0, :n] != tr.REFINED).sum())
        print("%s: ties %d not refined %d rms before %.4f after %.4f ratio %.4f" % (name, n, not_refined, before, after, after / before))
        assert not_refined <= 0.10 * n and after <= before / 3.0
    false = [tc.render(tc.scene(9), tc.similarity(12.0, 1.06, 150.0, 90.0, 4e-5, -3e-5), 240, 240, np.random.default_rng(109), 2.0), q["imgs"][1]]
    want = check(ctx, torch, q["rec"], false, drop_mask=0x30)
    assert np.isin(want[1][0, :n], (tr.LOW, tr.BORDER)).all() and want[3]["n_out"][0] == 0 and want[3]["flags"][0] == tr.F_DEMOTED
    assert want[0]["accepted"][0] == 0


# ---- 7 downstream ------------------------------------------------------------------------------------------------------------------------
def survey4():
    """four 160 x 120 frames of one scene under known affine maps, the six pairs' ties with 0.5 px of noise"""
    sc = tc.scene(21, 360)
    rng = np.random.default_rng(22)
    G = [tc.similarity(d, s, tx, ty) for d, s, tx, ty in ((0, 1.0, 60, 70), (6, 1.03, 100, 62), (-5, 0.97, 70, 110), (9, 1.05, 118, 104))]
    imgs = [tc.render(sc, g, 160, 120, rng, 2.0) for g in G]
    recs = []
    for i in range(4):
        for j in range(i + 1, 4):
            H = np.linalg.inv(G[i]) @ G[j]
            b = np.stack([rng.uniform(12, 147, 300), rng.uniform(12, 107, 300)], 1)
            tx, ty = tc.project(H, b[:, 0], b[:, 1])
            ok = (tx >= 12) & (tx < 147) & (ty >= 12) & (ty < 107)
            assert ok.sum() > 40
            t = np.stack([tx[ok], ty[ok]], 1)
            recs.append(tc.record(i, j, t + rng.normal(0, 0.5, t.shape), b[ok], H.reshape(9)))
    truth = [np.linalg.inv(G[0]) @ g for g in G]
    return imgs, tc.records(*recs), truth


def corner_error(transforms, truth):
    worst = 0.0
    for k, T in enumerate(truth):
        m = transforms["m"][k].astype(np.float64).reshape(3, 3)
        for x, y in ((0, 0), (159, 0), (0, 119), (159, 119)):
            gx, gy = tc.project(m, x, y)
            wx, wy = tc.project(T, x, y)
            worst = max(worst, float(np.hypot(gx - wx, gy - wy)))
    return worst


def test_downstream_alignment_improves_and_takes_the_refined_records(ctx):
    import torch
    import imagemosaicing_amd as im
    imgs, recs, truth = survey4()
    fr = DevFrames(torch, imgs)
    n = len(recs)
    d = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    ctx.RefineTiesDev(d.data_ptr(), n, fr.ptrs, fr.w, fr.h, fr.ws, d.data_ptr(), drop_mask=0x3c)
    ctx.synchronize()
    refined = d.cpu().numpy().view(im.PAIR_RESULT)
    assert refined.tobytes() == tr.refine_ties(recs, imgs, drop_mask=0x3c)[0].tobytes()
    assert (refined["accepted"] == 1).all() and (refined["n_in"] >= 0.9 * recs["n_in"]).all()
    e0 = corner_error(im.global_affine_align_results(recs, 4), truth)
    e1 = corner_error(im.global_affine_align_results(refined, 4), truth)
    print("largest corner error: unrefined %.4f px, refined %.4f px" % (e0, e1))
    assert e1 < e0
    # the refined device records go on as they are
    d_m = torch.zeros((n, im.PAIR_MOMENTS.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.PairMomentsDev(d.data_ptr(), n, d_m.data_ptr())
    ctx.synchronize()
    assert d_m.cpu().numpy().reshape(-1).view(im.PAIR_MOMENTS).tobytes() == im.pair_moments_host(refined).tobytes()
    start = im.global_affine_align_results(refined, 4)
    ww, hh = np.full(4, 160, np.int32), np.full(4, 120, np.int32)
    got, rep = ctx.GlobalProjectiveRefineDev(d.data_ptr(), n, ww, hh, start)
    want, wrep = im.global_projective_refine_results(refined, ww, hh, start)
    assert got.tobytes() == want.tobytes() and rep == wrep and rep["n_pairs_used"] == n

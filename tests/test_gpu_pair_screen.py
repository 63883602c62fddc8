"""GPU: the descriptor-screened pair schedule (mi355_screen_scores_dev / mi355_screen_pairs, csrc/screen.hip).

  * scores: bit for bit equal to tests/screen_ref.py on 40 synthetic 1280x960 frames (all pairs) at top_k 32 / 160 / 256 / 512 and
    ratio_pct 80 / 100, with SetFeatures frames of 5 and 0 keypoints and one whose responses tie across the K boundary, and on keep-all
    frames (nfeatures <= 0, keypoints not in response order) of more than 2048 keypoints;
  * an unordered survey: the same 40 frames (a 4-row serpentine) with their ids permuted: a window of 3 over that order does not connect
    the survey, the screened list does, keeps every pair that exhaustive matching accepts with n_in >= 60, and its records equal the
    exhaustive ones byte for byte;
  * the schedule's form: order, window subset, rank shards, the selection against the restatement, a second context, max_pairs and the
    argument errors;
  * C4 at its own size: 500 frames of 4000x3000 screened in window 182 mode; the screened list is matched and compared with the window's.
"""
import ctypes as C

import numpy as np
import pytest

from tests import screen_ref as sr

pytestmark = pytest.mark.gpu
W, H, F = 1280, 960, 40


@pytest.fixture(scope="module")
def survey():
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    ctx = im.Context(0)
    frames, A, gains, ws = render_frames(ctx, torch, F, W, H, per_row=10)
    for k in range(F):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), W, H, ws)
    feats = [ctx.GetFeatures(k) for k in range(F)]
    rng = np.random.default_rng(11)
    extra = {}
    kp0, d0 = feats[0]
    sel = rng.choice(len(kp0), 5, replace=False)
    extra[100] = (kp0[sel].copy(), d0[sel].copy())                              # 5 keypoints
    extra[101] = (kp0[:0].copy(), d0[:0].copy())                                # none
    kp1, d1 = feats[1]
    kt = kp1[:700].copy()
    kt["response"] = (rng.integers(0, 4, len(kt)) + 1) / 4.0                   # 4 response values: ties across every K boundary
    extra[102] = (kt, d1[:700].copy())
    for i, (k, d) in extra.items():
        ctx.SetFeatures(i, k, d, W, H)
    yield ctx, frames, feats, extra
    ctx.close()


def dev_scores(ctx, ids, **params):
    import torch
    n = len(ids)
    d = torch.empty((n, n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.ScreenScoresDev(ids, d.data_ptr(), **params)
    return d.cpu().numpy()


def ref_lists(feats_by_id, ids, top_k):
    return [sr.top_list(feats_by_id[i][0], feats_by_id[i][1], top_k) for i in ids]


@pytest.mark.parametrize("top_k", [32, 160, 256, 512])
def test_scores_equal_restatement(survey, top_k):
    ctx, _, feats, extra = survey
    ids = list(range(F)) + sorted(extra)
    by_id = {i: feats[i] for i in range(F)}
    by_id.update(extra)
    lists = ref_lists(by_id, ids, top_k)
    for ratio in (80, 100):
        got = dev_scores(ctx, ids, top_k=top_k, ratio_pct=ratio)
        want = sr.score_matrix(lists, ratio)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"top_k {top_k} ratio {ratio}: {len(bad)} scores differ, first {[(int(a), int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:5]]}"
    assert (got[:F, :F][~np.eye(F, dtype=bool)] >= 0).all() and (np.diag(got) == -1).all()
    assert (got[F + 1] == np.where(np.arange(len(ids)) == F + 1, -1, 0)).all()          # the empty frame scores 0


def test_scores_keepall_frames_more_than_2048(survey):
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    p = im.default_params()
    p.nfeatures = 0
    ctx = im.Context(0, p)
    ctx.set_option("keepall_max", 131072)
    frames, _, _, ws = render_frames(ctx, torch, 3, 2560, 1920, per_row=3)
    for k in range(3):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), 2560, 1920, ws)
    feats = {k: ctx.GetFeatures(k, max_kp=131072) for k in range(3)}
    ns = [len(feats[k][0]) for k in range(3)]
    assert max(ns) > 2048, ns
    r = feats[0][0]["response"]
    assert not (np.diff(r) <= 0).all(), "a keep-all frame in response order shows nothing"
    for top_k in (256, 512):
        got = dev_scores(ctx, [0, 1, 2], top_k=top_k, ratio_pct=80)
        want = sr.score_matrix(ref_lists(feats, [0, 1, 2], top_k), 80)
        assert np.array_equal(got, want), (top_k, got, want)
        assert got[0, 1] > 0
    ctx.close()


def _match(ctx, pairs, seed=5):
    return ctx.MatchPairs(np.asarray(pairs, np.int32).reshape(-1, 2), 2.5, seed)


def test_unordered_survey(survey):
    import imagemosaicing_amd as im
    ctx = survey[0]
    perm = np.random.default_rng(2024).permutation(F).astype(np.int32)        # position -> image id
    win = im.pair_schedule(F, 3)
    rw = _match(ctx, perm[win])
    assert int(im.select_connected_results(rw[rw["accepted"] == 1], F).sum()) < F, "a window over the shuffled order connects the survey"
    scr = ctx.ScreenPairs(perm, window=0)
    rs = _match(ctx, scr)
    assert int(im.select_connected_results(rs[rs["accepted"] == 1], F).sum()) == F
    allp = im.pair_schedule(F, F)                                                # every a < b
    assert len(allp) == 780
    ra = _match(ctx, perm[allp])
    strong = {(int(r["i"]), int(r["j"])) for r in ra if r["accepted"] == 1 and r["n_in"] >= 60}
    got = {(int(i), int(j)) for i, j in scr}
    assert strong and strong <= got, sorted(strong - got)
    by = {(int(r["i"]), int(r["j"])): r for r in ra}
    for r in rs:
        assert r.tobytes() == by[(int(r["i"]), int(r["j"]))].tobytes()
    print("unordered survey: screened", len(scr), "of 780; strong", len(strong), "accepted", int((ra["accepted"] == 1).sum()))


def _positions(ids, pairs):
    pos = {int(v): k for k, v in enumerate(ids)}
    return np.array([[pos[int(i)], pos[int(j)]] for i, j in pairs], np.int64).reshape(-1, 2)


def test_schedule_form(survey):
    import imagemosaicing_amd as im
    ctx, _, feats, _ = survey
    perm = np.random.default_rng(7).permutation(F).astype(np.int32)
    pairs, scores = ctx.ScreenPairs(perm, return_scores=True)
    pos = _positions(perm, pairs)
    assert (pos[:, 0] < pos[:, 1]).all()
    assert [tuple(p) for p in pos.tolist()] == sorted(tuple(p) for p in pos.tolist())
    S = dev_scores(ctx, perm)
    assert np.array_equal(scores, S[pos[:, 0], pos[:, 1]])
    d = im.screen_params()
    for partners, min_score, window in [(d.partners, d.min_score, 0), (3, 0, 0), (0, 10, 0), (2, 5, 7), (1, 40, 0)]:
        got = _positions(perm, ctx.ScreenPairs(perm, window=window, partners=partners, min_score=min_score))
        Sw = dev_scores(ctx, perm, window=window)
        want = sr.select_pairs(Sw, partners, min_score, window)
        assert np.array_equal(got, want), (partners, min_score, window)
    # window mode: a subset of the window schedule
    w5 = _positions(perm, ctx.ScreenPairs(perm, window=5, partners=2, min_score=0))
    sched = {tuple(p) for p in im.pair_schedule(F, 5).tolist()}
    assert len(w5) and {tuple(p) for p in w5.tolist()} <= sched
    # rank shards partition the world-1 list
    one = ctx.ScreenPairs(perm)
    shards = [ctx.ScreenPairs(perm, rank=r, world=3) for r in range(3)]
    for r, s in enumerate(shards):
        assert (_positions(perm, s)[:, 0] % 3 == r).all()
    assert sorted(map(tuple, np.concatenate(shards).tolist())) == sorted(map(tuple, one.tolist()))
    # a second context with the same features gives the same scores
    ctx2 = im.Context(0)
    for k in range(F):
        ctx2.SetFeatures(k, feats[k][0], feats[k][1], W, H)
    assert np.array_equal(dev_scores(ctx2, perm), S)
    assert np.array_equal(ctx2.ScreenPairs(perm), one)
    ctx2.close()
    # max_pairs too small: ERR_ARG with the count
    ids = np.ascontiguousarray(perm, np.int32)
    p = im.screen_params()
    buf = np.zeros((4, 2), np.int32)
    n = C.c_int(0)
    rc = ctx.L.mi355_screen_pairs(ctx._h, ids.ctypes.data_as(C.c_void_p), len(ids), C.byref(p), 0, 1, buf.ctypes.data_as(C.c_void_p), None, 1, C.byref(n))
    assert rc == -1 and n.value == len(one)
    assert np.array_equal(buf[:1], one[:1]) and (buf[1:] == 0).all()


def test_argument_errors(survey):
    import imagemosaicing_amd as im
    ctx = survey[0]
    cases = [
        (dict(img_ids=[0, 1, 9999]), "9999"),
        (dict(img_ids=[0, 1, 2, 1]), "duplicate img_id 1"),
        (dict(top_k=48), "top_k=48"),
        (dict(top_k=0), "top_k=0"),
        (dict(top_k=544), "top_k=544"),
        (dict(window=1), "window=1"),
        (dict(rank=3, world=3), "rank=3"),
        (dict(rank=0, world=0), "world=0"),
    ]
    for kw, msg in cases:
        ids = kw.pop("img_ids", list(range(5)))
        with pytest.raises(im.Mi355Error) as e:
            ctx.ScreenPairs(ids, **kw)
        assert e.value.code == -1 and msg in str(e.value), (kw, str(e.value))
    import torch
    d = torch.empty((3, 3), dtype=torch.int32, device="cuda")
    for kw, msg in [(dict(top_k=33), "top_k=33"), (dict(window=1), "window=1")]:
        with pytest.raises(im.Mi355Error) as e:
            ctx.ScreenScoresDev([0, 1, 2], d.data_ptr(), **kw)
        assert msg in str(e.value)
    with pytest.raises(im.Mi355Error) as e:
        ctx.ScreenScoresDev([0, 7777, 2], d.data_ptr())
    assert "7777" in str(e.value)


def test_c4_screened_window_182():
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    ctx = im.Context(0)
    w, h, n = 4000, 3000, 500
    frames, _, _, ws = render_frames(ctx, torch, n, w, h)
    for k in range(n):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), w, h, ws)
    del frames
    ids = np.arange(n, dtype=np.int32)
    win = im.pair_schedule(n, 182)
    assert len(win) == 74029
    scr = ctx.ScreenPairs(ids, window=182)
    assert {tuple(p) for p in scr.tolist()} <= {tuple(p) for p in win.tolist()}
    seed = 17
    rw = ctx.MatchPairs(win, 2.5, seed)
    rs = ctx.MatchPairs(scr, 2.5, seed)
    acc_w = {(int(r["i"]), int(r["j"])) for r in rw if r["accepted"] == 1}
    strong = {(int(r["i"]), int(r["j"])) for r in rw if r["accepted"] == 1 and r["n_in"] >= 60}
    got = {tuple(p) for p in scr.tolist()}
    recall = len(acc_w & got) / len(acc_w)
    print("C4 screen: list", len(scr), "fraction", len(scr) / 74029, "recall", recall, "window accepted", len(acc_w))
    assert strong <= got, sorted(strong - got)[:10]
    assert recall >= 0.97, recall
    assert len(scr) <= 0.15 * 74029, len(scr)
    label = im.select_connected_results(rs[rs["accepted"] == 1], n)
    assert int(label.sum()) == n
    ctx.close()

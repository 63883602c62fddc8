"""GPU: keep-all SIFT (nfeatures <= 0) beyond 32 768 keypoints per frame, through the per-context ceiling "keepall_max" (a multiple of 2048 in
[32768, 262144], default 32768).

  * a 4000x3000 survey frame extracts bit for bit like the oracle's keep-all list, through the host form and a device batch of two frames;
  * a ctx that never sets the option behaves as before: the survey frame fails, naming the ceiling, and the reference's frame is unchanged;
  * the option's contract: bad values and a ceiling below a resident frame are rejected, mi355_set_features follows the ceiling;
  * the pair stage beyond 32 768 rows: 1-NN / 2-NN, the sorted list, SelectMatchPairs and the whole MatchPairs record against the oracle,
    mixed batches and runs split by the sub-pair bound equal to each pair alone;
  * the chunk exchange of a 70 000-keypoint frame (35 records), into a ctx with and without the option, and the RCCL world-1 collective.
"""
import os

import numpy as np
import pytest

from tests.golden_util import GOLD

pytestmark = pytest.mark.gpu
KMAX = 131072
W, H = 4000, 3000


def keepall_ctx(kmax=None):
    import imagemosaicing_amd as im
    p = im.default_params()
    p.nfeatures = 0
    ctx = im.Context(0, p)
    if kmax:
        ctx.set_option("keepall_max", kmax)
    return ctx


def golden_frame(name):
    PIL = pytest.importorskip("PIL.Image")
    return np.ascontiguousarray(np.array(PIL.open(os.path.join(GOLD, name)).convert("RGB"))[:, :, ::-1])


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 128)).astype(np.uint8)


def rand_kp(rng, n):
    from imagemosaicing_amd import KEYPOINT
    kp = np.zeros(n, KEYPOINT)
    kp["x"] = rng.uniform(40, W - 40, n); kp["y"] = rng.uniform(40, H - 40, n)      # + (30, -20) (_plant) stays inside
    kp["size"] = rng.uniform(2, 20, n); kp["angle"] = rng.uniform(0, 360, n); kp["response"] = rng.uniform(0, 1, n)
    kp["octave"] = rng.integers(0, 1 << 20, n); kp["class_id"] = -1
    return kp


def same_bytes(a, b):
    return np.array_equal(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8), np.frombuffer(np.ascontiguousarray(b).tobytes(), np.uint8))


def test_survey_frame_keepall_bit_for_bit():
    import torch
    from tests import oracle_lib as ol
    from tests.synth_survey import render_frames, host_image
    orc = ol.load_oracle_fast()
    ctx = keepall_ctx(KMAX)
    frames, _, _, ws = render_frames(ctx, torch, 2, W, H)
    imgs = [host_image(frames, k, W, H, ws) for k in range(2)]
    want = ol.parallel_map(lambda im: orc.sift(im, nfeatures=0, max_kp=KMAX), imgs)
    for k in range(2):                                   # one device batch of two frames
        ctx.SiftExtractDev(k, frames[k].data_ptr(), W, H, ws)
    dev = [ctx.GetFeatures(k, max_kp=KMAX) for k in range(2)]
    kh, dh = ctx.SiftExtract(10, imgs[0], max_kp=KMAX)   # the host form
    for tag, (kp, d), (okp, od) in (("dev 0", dev[0], want[0]), ("dev 1", dev[1], want[1]), ("host 0", (kh, dh), want[0])):
        assert 32768 < len(okp) < KMAX, (tag, len(okp))
        assert len(kp) == len(okp), (tag, len(kp), len(okp))
        assert np.array_equal(kp.view(np.uint8), okp.view(np.uint8)), f"{tag}: keep-all keypoints differ from the oracle's"
        assert np.array_equal(d.astype(np.uint8), od), f"{tag}: keep-all descriptors differ from the oracle's"
    ctx.close()


def test_default_ctx_unchanged():
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    ctx = keepall_ctx()
    frames, _, _, ws = render_frames(ctx, torch, 1, W, H)
    with pytest.raises(im.Mi355Error) as e:
        ctx.SiftExtractDev(0, frames[0].data_ptr(), W, H, ws, want_count=True)
    assert "keepall_max=32768" in str(e.value) and "overflow" not in str(e.value), str(e.value)
    c = ctx.last_sift_counters()
    assert c[2] > 32768 and c[4] == 0, c                 # oriented keypoints above the ceiling; no buffer overflowed
    # raised and lowered again: the reference's frame equals a fresh default ctx's, byte for byte
    img = golden_frame("DSC00004.JPG")
    ctx.set_option("keepall_max", 262144)
    ctx.set_option("keepall_max", 32768)
    kp, d = ctx.SiftExtract(1, img, max_kp=32768)
    fresh = keepall_ctx()
    kf, df = fresh.SiftExtract(1, img, max_kp=32768)
    assert 2048 < len(kp) < 32768
    assert same_bytes(kp, kf) and np.array_equal(d, df)
    fresh.close()
    ctx.close()


def test_option_contract():
    import imagemosaicing_amd as im
    rng = np.random.default_rng(3)
    ctx = im.Context(0)
    kp, d = rand_kp(rng, 40000), rand_desc(rng, 40000).astype(np.float32)
    for bad in (32767, 270336, 40000, 0, -2048):
        with pytest.raises(im.Mi355Error):
            ctx.set_option("keepall_max", bad)
    with pytest.raises(im.Mi355Error) as e:              # still the default after the rejected values
        ctx.SetFeatures(1, kp, d, W, H)
    assert "32768" in str(e.value)
    ctx.set_option("keepall_max", 40960)
    ctx.SetFeatures(1, kp, d, W, H)
    with pytest.raises(im.Mi355Error) as e:
        ctx.set_option("keepall_max", 32768)             # below the 40 000 rows of image 1
    assert "image 1" in str(e.value), str(e.value)
    k1, d1 = ctx.GetFeatures(1, max_kp=40960)            # unchanged, and the ceiling still 40960
    assert same_bytes(k1, kp) and np.array_equal(d1, d)
    ctx.SetFeatures(2, kp[:32769], d[:32769], W, H)
    ctx.DropFeatures(1); ctx.DropFeatures(2)
    ctx.set_option("keepall_max", 32768)
    with pytest.raises(im.Mi355Error):
        ctx.SetFeatures(1, kp, d, W, H)
    ctx.close()


def _plant(rng, d1, kp1, d2, kp2, n):
    """n exact correspondences: query q has train t's descriptor at t's position + (30, -20)"""
    q = rng.choice(len(d1), n, replace=False)
    t = rng.choice(len(d2), n, replace=False)
    d1[q] = d2[t]
    kp1["x"][q] = kp2["x"][t] + 30.0; kp1["y"][q] = kp2["y"][t] - 20.0


def _record_equals_oracle(r, orc, kp1, d1, kp2, d2, seed, tag):
    nin, i1, i2, Ho, ns = orc.match_pair(np.stack([kp1["x"], kp1["y"]], 1), d1, np.stack([kp2["x"], kp2["y"]], 1), d2, W, H, 2.5, seed)
    assert ns == int(r["n_selected"]), (tag, int(r["n_selected"]), ns)
    acc = nin > 30
    assert int(r["accepted"]) == int(acc), (tag, int(r["accepted"]), nin)
    if acc:
        assert nin == int(r["n_in"]), (tag, int(r["n_in"]), nin)
        assert np.array_equal(r["a"][:nin], i1[:nin]) and np.array_equal(r["b"][:nin], i2[:nin]), f"{tag}: inliers differ"
        assert np.array_equal(r["H"].view(np.uint32), Ho.view(np.uint32)), f"{tag}: H bits differ"
    return acc


def test_pair_stage_beyond_32768():
    import imagemosaicing_amd as im
    from tests import oracle_lib as ol
    orc = ol.load_oracle_fast()
    rng = np.random.default_rng(11)
    ctx = im.Context(0)
    ctx.set_option("keepall_max", KMAX)
    sets = {}
    for (a, b, n1, n2) in [(100, 101, 40000, 2500), (102, 103, 2500, 70000), (104, 105, 100000, 600)]:
        d1, d2 = rand_desc(rng, n1), rand_desc(rng, n2)
        kp1, kp2 = rand_kp(rng, n1), rand_kp(rng, n2)
        _plant(rng, d1, kp1, d2, kp2, 300)
        if n2 > 2100:
            d2[2050] = d2[3]; d1[0] = d2[3]                 # an exact tie between two train chunks: the lower index wins
            d2[n2 - 1] = d2[2047]; d1[1] = d2[2047]         # ... the last row of chunk 0 against the very last row
        if n2 > 40000:
            d2[36000] = d2[9]; d1[2] = d2[9]                # ... across the old 32 768 boundary
        if n1 > 2100:
            d1[2100] = d1[5]                                # equal distances for two queries of different query chunks: order by queryIdx
        if n1 > 40000:
            d1[n1 - 1] = d1[6]; d1[33000] = d1[6]           # ... beyond 32 768
        ctx.SetFeatures(a, kp1, d1.astype(np.float32), W, H)
        ctx.SetFeatures(b, kp2, d2.astype(np.float32), W, H)
        sets[(a, b)] = (kp1, d1, kp2, d2)
    accepted = 0
    for (a, b), (kp1, d1, kp2, d2) in sets.items():
        n1 = len(d1)
        idx, b1, b2 = orc.bf_match(d1, d2)
        m, g1, g2 = ctx.BFMatch(a, b, sorted_=False, max_matches=n1)
        assert len(m) == n1
        assert np.array_equal(m["trainIdx"], idx) and np.array_equal(g1, b1) and np.array_equal(g2, b2), (a, b)
        ms, _, _ = ctx.BFMatch(a, b, sorted_=True, max_matches=n1)
        want = orc.sort_matches(idx, b1)
        assert np.array_equal(np.stack([ms["queryIdx"], ms["trainIdx"]], 1), want), (a, b)
        xy1, xy2 = np.stack([kp1["x"], kp1["y"]], 1), np.stack([kp2["x"], kp2["y"]], 1)
        a1, a2 = ctx.SelectMatchPairs(want, xy1, xy2, 400, W, H)
        o1, o2 = orc.select(want, xy1, xy2, 400, W, H)
        assert len(a1) == len(o1) and np.array_equal(a1, o1) and np.array_equal(a2, o2), (a, b)
        r = ctx.MatchPairs([(a, b)], 2.5, 3)[0]
        accepted += _record_equals_oracle(r, orc, kp1, d1, kp2, d2, 3, (a, b))
    assert accepted >= 1
    # a batch mixing <= 2048, <= 32 768 and > 32 768 pairs: every record equals the pair's record alone
    ctx.SetFeatures(106, rand_kp(rng, 1500), rand_desc(rng, 1500).astype(np.float32), W, H)
    ctx.SetFeatures(107, rand_kp(rng, 9000), rand_desc(rng, 9000).astype(np.float32), W, H)
    mixed = [(106, 106), (100, 101), (106, 107), (107, 103), (104, 105), (106, 101), (102, 103), (101, 100)]
    together = ctx.MatchPairs(mixed, 2.5, 5)
    alone = [ctx.MatchPairs([p], 2.5, 5)[0] for p in mixed]
    for p, r, s in zip(mixed, together, alone):
        assert same_bytes(r, s), p
    # the same batch in runs split by the sub-pair bound (one pair per run where a pair alone exceeds it)
    ctx.set_option("big_subpairs_max", 40)
    split = ctx.MatchPairs(mixed, 2.5, 5)
    ctx.set_option("big_subpairs_max", 65536)
    assert same_bytes(split, together)
    ctx.close()


def test_exchange_70000_keypoints():
    import torch
    import imagemosaicing_amd as im
    from imagemosaicing_amd import dist as md
    rng = np.random.default_rng(5)
    src = keepall_ctx(KMAX)
    kp7, d7 = rand_kp(rng, 70000), rand_desc(rng, 70000)
    kp8, d8 = rand_kp(rng, 2500), rand_desc(rng, 2500)
    _plant(rng, d7, kp7, d8, kp8, 300)
    src.SetFeatures(7, kp7, d7.astype(np.float32), W, H)
    src.SetFeatures(8, kp8, d8.astype(np.float32), W, H)
    assert src.FeatureChunkCount([7]) == 35
    pay = torch.empty((37, im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    hdr = src.PackFeatureChunksDev([7, 8], pay.data_ptr(), 37)        # 35 + 2 records
    assert len(hdr) == 37 and int(hdr["n_kp"][0]) == 70000 and int(hdr["n_chunks"][0]) == 35
    pairs = [(8, 7), (7, 8)]
    rec = src.MatchPairs(pairs, 2.5, 3)
    assert int(rec[0]["accepted"]) == 1
    # into a second ctx with the option: the same bytes, the same records
    dst = keepall_ctx(KMAX)
    dst.InstallFeatureChunksDev(hdr, pay.data_ptr())
    for k in (7, 8):
        a, b = src.GetFeatures(k, max_kp=KMAX), dst.GetFeatures(k, max_kp=KMAX)
        assert same_bytes(a[0], b[0]) and np.array_equal(a[1], b[1]), k
    assert same_bytes(dst.MatchPairs(pairs, 2.5, 3), rec)
    dst.close()
    # into a default ctx: refused, naming the ceiling in force, nothing changed
    dflt = keepall_ctx()
    dflt.SetFeatures(8, kp8[:100], d8[:100].astype(np.float32), W, H)
    before = dflt.GetFeatures(8, max_kp=32768)
    with pytest.raises(im.Mi355Error) as e:
        dflt.InstallFeatureChunksDev(hdr, pay.data_ptr())
    assert "32768" in str(e.value), str(e.value)
    after = dflt.GetFeatures(8, max_kp=32768)
    assert same_bytes(after[0], before[0]) and np.array_equal(after[1], before[1])
    with pytest.raises(im.Mi355Error):
        dflt.GetFeatures(7)
    dflt.close()
    # RCCL, one rank: the collective over the 70 000-keypoint frame and a reference frame leaves features and records unchanged
    src.SiftExtract(100, golden_frame("DSC00004.JPG"), max_kp=KMAX)
    src.SiftExtract(101, golden_frame("DSC00005.JPG"), max_kp=KMAX)
    ids = [7, 100, 8, 101]
    assert im.comm_available()
    ex = md.Exchange(src, "rccl")
    pairs = [(8, 7), (100, 101), (7, 100)]
    before = [src.GetFeatures(k, max_kp=KMAX) for k in ids]
    rec0 = src.MatchPairs(pairs, 2.5, 5)
    src.AllGatherFeatureChunks(ids, install_own=True)
    for k, (kp, d) in zip(ids, before):
        kp1, d1 = src.GetFeatures(k, max_kp=KMAX)
        assert same_bytes(kp1, kp) and np.array_equal(d1, d), k
    assert same_bytes(src.MatchPairs(pairs, 2.5, 5), rec0), "pair records changed after the collective"
    ex.close()
    src.close()

"""GPU: the chunk-record feature exchange (mi355_pack_feature_chunks_dev / mi355_install_feature_chunks_dev / mi355_allgather_feature_chunks),
which carries frames of any keypoint count -- keep-all frames (nfeatures <= 0) hold up to 32 768 -- between ranks.

  * pack on one ctx, install on a second ctx of the same device: the installed features equal the source byte for byte, and the matcher
    (mi355_bf_match, mi355_match_pairs, both the <= 2048 path and the large-pair path) gives the same bytes on both contexts;
  * the record layout: chunk c holds rows [2048 c, 2048 c + rows), zeros elsewhere; a frame of <= 2048 keypoints is one chunk, byte for byte
    mi355_pack_features_dev's record;
  * malformed tables raise and change nothing, the fixed form's included (a bad header, an image named twice);
  * one layout, two headers: records packed by the fixed form install through the chunk form and the other way round, at frame sizes around
    the 256-row padding and the 2048-row record; a smaller frame installed over a larger one leaves no stale padding rows;
  * RCCL, a communicator of one rank: the collective over keep-all frames, re-installing the rank's own frames, leaves features and pair
    records as they were; an unknown id fails and the communicator still works.
"""
import os

import numpy as np
import pytest

from tests.golden_util import GOLD

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2047, 2048, 2049, 4097, 32768]      # image id k has SIZES[k] keypoints
W, H = 4000, 3000
PAIRS = [(2, 4), (3, 4), (4, 5), (5, 6), (6, 2), (1, 3), (3, 2), (6, 4)]


def synth_features(n, k):
    """n keypoints of image k: rows of one shared pool (so that every pair of images has exact matches), translated by (7 k, -5 k)"""
    rng = np.random.default_rng(77)
    pool_d = rng.integers(0, 256, (32768, 128)).astype(np.float32)
    pool_xy = rng.uniform(100.0, [W - 100.0, H - 100.0], (32768, 2)).astype(np.float32)
    import imagemosaicing_amd as im
    kp = np.zeros(n, im.KEYPOINT)
    kp["x"] = pool_xy[:n, 0] + 7.0 * k; kp["y"] = pool_xy[:n, 1] - 5.0 * k
    r2 = np.random.default_rng(k)
    kp["size"] = r2.uniform(2, 20, n); kp["angle"] = r2.uniform(0, 360, n); kp["response"] = r2.uniform(0, 1, n)
    kp["octave"] = r2.integers(0, 1 << 20, n); kp["class_id"] = -1
    return kp, pool_d[:n].copy()


def golden_frame(name):
    PIL = pytest.importorskip("PIL.Image")
    return np.ascontiguousarray(np.array(PIL.open(os.path.join(GOLD, name)).convert("RGB"))[:, :, ::-1])


def keepall_params():
    import imagemosaicing_amd as im
    p = im.default_params()
    p.nfeatures = 0
    return p


def same_features(a, b, ids):
    for k in ids:
        ka, da = a.GetFeatures(k, max_kp=32768)
        kb, db = b.GetFeatures(k, max_kp=32768)
        assert len(ka) == len(kb), k
        assert np.array_equal(ka.view(np.uint8), kb.view(np.uint8)) and np.array_equal(da, db), f"image {k}: features differ"


@pytest.fixture(scope="module")
def src():
    """ctx A: the synthetic frames 0..6 and the reference's frames DSC00004 / DSC00005 extracted with keep-all as images 100 / 101"""
    import imagemosaicing_amd as im
    a = im.Context(0, keepall_params())
    for k, n in enumerate(SIZES):
        kp, d = synth_features(n, k)
        a.SetFeatures(k, kp, d, W, H)
    for k, name in ((100, "DSC00004.JPG"), (101, "DSC00005.JPG")):
        kp, _ = a.SiftExtract(k, golden_frame(name), max_kp=32768)
        assert 2048 < len(kp) <= 4096                 # about 2 900: two chunks each
    yield a
    a.close()


def test_pack_install_round_trip_and_layout(src):
    import torch
    import imagemosaicing_amd as im
    ids = list(range(len(SIZES))) + [100, 101]
    n_kp = [len(src.GetFeatures(k, max_kp=32768)[0]) for k in ids]
    want = sum(max(1, -(-n // 2048)) for n in n_kp)
    assert src.FeatureChunkCount(ids) == want == 1 + 1 + 1 + 1 + 2 + 3 + 16 + 2 + 2
    pay = torch.empty((want, im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    hdr = src.PackFeatureChunksDev(ids, pay.data_ptr(), want)
    assert len(hdr) == want
    # headers: every image's chunks in order, 2048-row windows
    q = 0
    for k, n in zip(ids, n_kp):
        nc = max(1, -(-n // 2048))
        for c in range(nc):
            assert tuple(hdr[q]) == (k, n, W if k < 100 else 1000, H if k < 100 else 750, c, nc, 2048 * c, min(2048, n - 2048 * c)), (k, c, hdr[q])
            q += 1
    # the payload: rows of the window, zeros elsewhere (image 5, 4097 keypoints: 2048 + 2048 + 1 rows)
    p = pay.cpu().numpy()
    kp5, d5 = src.GetFeatures(5, max_kp=32768)
    for r in np.flatnonzero(hdr["img_id"] == 5):
        r0, rows = int(hdr["row0"][r]), int(hdr["rows"][r])
        assert np.array_equal(p[r, :rows * 28], kp5[r0:r0 + rows].view(np.uint8).reshape(-1))
        assert np.array_equal(p[r, 57344:57344 + rows * 128], d5[r0:r0 + rows].astype(np.uint8).reshape(-1))
        assert not p[r, rows * 28:57344].any() and not p[r, 57344 + rows * 128:].any()
    # a frame of <= 2048 keypoints is one chunk: byte for byte the fixed record
    small = [0, 1, 2, 3]
    fixed = torch.empty((len(small), im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    fh = src.PackFeaturesDev(small, fixed.data_ptr())
    fx = fixed.cpu().numpy()
    for q, k in enumerate(small):
        r = int(np.flatnonzero(hdr["img_id"] == k)[0])
        assert np.array_equal(p[r], fx[q]), k
        assert tuple(fh[q]) == tuple(hdr[r])[:4]
    # install on a second ctx: the same features
    dst = im.Context(0, keepall_params())
    dst.InstallFeatureChunksDev(hdr, pay.data_ptr())
    same_features(src, dst, ids)
    dst.close()


def test_matcher_equal_after_install(src):
    import torch
    import imagemosaicing_amd as im
    ids = list(range(len(SIZES))) + [100, 101]
    n = src.FeatureChunkCount(ids)
    pay = torch.empty((n, im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    hdr = src.PackFeatureChunksDev(ids, pay.data_ptr(), n)
    dst = im.Context(0, keepall_params())
    dst.InstallFeatureChunksDev(hdr, pay.data_ptr())
    for i, j in PAIRS + [(100, 101)]:
        a, b = src.BFMatch(i, j, True, 32768), dst.BFMatch(i, j, True, 32768)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (i, j)
    pairs = PAIRS + [(100, 101), (101, 100)]
    ra, rb = src.MatchPairs(pairs, 2.5, 3), dst.MatchPairs(pairs, 2.5, 3)
    assert np.array_equal(ra.view(np.uint8), rb.view(np.uint8)), "pair records differ after the chunk install"
    acc = {(int(r["i"]), int(r["j"])) for r in ra if r["accepted"]}
    assert {(2, 4), (4, 5), (5, 6), (6, 4), (100, 101)} <= acc, acc     # pairs across the 2048-row boundary, and the reference's frames
    dst.close()


def test_malformed_tables_raise_and_change_nothing(src):
    import torch
    import imagemosaicing_amd as im
    dst = im.Context(0)
    # image 500 on dst: the features of image 4 (2049 keypoints)
    p4 = torch.empty((2, im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    h4 = src.PackFeatureChunksDev([4], p4.data_ptr(), 2)
    h4["img_id"] = 500
    dst.InstallFeatureChunksDev(h4, p4.data_ptr())
    before = dst.GetFeatures(500, max_kp=32768)
    # a table: image 2 (2047 keypoints, valid) as 500 + image 5 (4097 keypoints, 3 chunks) as 501
    pay = torch.empty((4, im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    good = src.PackFeatureChunksDev([2, 5], pay.data_ptr(), 4)
    good["img_id"] = [500, 501, 501, 501]

    def broken(field, rows, value):
        h = good.copy()
        h[field][rows] = value
        return h

    cases = {
        "missing chunk": broken("img_id", 2, -1),
        "duplicate chunk": broken("chunk", 3, 1),
        "disagreeing n_kp": broken("n_kp", 2, 4096),
        "rows do not tile": broken("rows", 1, 2047),
        "n_kp > 32768": broken("n_kp", slice(1, 4), 40000),
    }
    for name, h in cases.items():
        with pytest.raises(im.Mi355Error) as e:
            dst.InstallFeatureChunksDev(h, pay.data_ptr())
        assert "501" in str(e.value), (name, str(e.value))
        if name == "n_kp > 32768":
            assert "32768" in str(e.value)
        after = dst.GetFeatures(500, max_kp=32768)
        assert np.array_equal(after[0].view(np.uint8), before[0].view(np.uint8)) and np.array_equal(after[1], before[1]), name
        with pytest.raises(im.Mi355Error):
            dst.GetFeatures(501)                      # not created either
    # too few records for the pack: an error, nothing written
    pay.fill_(0xAB)
    torch.cuda.synchronize()
    with pytest.raises(im.Mi355Error):
        src.PackFeatureChunksDev([2, 5], pay.data_ptr(), 3)
    assert bool((pay == 0xAB).all())
    # the good table still installs
    src.PackFeatureChunksDev([2, 5], pay.data_ptr(), 4)
    dst.InstallFeatureChunksDev(good, pay.data_ptr())
    k2, d2 = src.GetFeatures(2, max_kp=32768)
    k500, d500 = dst.GetFeatures(500, max_kp=32768)
    assert np.array_equal(k2.view(np.uint8), k500.view(np.uint8)) and np.array_equal(d2, d500)
    dst.close()


def test_rccl_collective_world1_keepall(src):
    import torch
    import imagemosaicing_amd as im
    from imagemosaicing_amd import dist as md
    ctx = im.Context(0, keepall_params())
    for k in (4, 5, 1):
        kp, d = src.GetFeatures(k, max_kp=32768)
        ctx.SetFeatures(k, kp, d, W, H)
    for k, name in ((100, "DSC00004.JPG"), (101, "DSC00005.JPG")):
        ctx.SiftExtract(k, golden_frame(name), max_kp=32768)
    ids = [100, 101, 4, 5, 1]
    assert im.comm_available()
    ex = md.Exchange(ctx, "rccl")
    assert ctx.CommInfo() == (0, 1)
    pairs = [(100, 101), (4, 5), (1, 4), (101, 5)]
    before = [ctx.GetFeatures(k, max_kp=32768) for k in ids]
    rec0 = ctx.MatchPairs(pairs, 2.5, 5)
    ctx.AllGatherFeatureChunks(ids, install_own=True)            # every frame through ncclAllGather and the install kernel
    for k, (kp, d) in zip(ids, before):
        kp1, d1 = ctx.GetFeatures(k, max_kp=32768)
        assert np.array_equal(kp1.view(np.uint8), kp.view(np.uint8)) and np.array_equal(d1, d), k
    rec1 = ctx.MatchPairs(pairs, 2.5, 5)
    assert np.array_equal(rec0.view(np.uint8), rec1.view(np.uint8)), "pair records changed after the collective"
    assert int(rec1[0]["accepted"]) == 1
    ex.allgather_features(ids, None, "cuda", chunked=True)       # the Exchange form (own frames skipped)
    with pytest.raises(im.Mi355Error):
        ctx.AllGatherFeatureChunks([100, 77])                     # image 77 has no features: the rank reports it through the status word
    ctx.AllGatherFeatureChunks([101, 4], install_own=True)       # the communicator still works
    ctx.AllGatherFeatures([1], 1)                                 # and so does the fixed-record collective
    rec2 = ctx.MatchPairs(pairs, 2.5, 5)
    assert np.array_equal(rec0.view(np.uint8), rec2.view(np.uint8))
    ex.close()
    ctx.close()


# ---- one layout, two headers: the fixed record is the chunk {row0 0, rows n_kp} --------------------------------------------------------------
EDGE = [0, 1, 255, 256, 257, 2047, 2048]          # image id k has EDGE[k] keypoints: around the 256-row padding and the 2048-row record
EDGE_PAIRS = [(6, 5), (5, 6), (4, 6), (6, 4), (3, 4), (2, 3), (1, 6), (6, 1), (4, 2)]


@pytest.fixture(scope="module")
def edge():
    """a ctx with the synthetic frames 0..6 of EDGE keypoints; their fixed and chunk packs (headers, payload on the device)"""
    import torch
    import imagemosaicing_amd as im
    a = im.Context(0)
    for k, n in enumerate(EDGE):
        kp, d = synth_features(n, k)
        a.SetFeatures(k, kp, d, W, H)
    ids = list(range(len(EDGE)))
    fixed = torch.empty((len(ids), im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    chunks = torch.empty((len(ids), im.FEATURE_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    fh = a.PackFeaturesDev(ids, fixed.data_ptr())
    ch = a.PackFeatureChunksDev(ids, chunks.data_ptr(), len(ids))
    assert len(ch) == len(ids) and torch.equal(fixed, chunks)
    yield a, ids, fh, fixed, ch, chunks
    a.close()


def as_chunk_headers(fh):
    import imagemosaicing_amd as im
    ch = np.zeros(len(fh), im.FEATURE_CHUNK_HEADER)
    for f in ("img_id", "n_kp", "w", "h"):
        ch[f] = fh[f]
    ch["n_chunks"] = 1
    ch["rows"] = fh["n_kp"]
    return ch


def as_fixed_headers(ch):
    import imagemosaicing_amd as im
    fh = np.zeros(len(ch), im.FEATURE_HEADER)
    for f in ("img_id", "n_kp", "w", "h"):
        fh[f] = ch[f]
    return fh


def same_matches(a, b, pairs):
    for i, j in pairs:
        for x, y in zip(a.BFMatch(i, j, True, 2048), b.BFMatch(i, j, True, 2048)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (i, j)
    ra, rb = a.MatchPairs(pairs, 2.5, 3), b.MatchPairs(pairs, 2.5, 3)
    assert np.array_equal(ra.view(np.uint8), rb.view(np.uint8)), "pair records differ"
    return ra


@pytest.mark.parametrize("form", ["fixed_pack_chunk_install", "chunk_pack_fixed_install"])
def test_cross_form_install(edge, form):
    import imagemosaicing_amd as im
    src, ids, fh, fixed, ch, chunks = edge
    assert [int(n) for n in fh["n_kp"]] == EDGE and np.array_equal(as_chunk_headers(fh), ch) and np.array_equal(as_fixed_headers(ch), fh)
    dst = im.Context(0)
    if form == "fixed_pack_chunk_install":
        dst.InstallFeatureChunksDev(as_chunk_headers(fh), fixed.data_ptr())
    else:
        dst.InstallFeaturesDev(as_fixed_headers(ch), chunks.data_ptr())
    same_features(src, dst, ids)
    rec = same_matches(src, dst, EDGE_PAIRS)
    assert int(rec[0]["accepted"]) == 1               # 2048 against 2047 rows of one pool
    dst.close()


def test_shrinking_reinstall_rewrites_the_padding_rows(edge):
    """257 keypoints, then 1 under the same id: the rows [1, 256) the matcher reads as padding must not keep the first frame's descriptors"""
    import imagemosaicing_amd as im
    src, ids, fh, fixed, ch, chunks = edge
    dst, fresh = im.Context(0), im.Context(0)
    h = fh[[4, 6]].copy()
    h["img_id"] = [7, 8]
    pay, pay1 = fixed[[4, 6]].contiguous(), fixed[[1]].contiguous()
    dst.InstallFeaturesDev(h, pay.data_ptr())
    h1 = fh[[1]].copy()
    h1["img_id"] = 7
    dst.InstallFeaturesDev(h1, pay1.data_ptr())
    for k, q in ((7, 1), (8, 6)):
        kp, d = src.GetFeatures(q)
        fresh.SetFeatures(k, kp, d, W, H)
    same_features(fresh, dst, [7, 8])
    same_matches(fresh, dst, [(7, 8), (8, 7)])
    dst.close(); fresh.close()


def test_fixed_table_is_checked_before_anything_changes(edge):
    import imagemosaicing_amd as im
    src, ids, fh, fixed, ch, chunks = edge
    dst = im.Context(0)
    for k, q in ((10, 2), (11, 4)):                   # what dst holds before: frames 2 and 4 as images 10 and 11
        kp, d = src.GetFeatures(q)
        dst.SetFeatures(k, kp, d, W, H)
    before = [dst.GetFeatures(k) for k in (10, 11)]
    pay = fixed[[1, 3, 5]].contiguous()
    good = fh[[1, 3, 5]].copy()
    good["img_id"] = [10, 11, 12]

    def broken(field, value):
        h = good.copy()
        h[field][2] = value
        return h

    for name, h in (("n_kp = 2049", broken("n_kp", 2049)), ("w = 0", broken("w", 0)), ("an image named twice", broken("img_id", 10))):
        with pytest.raises(im.Mi355Error):
            dst.InstallFeaturesDev(h, pay.data_ptr())
        for k, (kp, d) in zip((10, 11), before):
            kp1, d1 = dst.GetFeatures(k)
            assert len(kp1) == len(kp) and np.array_equal(kp1.view(np.uint8), kp.view(np.uint8)) and np.array_equal(d1, d), (name, k)
        with pytest.raises(im.Mi355Error):
            dst.GetFeatures(12)                       # not created either
    dst.InstallFeaturesDev(good, pay.data_ptr())      # the good table still installs
    for k, q in ((10, 1), (11, 3), (12, 5)):
        ka, da = src.GetFeatures(q)
        kb, db = dst.GetFeatures(k)
        assert np.array_equal(ka.view(np.uint8), kb.view(np.uint8)) and np.array_equal(da, db), k
    dst.close()

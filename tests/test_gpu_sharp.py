"""Frame sharpness on the GPU: sharp_stats_kernel (csrc/sharp.hip) against the numpy restatement (tests/sharp_ref.py) on every stats case of
tests/sharp_patterns.py at each of its steps, byte for byte; the records with and without per-frame tiles, on a second context and after an
interleaved gain statistics call; mi355_sharpness_dev against stats -> host solve -> host select; renders of the kept frames; one
end-to-end strip with a blurred frame; and the argument errors.  Frames are tens of pixels wide.
(tests/test_sharp_patterns_ref.py checks the cases and the restatement themselves, tests/test_sharp_host.py the host half, without a GPU.)
"""
import numpy as np
import pytest

from tests import sharp_patterns as sp
from tests import sharp_ref as sr

pytestmark = pytest.mark.gpu

CASES = sp.stats_cases()
IDS = [c.tag for c in CASES]
TAGS = {c.tag: c for c in CASES}
PAD_BYTE = 0xEE


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


_DEV = {}


def _upload(imgs, pads=None):
    """the frames on the device, rows padded by pads[k] bytes of PAD_BYTE: (tensors, ptrs, w, h, ws)"""
    import torch
    ts, ws = [], []
    for k, a in enumerate(imgs):
        h, w = a.shape[:2]
        pitch = 3 * w + (pads[k] if pads else 0)
        buf = np.full((h, pitch), PAD_BYTE, np.uint8)
        buf[:, :3 * w] = a.reshape(h, 3 * w)
        ts.append(torch.from_numpy(buf).cuda())
        ws.append(pitch)
    torch.cuda.synchronize()
    return ts, [t.data_ptr() for t in ts], [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], ws


def _frames(case):
    if case.tag not in _DEV:
        _DEV[case.tag] = _upload(case.render.imgs, case.pads)
    return _DEV[case.tag]


def _same(st, fs, ref_st, ref_fs, what):
    import imagemosaicing_amd as im
    assert st.dtype == im.SHARP_PAIR_STATS and len(st) == len(ref_st), what
    for i in range(len(st)):
        got, want = tuple(int(v) for v in st[i]), tuple(int(v) for v in ref_st[i])
        assert got == want, f"{what}: pair {i}: got (a, b, n, e_a, e_b, s_a, s_b) {got}, expected {want}"
    assert st.tobytes() == ref_st.tobytes(), what
    if fs is not None:
        for k in range(len(fs)):
            got, want = tuple(int(v) for v in fs[k]), tuple(int(v) for v in ref_fs[k])
            assert got == want, f"{what}: frame {k}: got (n, e, s) {got}, expected {want}"
        assert fs.tobytes() == ref_fs.tobytes(), what


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_sharp_stats_equal_restatement(ctx, oracle, case):
    r = sp.restate(oracle, case)
    d = _frames(case)
    for step in case.steps:
        st, fs = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, step)
        _same(st, fs, *r.stats(step), f"{case.tag} step {step}")
        st2, none = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, step, frames=False)
        assert none is None and st2.tobytes() == st.tobytes(), f"{case.tag} step {step}: records differ without per-frame tiles"
    # one pair the other way round: a and b change places with their sums
    if len(r.pairs):
        a, b = r.pairs[0]
        sw = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, [(b, a)] + r.pairs[1:], case.steps[0], frames=False)[0][0]
        ref = r.stats(case.steps[0])[0][0]
        assert tuple(int(v) for v in sw) == (b, a, int(ref["n"]), int(ref["e_b"]), int(ref["e_a"]), int(ref["s_b"]), int(ref["s_a"])), case.tag


@pytest.mark.parametrize("tag", ["straddle_overlap", "sharp_seventy", "sharp_steps", "m8_zero_ends"])
def test_gpu_records_on_a_second_context_and_after_gain_stats(ctx, oracle, tag):
    """the statistics share the frame table's buffer with the gain statistics: a gain call between two sharpness calls leaves no trace, nor
    does a context's history"""
    import imagemosaicing_amd as im
    from tests import gain_ref as gr
    case = TAGS[tag]
    r = sp.restate(oracle, case)
    d = _frames(case)
    step = case.steps[-1] if tag == "sharp_steps" else case.steps[0]
    first = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, step)
    gst, gcov = ctx.GainStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, 3)
    again = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, step)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    recs, cov_ref = gr.stats_ref(r.maps, r.pairs, 3)                        # and the gain statistics are still the gain statistics
    assert np.array_equal(gcov, cov_ref) and [int(s["n"]) for s in gst] == [nn for nn, _, _ in recs]
    other = im.Context(0)
    try:
        fresh = other.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, step)
    finally:
        other.close()
    assert fresh[0].tobytes() == first[0].tobytes() and fresh[1].tobytes() == first[1].tobytes()
    _same(first[0], first[1], *r.stats(step), f"{tag} step {step}")


@pytest.mark.parametrize("tag,ratio", [("sharp_steps", 0.98), ("forty", 0.9), ("sharp_seventy", 0.95), ("hidden", 0.58), ("sharp_flat", 0.58), ("m8_zero_ends", 0.99)])
def test_gpu_sharpness_dev_is_stats_then_host_solve_then_host_select(ctx, oracle, tag, ratio):
    import imagemosaicing_amd as im
    case = TAGS[tag]
    r = sp.restate(oracle, case)
    d = _frames(case)
    n = len(d[1])
    step = 1 if tag != "sharp_steps" else 3
    sharp, status, kept = ctx.SharpnessDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, blur_ratio=ratio, step=step)
    st = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], case.render.h9s, r.pairs, step, frames=False)[0]
    status2, sharp2 = im.select_sharp_frames(st, n, blur_ratio=ratio)
    assert status.tobytes() == status2.tobytes() and sharp.tobytes() == sharp2.tobytes() and sharp.tobytes() == im.solve_sharpness(st, n, blur_ratio=ratio)[0].tobytes()
    want = np.asarray(case.render.h9s, np.float32).reshape(n, 9).copy()
    want[status == 1, 8] = 0
    assert kept.dtype == np.float32 and np.array_equal(kept, want)
    # the restatement agrees wherever no decision hangs on the solve's last digits
    ref_st = r.stats(step)[0]
    rel = sr.rel_ref(sr.solve_ref(ref_st, n), ref_st, n)
    if sr.min_margin(rel, ref_st, n, ratio) > 1e-6:
        assert np.array_equal(status, sr.select_ref(rel, ref_st, n, ratio)[0]), (tag, status.tolist())
    if tag == "sharp_flat":
        assert status.tolist() == [3, 3] and (sharp == 1.0).all()


def test_gpu_strip_with_a_blurred_frame_end_to_end(ctx, oracle):
    """an 8-frame 160 x 120 strip, frame 3 blurred at sigma 2: it is flagged and dropped, nobody else is, a seamline render of the kept frames
    holds no pixel of it, and the renders of h9s_kept are the renders of the survey with that frame removed by hand"""
    imgs, h9s, pairs = sp.blur_strip(1, 2.0)
    assert len(imgs) == 8 and imgs[0].shape == (120, 160, 3)
    d = _upload(imgs)
    sharp, status, kept = ctx.SharpnessDev(d[1], d[2], d[3], d[4], h9s, pairs)
    print("sharp", sharp.tolist(), "status", status.tolist())
    assert status.tolist() == [0, 0, 0, 1, 0, 0, 0, 0], (status.tolist(), sharp.tolist())
    assert sharp[3] < 0.58 * np.delete(sharp, 3).min()
    assert kept[3, 8] == 0 and np.array_equal(np.delete(kept, 3, 0), np.delete(h9s, 3, 0)) and np.array_equal(kept[3, :8], h9s[3, :8])
    canvas, cw, ch, cws, own = ctx.MosaicSeamline(imgs, kept, want_owner=True)
    assert not (own == 4).any() and set(np.unique(own).tolist()) == {0, 1, 2, 3, 5, 6, 7, 8}          # owner holds index + 1, 0 = nobody
    before = ctx.MosaicSeamline(imgs, h9s, want_owner=True)
    assert (before[4] == 4).any() and (before[1], before[2]) == (cw, ch)
    by_hand_imgs, by_hand_h9s = [a for k, a in enumerate(imgs) if k != 3], np.delete(h9s, 3, 0)
    hand = ctx.MosaicSeamline(by_hand_imgs, by_hand_h9s, want_owner=True)
    assert (hand[1], hand[2], hand[3]) == (cw, ch, cws) and np.array_equal(hand[0], canvas)
    assert np.array_equal(hand[4] + (hand[4] >= 4), own)                    # the same owners, renumbered
    ref_kept, ref_hand = ctx.MosaicImagesRefined(imgs, kept), ctx.MosaicImagesRefined(by_hand_imgs, by_hand_h9s)
    assert ref_kept[1:] == ref_hand[1:] and np.array_equal(ref_kept[0], ref_hand[0])
    # the restatement sees the same records, so the same decision
    from tests import gain_ref as gr
    st = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], h9s, pairs, 8, frames=False)[0]
    ref = sr.stats_ref(sr.lap_maps(gr.frame_sample_maps(oracle, imgs, h9s)), pairs, 8)[0]
    assert st.tobytes() == ref.tobytes()


def test_gpu_argument_errors(ctx, oracle):
    """every refusal of the gain statistics' list, under this stage's name; the context goes on working afterwards"""
    import imagemosaicing_amd as im
    case = TAGS["hidden"]
    r = sp.restate(oracle, case)
    d = _frames(case)
    h9s = case.render.h9s

    def refused(fn, *needles):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == -1 and all(s in str(e.value) for s in needles), str(e.value)

    stats = lambda ptrs=d[1], w=d[2], h=d[3], ws=d[4], pairs=r.pairs, step=1: ctx.SharpStatsDev(ptrs, w, h, ws, h9s, pairs, step)
    refused(lambda: stats(step=0), "sharp_stats: ", "step=0 outside [1, 64]")
    refused(lambda: stats(step=65), "sharp_stats: ", "step=65 outside [1, 64]")
    refused(lambda: stats(pairs=[(0, 0)]), "sharp_stats: ", "pair 0 (0, 0)", "a == b")
    refused(lambda: stats(pairs=[(0, 3)]), "sharp_stats: ", "pair 0 (0, 3)", "outside [0, 3)")
    refused(lambda: stats(pairs=[(0, 1), (1, 0)]), "sharp_stats: ", "pair 1 (1, 0) repeats pair 0")
    refused(lambda: stats(ptrs=[d[1][0], 0, d[1][2]]), "sharp_stats: ", "frame 1 takes part but its pointer is NULL")
    refused(lambda: stats(w=[d[2][0], 1, d[2][2]]), "sharp_stats: ", "frame 1: bad geometry w=1")
    refused(lambda: stats(h=[d[3][0], d[3][1], 1]), "sharp_stats: ", "frame 2: bad geometry", "h=1")
    refused(lambda: stats(ws=[3 * d[2][0] - 1, d[4][1], d[4][2]]), "sharp_stats: ", "frame 0: bad geometry", "ws=%d" % (3 * d[2][0] - 1))
    big = 65536
    refused(lambda: ctx.SharpStatsDev([d[1][0]] * big, [d[2][0]] * big, [d[3][0]] * big, [d[4][0]] * big, np.tile(h9s[0], (big, 1)), [(0, 1)], 1), "sharp_stats: ", "n=65536 outside [1, 65535]")
    call = lambda **kw: ctx.SharpnessDev(d[1], d[2], d[3], d[4], h9s, r.pairs, **kw)
    refused(lambda: call(prior=0.0), "sharpness: ", "prior=0.0")
    refused(lambda: call(blur_ratio=1.25), "sharpness: ", "blur_ratio=1.25", "outside (0, 1]")
    refused(lambda: call(step=0), "sharpness: ", "step=0 outside [1, 64]")
    refused(lambda: ctx.SharpnessDev(d[1], d[2], d[3], d[4], h9s, [(1, 1)]), "sharp_stats: ", "a == b")
    st, fs = stats()
    _same(st, fs, *r.stats(1), "hidden after the refusals")

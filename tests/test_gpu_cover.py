"""Cover depth on the GPU: cover_depth_kernel (csrc/cover.hip) against the numpy restatement (tests/cover_ref.py) on every statistics case of
tests/cover_patterns.py at each of its steps and under each keep mask, byte for byte; the frame_cover identity against the gain statistics on
the same context, interleaved; the same bytes on a second context and after a render call; mi355_cover_select_dev against the reference's
round rule on every selection layout, and against the host loop with a callback that itself calls the kernel; the "blurred frames,
coverage-checked" recipe of INTEGRATION.md end to end; and the argument errors.  Frames are tens of pixels wide.
(tests/test_cover_patterns_ref.py checks the cases and the restatement themselves, tests/test_cover_host.py the host loop, without a GPU.)
"""
import numpy as np
import pytest

from tests import cover_patterns as cp
from tests import cover_ref as cr

pytestmark = pytest.mark.gpu

CASES = cp.stats_cases()
IDS = [c.tag for c in CASES]
TAGS = {c.tag: c for c in CASES}
SELECTS = cp.select_cases()


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


def _wh(case):
    return [s[0] for s in case.sizes], [s[1] for s in case.sizes]


def _same(fs, hist, ref_fs, ref_hist, what):
    import imagemosaicing_amd as im
    assert fs.dtype == im.COVER_FRAME_STATS and len(fs) == len(ref_fs) and hist.dtype == np.int64 and len(hist) == cr.BINS, what
    assert hist.tolist() == ref_hist.tolist(), f"{what}: hist {hist.tolist()}, expected {ref_hist.tolist()}"
    for k in range(len(fs)):
        got, want = fs["at_depth"][k].tolist(), ref_fs["at_depth"][k].tolist()
        assert got == want, f"{what}: frame {k}: at_depth {got}, expected {want}"
    assert fs.tobytes() == ref_fs.tobytes(), what


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_cover_stats_equal_restatement(ctx, oracle, case):
    r = cp.restate(oracle, case)
    w, h = _wh(case)
    for step in case.steps:
        for keep in cp.KEEPS:
            fs, hist = ctx.CoverStatsDev(w, h, case.h9s, cp.keep_mask(keep, r.n), step)
            _same(fs, hist, *r.stats(step, keep), f"{case.tag} step {step} keep {keep}")


def _upload(imgs):
    import torch
    ts = [torch.from_numpy(np.ascontiguousarray(a).reshape(a.shape[0], 3 * a.shape[1])).cuda() for a in imgs]
    torch.cuda.synchronize()
    return ts, [t.data_ptr() for t in ts], [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], [3 * a.shape[1] for a in imgs]


@pytest.mark.parametrize("tag", ["forty", "straddle_overlap", "turns", "m8_zero_ends", "rank_deficient"])
def test_gpu_every_frame_kept_gives_the_gain_stages_frame_cover(ctx, oracle, tag):
    """sum_j at_depth[k][j] == mi355_gain_stats_dev's frame_cover[k] at the same step, the two stages interleaved on one context (they share
    nothing but the context: the cover stage takes no images)"""
    case = TAGS[tag]
    r = cp.restate(oracle, case)
    d = _upload(case.render.imgs)
    for step in case.steps:
        fs, hist = ctx.CoverStatsDev(d[2], d[3], case.h9s, None, step)
        cover = ctx.GainStatsDev(d[1], d[2], d[3], d[4], case.h9s, [], step)[1]
        again = ctx.CoverStatsDev(d[2], d[3], case.h9s, None, step)
        assert np.array_equal(fs["at_depth"].sum(axis=1), cover), (tag, step, cover.tolist())
        assert again[0].tobytes() == fs.tobytes() and np.array_equal(again[1], hist)
        _same(fs, hist, *r.stats(step), f"{tag} step {step}")


@pytest.mark.parametrize("tag", ["straddle_overlap", "list257", "edge_255_256"])
def test_gpu_same_bytes_on_a_second_context_and_after_a_render(ctx, oracle, tag):
    """the stage builds its frame table in the renders' buffers: a render between two cover calls leaves no trace, nor does a context's history"""
    import imagemosaicing_amd as im
    from tests import warp_patterns as wp
    case = TAGS[tag]
    r = cp.restate(oracle, case)
    w, h = _wh(case)
    step, keep = case.steps[-1], cp.keep_mask("alternate", r.n)
    first = ctx.CoverStatsDev(w, h, case.h9s, keep, step)
    canvas = ctx.MosaicImagesRefined([wp.noise(40, 30, 1), wp.noise(40, 30, 2)], np.stack([wp.shift(0, 0), wp.shift(300.5, 7)]))
    assert canvas[1] > 256
    again = ctx.CoverStatsDev(w, h, case.h9s, keep, step)
    other = im.Context(0)
    try:
        fresh = other.CoverStatsDev(w, h, case.h9s, keep, step)
    finally:
        other.close()
    for got in (again, fresh):
        assert got[0].tobytes() == first[0].tobytes() and np.array_equal(got[1], first[1])
    _same(first[0], first[1], *r.stats(step, "alternate"), f"{tag} step {step}")


# ---- selection ------------------------------------------------------------------------------------------------------------------------------
def _select_args(case):
    return dict(order=case.order, pairs=case.pairs, keep=None if case.keep is None else np.array(case.keep, np.uint8), step=case.step, min_depth=case.min_depth,
                max_loss=case.max_loss)


@pytest.mark.parametrize("case", SELECTS, ids=[s.tag for s in SELECTS])
def test_gpu_cover_select_equals_the_reference(ctx, case):
    want = cp.reference(case)
    w, h = _wh(case)
    status, keep_out, rounds, lost = ctx.CoverSelectDev(w, h, case.h9s, **_select_args(case))
    assert status.tolist() == want.status.tolist() and keep_out.tolist() == want.keep_out.tolist(), (case.tag, status.tolist(), keep_out.tolist())
    assert (rounds, lost) == (want.rounds, want.lost), (case.tag, rounds, lost)
    # the final pass, when asked for: the statistics under keep_out; everything else unchanged
    out = ctx.CoverSelectDev(w, h, case.h9s, final=True, **_select_args(case))
    assert len(out) == 6 and out[0].tolist() == status.tolist() and out[1].tolist() == keep_out.tolist() and out[2:4] == (rounds, lost)
    covers, _, (cw, ch) = cp.geometry_of(case)
    _same(out[4], out[5], *cr.stats_ref(covers, want.keep_out, case.step, (ch, cw)), f"{case.tag} final")


@pytest.mark.parametrize("seed", [3, 17, 42, 99])
def test_gpu_cover_select_is_the_host_loop_over_the_kernel(ctx, seed):
    """mi355_cover_select_dev against mi355_cover_select with a callback that itself calls CoverStatsDev, with and without a pair list; and
    against the reference"""
    import imagemosaicing_amd as im
    for with_pairs in (False, True):
        case = cp.random_layout(seed, with_pairs)
        w, h = _wh(case)
        args = _select_args(case)
        dev = ctx.CoverSelectDev(w, h, case.h9s, **args)
        calls = []

        def stats(keep):
            calls.append(1)
            return ctx.CoverStatsDev(w, h, case.h9s, keep, case.step)[0]
        host = im.cover_select(w, h, case.h9s, stats, **args)
        assert dev[0].tolist() == host[0].tolist() and dev[1].tolist() == host[1].tolist() and dev[2:] == host[2:] and len(calls) == host[2]
        want = cp.reference(case)
        assert dev[0].tolist() == want.status.tolist() and dev[1].tolist() == want.keep_out.tolist() and dev[2:] == (want.rounds, want.lost), case.tag


# ---- the recipe of INTEGRATION.md: blurred frames, coverage-checked ----------------------------------------------------------------------------
def _count_map(ctx, w, h, h9s):
    import torch
    import imagemosaicing_amd as im
    cw, ch, cws, _ = im.mosaic_layout(w, h, h9s)
    t = torch.zeros(ch * cw, dtype=torch.int16, device="cuda")
    ctx.MosaicSeamlineDev(None, w, h, None, h9s, 0, cw, ch, cws, d_count=t.data_ptr())
    return t.cpu().numpy().view(np.uint16).reshape(ch, cw)


def _recipe(ctx, imgs, h9s, pairs):
    """SharpStatsDev -> solve_sharpness -> order = the blurred frames by ascending (rel, index) -> CoverSelectDev over the usable pairs ->
    m8 = 0 for status 1"""
    import imagemosaicing_amd as im
    d = _upload(imgs)
    n = len(imgs)
    st = ctx.SharpStatsDev(d[1], d[2], d[3], d[4], h9s, pairs, 8, frames=False)[0]
    sharp, rel = im.solve_sharpness(st, n)
    limit = np.log(im.sharp_params().blur_ratio)
    usable = [(int(s["a"]), int(s["b"])) for s in st if min(int(s["n"]), int(s["e_a"]), int(s["e_b"]), int(s["s_a"]), int(s["s_b"])) > 0]
    in_pair = {k for p in usable for k in p}
    order = sorted((k for k in range(n) if k in in_pair and rel[k] < limit), key=lambda k: (rel[k], k))
    status, keep_out, rounds, lost = ctx.CoverSelectDev(d[2], d[3], h9s, order=order, pairs=usable, step=1)
    kept = np.array(h9s, np.float32).copy()
    kept[status == im.COVER_DROPPED, 8] = 0
    before, after = _count_map(ctx, d[2], d[3], h9s), _count_map(ctx, d[2], d[3], kept)
    return order, status, lost, before, after


def test_gpu_recipe_drops_the_blurred_frame_where_the_ground_stays_covered(ctx):
    """the 8-frame strip at 60 % forward overlap with frame 3 blurred, and a ninth frame from a cross strip that lies over frame 3's ground (in
    no listed pair: it only covers).  The strip's own neighbours leave slivers of frame 3 uncovered (their rows are offset by a few pixels),
    which is why the strip alone would keep it: see the next test"""
    from tests import sharp_patterns as sp
    from tests import warp_patterns as wp
    imgs, h9s, pairs = sp.blur_strip(1, 2.0)
    imgs = imgs + [wp.noise(164, 124, 5)]
    h9s = np.concatenate([h9s, wp.shift(float(h9s[3][2]) - 2, float(h9s[3][5]) - 2)[None]])
    order, status, lost, before, after = _recipe(ctx, imgs, h9s, pairs)
    assert order == [3] and status.tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0] and lost == 0, (order, status.tolist(), lost)
    assert before.shape == after.shape and (after[before > 0] > 0).all() and (after < before).any()
    # without the ninth frame the strip's neighbours leave 34 pixels of frame 3 uncovered, and at step 1 it stays
    order, status, lost, before, after = _recipe(ctx, imgs[:8], h9s[:8], pairs)
    assert order == [3] and status.tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and np.array_equal(before, after), (order, status.tolist())


def test_gpu_recipe_keeps_the_blurred_frame_that_alone_covers_a_band(ctx):
    """the strip without frames 2 and 4: the blurred frame is still flagged, but a band of the canvas has no other cover, so it stays, and
    for coverage (status 2), although it is a cut vertex of the chain as well"""
    from tests import sharp_patterns as sp
    imgs, h9s, _ = sp.blur_strip(1, 2.0)
    left = [0, 1, 3, 5, 6, 7]
    imgs, h9s = [imgs[k] for k in left], h9s[left]
    order, status, lost, before, after = _recipe(ctx, imgs, h9s, [(k, k + 1) for k in range(5)])
    assert order[0] == 2 and status[2] == 2 and not (status == 1).any() and lost == 0, (order, status.tolist())
    assert np.array_equal(before, after)
    sole = (before == 1)
    assert sole[:, 230:300].any()                                           # the band only the blurred frame covers


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------
def test_gpu_argument_errors(ctx, oracle):
    import imagemosaicing_amd as im
    case = TAGS["hidden"]
    r = cp.restate(oracle, case)
    w, h = _wh(case)

    def refused(fn, *needles):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == -1 and all(s in str(e.value) for s in needles), str(e.value)

    refused(lambda: ctx.CoverStatsDev(w, h, case.h9s, None, 0), "cover_stats: ", "step=0 outside [1, 64]")
    refused(lambda: ctx.CoverStatsDev(w, h, case.h9s, None, 65), "cover_stats: ", "step=65 outside [1, 64]")
    refused(lambda: ctx.CoverStatsDev([w[0], 1, w[2]], h, case.h9s, None, 1), "cover_stats: ", "frame 1: bad geometry w=1")
    refused(lambda: ctx.CoverStatsDev(w, [h[0], h[1], 1], case.h9s, None, 1), "cover_stats: ", "frame 2: bad geometry", "h=1")
    big = 65536
    refused(lambda: ctx.CoverStatsDev([w[0]] * big, [h[0]] * big, np.tile(case.h9s[0], (big, 1)), None, 1), "cover_stats: ", "n=65536 outside [1, 65535]")
    sel = lambda **kw: ctx.CoverSelectDev(w, h, case.h9s, **kw)
    refused(lambda: sel(step=0), "cover_select: ", "step=0 outside [1, 64]")
    refused(lambda: sel(min_depth=0), "cover_select: ", "min_depth=0 outside [1, 8]")
    refused(lambda: sel(min_depth=9), "cover_select: ", "min_depth=9 outside [1, 8]")
    refused(lambda: sel(max_loss=-5), "cover_select: ", "max_loss=-5 < 0")
    refused(lambda: sel(order=[0, 3]), "cover_select: ", "order[1]=3 outside [0, 3)")
    refused(lambda: sel(order=[1, 1]), "cover_select: ", "order[1]=1 repeats order[0]")
    refused(lambda: sel(pairs=[(0, 0)]), "cover_select: ", "pair 0 (0, 0)", "a == b")
    refused(lambda: sel(pairs=[(0, 3)]), "cover_select: ", "pair 0 (0, 3)", "outside [0, 3)")
    refused(lambda: sel(pairs=[(0, 1), (1, 0)]), "cover_select: ", "pair 1 (1, 0) repeats pair 0")
    refused(lambda: ctx.CoverSelectDev([w[0], 1, w[2]], h, case.h9s), "cover_select: ", "frame 1: bad geometry w=1")
    fs, hist = ctx.CoverStatsDev(w, h, case.h9s, None, 1)                   # the context goes on working afterwards
    _same(fs, hist, *r.stats(1), "hidden after the refusals")

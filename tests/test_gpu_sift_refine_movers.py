"""GPU: refine_kernel's movers -- the candidates whose first Newton step does not converge -- against oracle/oracle_sift.c, bit for bit, in
top-k and keep-all, on content made of them: blobs centred half a pixel off in x, in y and in both, with widths between two DoG layers
(sift_moves_ref.half_pixel_blobs), whose candidates flip between two pixels or two layers.  The kernel drops such a candidate at the first
move that lands on a location it was fitted at before, instead of running its steps out (counter 6 of the frame counts them).

What the inputs hold is not taken on trust: the numpy restatement of the refinement (sift_moves_ref.summary, tied to the oracle in
test_sift_refine_revisit_rule.py) must find in each frame a row-only move, a layer-only move, a column move, a move of more than one
pixel and a mover that converges, and counter 6 must be the number of early exits it expects.

  128x96, 256x192   tiled route: every candidate's first step from extrema_kernel's cube, the later ones gathered
  512x384           streamed route (xstream_min_w = 256): the movers start from the cubes extrema_stream saved
  250x187           octave 1 is 125 wide: odd level widths take the loop that reads the levels sample by sample
  batch of three    binary noise in 4-pixel cells (candidates moving in every direction), zeros, the 256x192 blob frame: one launch"""
import numpy as np
import pytest

from tests import sift_moves_ref as mr
from tests import sift_patterns as sp
from tests.test_gpu_sift_edges import KEEPALL_CAP, _pmap, _same
from tests.test_gpu_sift_handoff import _context, _extract

pytestmark = pytest.mark.gpu
SHAPES = ((128, 96, False), (256, 192, False), (512, 384, True), (250, 187, False))      # width, height, streamed route
MOVES = ("row_only", "layer_only", "column", "far", "mover_converged")


@pytest.fixture(scope="module")
def frames():
    """the blob frames, what their candidates do, and the oracle's top-k and keep-all results (shared, never modified)"""
    from tests import oracle_lib
    o = oracle_lib.load_oracle()
    imgs = {(w, h): mr.half_pixel_blobs(w, h) for w, h, _ in SHAPES}
    # binary noise in cells of 4 x 4 pixels: single-pixel noise is blurred below the contrast threshold (33 candidates, no layer-only move)
    imgs["noise"] = np.ascontiguousarray(np.kron(sp.binary_noise(64, 48, 23)[:, :, 0], np.ones((4, 4), np.uint8))[:, :, None].repeat(3, 2))
    imgs["zeros"] = np.zeros((192, 256, 3), np.uint8)
    keys = list(imgs)
    vals = [imgs[k] for k in keys]
    return imgs, dict(zip(keys, _pmap(mr.summary, vals))), dict(zip(keys, _pmap(lambda i: o.sift(i), vals))), dict(zip(keys, _pmap(lambda i: o.sift(i, 0, KEEPALL_CAP), vals)))


def _has_every_move(s, tag):
    for m in MOVES:
        assert s[m] >= 1, f"{tag}: no {m} among the candidates' moves"
    assert s["early_exits"] >= 1, tag


@pytest.mark.parametrize("keepall", [False, True])
@pytest.mark.parametrize("w,h,streamed", SHAPES)
def test_blob_frames(frames, w, h, streamed, keepall):
    imgs, what, want, want_all = frames
    s = what[(w, h)]
    tag = f"blobs {w}x{h} streamed={streamed} keepall={keepall}"
    _has_every_move(s, tag)
    if (w >> 1) & 1:
        assert s["early_exits_by_octave"][1] >= 1, f"{tag}: no early exit on the odd-width octave"
    c = _context(1, keepall, streamed)
    got, cnt = _extract(c, [imgs[(w, h)]], KEEPALL_CAP if keepall else 4096)
    c.close()
    print(f"{tag}: candidates {cnt[0]} (restatement {s['candidates']}), refined {cnt[1]}, early exits {cnt[6]} (restatement {s['early_exits']}, "
          f"{s['early_exits_full']} against all four locations, {s['ran_out']} ran out), moves " + ", ".join(f"{m} {s[m]}" for m in MOVES))
    assert cnt[0] == s["candidates"], tag
    assert cnt[6] > 0 and cnt[6] == s["early_exits"], tag
    _same(got[0], (want_all if keepall else want)[(w, h)], tag)


@pytest.mark.parametrize("keepall", [False, True])
def test_batch_of_noise_zeros_and_blobs(frames, keepall):
    imgs, what, want, want_all = frames
    names = ("noise", "zeros", (256, 192))
    _has_every_move(what["noise"], "binary noise 256x192")
    assert what["zeros"]["candidates"] == 0
    by_candidates = {what[n]["candidates"]: n for n in names}
    assert len(by_candidates) == 3
    c = _context(3, keepall, streamed=False)
    got, _ = _extract(c, [imgs[n] for n in names], KEEPALL_CAP if keepall else 4096)
    seen = set()
    for k in range(3):                                                        # whichever frame's counters the context holds after a fetch: that frame's early exits
        c.GetFeatures(k, max_kp=KEEPALL_CAP if keepall else 4096)
        cnt = c.last_sift_counters()
        n = by_candidates[cnt[0]]
        assert cnt[6] == what[n]["early_exits"], f"{n} in a batch of three, keepall={keepall}"
        seen.add(n)
    c.close()
    assert any(what[n]["early_exits"] > 0 for n in seen)
    for n, g in zip(names, got):
        o = (want_all if keepall else want)[n]
        assert (len(o[0]) == 0) == (n == "zeros")
        _same(g, o, f"{n} in a batch of three, keepall={keepall}")

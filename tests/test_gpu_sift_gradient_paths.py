"""GPU: the gradient paths of orient_kernel and describe_kernel -- the branch-free det_atan2deg, the 32-bit sample offsets off a scalar
level base, and describe_kernel's queue of passing samples with one trip of loads pending -- against oracle/oracle_sift.c, bit for bit.

Every case first asserts, from the oracle's own keypoints or with numpy on the frame, that the input holds what the case is for; a case
whose input stops exercising its path fails instead of passing.

What the numpy side recomputes, and how exactly:
  * gray x 48 is the 16-bit image the pyramid starts from (BGR2GRAY in 14-bit fixed point, then x 48); its central differences are the
    unblurred counterpart of the gradients the kernels take on the Gaussian levels.  Symmetry about the main diagonal survives the blurs,
    so |dx| == |dy| on the diagonal of every level; a flat field stays flat, so dx == dy == 0 there on every level.
  * a keypoint's octave coordinates come back exactly from the record: x = ptx * 2^o, y = pty * 2^o, size = scl * 2^o * 2 (powers of
    two), octave and layer from the packed field.
  * the descriptor window test (rbin, cbin in (-1, 4), the sample at least one pixel inside the level) is evaluated in float32 in the
    kernel's order of operations.  det_sincosdeg's fmaf is formed in float64 and rounded once more (numpy has no fused multiply-add): the
    product of two float32 is exact in float64, so the result differs from fmaf only where the float64 sum lands on a float32 tie."""
import numpy as np
import pytest

from tests import sift_patterns as sp
from tests.synth_frames import terrain
from tests.test_gpu_sift_edges import KEEPALL_CAP, _pmap, _same

pytestmark = pytest.mark.gpu
F = np.float32


# ---- numpy side ---------------------------------------------------------------------------------------------------------------------
def gray48(bgr):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14) * 48


def central_differences(g):
    """(dx, dy) of the interior samples, as the kernels form them: right - left, above - below"""
    return g[1:-1, 2:] - g[1:-1, :-2], g[:-2, 1:-1] - g[2:, 1:-1]


def octave_coords(kp):
    """(o, layer, ptx, pty, scl) per keypoint, exact (see the module docstring)"""
    o = (kp["octave"] & 255).astype(np.int64)
    layer = ((kp["octave"] >> 8) & 255).astype(np.int64)
    s2 = np.exp2(o).astype(F)
    return o, layer, kp["x"] / s2, kp["y"] / s2, kp["size"] / (s2 * F(2.0))


def descriptor_radius(scl):
    hw = F(3.0) * scl.astype(F)
    return np.rint(hw * F(1.4142135623730951) * F(5.0) * F(0.5)).astype(np.int64)


def _fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def sincosdeg(deg):
    """det_sincosdeg (csrc/detmath.h) on a float32 array"""
    deg = deg.astype(F)
    q = np.rint(deg * F(1.0 / 90.0))
    r = _fmaf(np.full_like(deg, -90.0), q, deg)
    t = r * F(0.017453292519943295)
    t2 = t * t
    s = _fmaf(t2, np.full_like(t, 2.7557319e-6), np.full_like(t, -1.9841270e-4))
    s = _fmaf(s, t2, np.full_like(t, 8.3333333e-3))
    s = _fmaf(s, t2, np.full_like(t, -1.6666667e-1))
    s = _fmaf(s * t2, t, t)
    c = _fmaf(t2, np.full_like(t, 2.4801587e-5), np.full_like(t, -1.3888889e-3))
    c = _fmaf(c, t2, np.full_like(t, 4.1666667e-2))
    c = _fmaf(c, t2, np.full_like(t, -0.5))
    c = _fmaf(c, t2, np.full_like(t, 1.0))
    k = q.astype(np.int64) & 3
    sn = np.select([k == 0, k == 1, k == 2], [s, c, -s], -c)
    cs = np.select([k == 0, k == 1, k == 2], [c, -s, -c], s)
    return sn.astype(F), cs.astype(F)


def queued_samples(kp, w, h):
    """per keypoint: the number of samples of its descriptor window that pass describe_kernel's test, i.e. that it queues, and the number
    of the kernel's rounds that start with a trip pending and complete no trip of their own.  A round is the kernel's: lane l tests the
    samples [l * per, (l + 1) * per) of the window in scan order, per = ceil(S / 64), four per round, and after a round every full 64 of
    the queue make a trip."""
    o, _, ptx, pty, scl = octave_coords(kp)
    sn, cs = sincosdeg(kp["angle"])
    rad = descriptor_radius(scl)
    out, idle = np.zeros(len(kp), np.int64), np.zeros(len(kp), np.int64)
    for q in range(len(kp)):
        rows, cols = h >> o[q], w >> o[q]
        hw = F(3.0) * scl[q]
        cos_t, sin_t = cs[q] / hw, sn[q] / hw
        px, py = int(np.rint(ptx[q])), int(np.rint(pty[q]))
        ii, jj = np.mgrid[-rad[q]:rad[q] + 1, -rad[q]:rad[q] + 1]
        fi, fj = ii.astype(F), jj.astype(F)
        c_rot = fj * cos_t - fi * sin_t
        r_rot = fj * sin_t + fi * cos_t
        rbin = r_rot + F(2.0) - F(0.5)
        cbin = c_rot + F(2.0) - F(0.5)
        r, c = py + ii, px + jj
        ok = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)
        out[q] = int(ok.sum())
        S = ok.size
        per = (S + 63) // 64
        rnd = (np.arange(S) % per) // 4
        qn, trips = 0, 0
        for passed in np.bincount(rnd[ok.ravel()], minlength=(per + 3) // 4):
            qn += int(passed)
            if trips and qn < 64:
                idle[q] += 1
            trips += qn // 64
            qn %= 64
    return out, idle


def window_mask(kp, w, h):
    """octave-0 pixels inside some keypoint's descriptor window (the window of an octave-o keypoint, scaled back by 2^o)"""
    o, _, ptx, pty, scl = octave_coords(kp)
    rad = descriptor_radius(scl)
    m = np.zeros((h, w), bool)
    for q in range(len(kp)):
        s = 1 << int(o[q])
        x, y, r = int(np.rint(ptx[q])) * s, int(np.rint(pty[q])) * s, int(rad[q]) * s
        m[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return m


# ---- GPU side -----------------------------------------------------------------------------------------------------------------------
def _context(batch, keepall):
    import imagemosaicing_amd as im
    p = im.default_params()
    if keepall:
        p.nfeatures = 0
    c = im.Context(0, p)
    c.set_option("sift_batch", batch)
    return c


def _extract(c, imgs, keepall):
    """the frames as ONE batch (the context's sift_batch is len(imgs)): (keypoints, u8 descriptors) per frame"""
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs]
    torch.cuda.synchronize()
    for k, (d, i) in enumerate(zip(dev, imgs)):
        c.SiftExtractDev(k, d.data_ptr(), i.shape[1], i.shape[0], 3 * i.shape[1])
    out = []
    for k in range(len(imgs)):
        kp, desc = c.GetFeatures(k, max_kp=KEEPALL_CAP if keepall else 4096)
        d8 = desc.astype(np.uint8)
        assert np.array_equal(desc, d8.astype(np.float32)), "descriptors are not integer valued"
        out.append((kp, d8))
    return out


def _oracle_both(imgs):
    """per frame: (top-k result, keep-all result) of the oracle"""
    from tests import oracle_lib
    o = oracle_lib.load_oracle()
    return list(zip(_pmap(lambda i: o.sift(i), imgs), _pmap(lambda i: o.sift(i, 0, KEEPALL_CAP), imgs)))


def _run_single(frames, want, tag):
    """every frame alone, top-k and keep-all, against the oracle"""
    for keepall in (False, True):
        c = _context(1, keepall)
        for name, img in frames.items():
            got = _extract(c, [img], keepall)[0]
            _same(got, want[name][int(keepall)], f"{tag} {name} keepall={keepall}")
        c.close()


# ---- inputs (built once per module, never modified) ----------------------------------------------------------------------------------
SYM = 192


def symmetric_terrain():
    g = terrain(SYM, SYM, seed=23).astype(np.int32)
    return np.ascontiguousarray(((g + g.transpose(1, 0, 2)) // 2).astype(np.uint8))


@pytest.fixture(scope="module")
def square_frames():
    """192 x 192: the frames of the atan2 case and two more contents for the batch of four, with the oracle's results"""
    m = {"symmetric": symmetric_terrain(), "impulses": sp.impulses(SYM, SYM, 0, 255), "terrain": terrain(SYM, SYM, seed=sp.shape_seed(SYM, SYM)),
         "binary_noise": sp.binary_noise(SYM, SYM, 17)}
    return m, dict(zip(m, _oracle_both(list(m.values()))))


def test_tie_and_zero_arms_of_atan2(square_frames):
    """det_atan2deg selects numerator and denominator by ax >= ay.  `symmetric` is symmetric about its main diagonal, where every sample has
    |dx| == |dy| (the tie, which must take the first form); `impulses` is single pixels and 3 x 3 squares on a flat field: dx == dy == 0
    (0 / eps) over most of every window and one of the two zero next to an impulse.  Between them the oracle's orientations cover all four
    quadrants, i.e. both sign folds."""
    m, want = square_frames
    for name, what in (("symmetric", "ties"), ("impulses", "zeros")):
        img, kp = m[name], want[name][1][0]
        assert len(want[name][0][0]) >= 50 and len(kp) >= 50, name
        dx, dy = central_differences(gray48(img))
        inside = window_mask(kp, SYM, SYM)[1:-1, 1:-1]
        ties = int(((np.abs(dx) == np.abs(dy)) & (dx != 0) & inside).sum())
        zeros = int(((dx == 0) & (dy == 0) & inside).sum())
        one_zero = int((((dx == 0) != (dy == 0)) & inside).sum())
        quadrants = np.bincount((kp["angle"] // 90).astype(np.int64) % 4, minlength=4)
        print(f"{name}: {len(kp)} keypoints, ties {ties}, zeros {zeros}, one component zero {one_zero}, angles per quadrant {quadrants}")
        if what == "ties":
            assert np.array_equal(img, img.transpose(1, 0, 2))
            assert ties >= 150          # the diagonal alone has 190 interior samples
        else:
            assert zeros >= 10000 and one_zero >= 1000
        assert (quadrants > 0).all(), name
    _run_single({n: m[n] for n in ("symmetric", "impulses")}, want, "atan2 arms")


EDGE_W, EDGE_H, EDGE_D = 200, 136, 5          # d = 4 puts every extremum at the edge inside IMG_BORDER, where it is dropped (sp.edge_dots)


def test_windows_cut_by_all_four_borders():
    """Gaussian dots 5 px from every edge of a 200 x 136 frame: descriptor and orientation windows that reach past row 0, column 0, the last
    row and the last column.  The samples that remain start at row 1 / column 1, where the 32-bit offset of the sample above / to the left
    is smallest (row 0, column 0: offset 0 must not wrap)."""
    img = sp.edge_dots(EDGE_W, EDGE_H, EDGE_D)
    want = {"edge_dots": _oracle_both([img])[0]}
    for kp, _ in want["edge_dots"]:
        o, _, ptx, pty, scl = octave_coords(kp)
        rad = descriptor_radius(scl)
        px, py = np.rint(ptx).astype(np.int64), np.rint(pty).astype(np.int64)
        cols, rows = EDGE_W >> o, EDGE_H >> o
        cut = {"left": rad > px, "top": rad > py, "right": rad > cols - 1 - px, "bottom": rad > rows - 1 - py}
        print(f"edge_dots{EDGE_D} {EDGE_W}x{EDGE_H}: {len(kp)} keypoints, cut by " + ", ".join(f"{k} {int(v.sum())}" for k, v in cut.items()))
        for k, v in cut.items():
            assert v.any(), f"no keypoint whose window is cut by the {k} edge"
    _run_single({"edge_dots": img}, want, f"{EDGE_W}x{EDGE_H}")


QUEUE_SHAPES = [(48, 48), (100, 300), (300, 100), (111, 111)]


def test_short_and_exact_queues():
    """describe_kernel queues the samples that pass the window test and consumes them 64 at a time, one trip pending; what is left goes to
    the tail.  Asserted with the kernel's own test in numpy: at least one keypoint queues an exact multiple of 64 samples (full trips and an
    empty tail), and some keypoints have a short queue -- a round that starts with a trip pending, queues fewer than 64 samples and
    completes no trip, so the pending trip's loads stay outstanding across a whole round of the cheap test.

    A keypoint that queues fewer than 64 samples IN ALL (the tail alone, nothing ever pending) does not exist: the smallest level is 12
    samples a side, its 10 x 10 interior lies within 10 samples of any keypoint in it and the 4 x 4 grid reaches 2.5 x 3 x scl >= 12
    samples in every direction, so no keypoint queues fewer than 100; over all of sp.SMALL_OCTAVE with terrain, impulses and binary noise
    the smallest count the oracle's keypoints give is 244.  The smallest count of these frames is printed and must stay below 512, i.e.
    keypoints with few trips are present."""
    assert all(s in sp.SMALL_OCTAVE for s in QUEUE_SHAPES)
    frames = {f"{w}x{h}": terrain(w, h, seed=sp.shape_seed(w, h)) for (w, h) in QUEUE_SHAPES}
    want = dict(zip(frames, _oracle_both(list(frames.values()))))
    short = exact = total = 0
    least = 1 << 30
    for (w, h), name in zip(QUEUE_SHAPES, frames):
        kp = want[name][1][0]                    # keep-all: every keypoint of the frame, the top-k set among them
        n, idle = queued_samples(kp, w, h)
        short += int((idle > 0).sum()); exact += int((n % 64 == 0).sum()); total += len(n); least = min(least, int(n.min()))
        print(f"{name}: {len(n)} keypoints, queued samples min {n.min()} max {n.max()}, with a short round: {int((idle > 0).sum())}, multiples of 64: {int((n % 64 == 0).sum())}")
    assert total >= 100 and short >= 1 and exact >= 1 and 100 <= least < 512, (total, short, exact, least)
    _run_single(frames, want, "queues")


def test_batch_of_four_equals_single_frames(square_frames):
    """four different contents in one launch: every frame equals its single-frame result, the oracle's (a wave's pending trip or its
    scalar level base must not reach the next keypoint or frame)"""
    m, want = square_frames
    for keepall in (False, True):
        c = _context(4, keepall)
        got = _extract(c, list(m.values()), keepall)
        for n, g in zip(m, got):
            assert len(want[n][int(keepall)][0]) >= 20, n
            _same(g, want[n][int(keepall)], f"{n} {SYM}x{SYM} in a batch of four, keepall={keepall}")
        c.close()

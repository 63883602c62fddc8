"""Inputs of the tie-refinement tests (tests/test_tie_refine_ref.py on the CPU, tests/test_gpu_tie_refine.py on the GPU): the quality scene
with its ground truth, small frames, and pair records built from point lists.  Nothing here is cached on disk; the quality case is built
once per process."""
import functools

import numpy as np

from tests import tie_refine_ref as tr

f32 = np.float32


def blur(img, sigma):
    r = int(4 * sigma + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        pad = [(r, r) if a == axis else (0, 0) for a in (0, 1)]
        p = np.pad(img, pad, mode="reflect")
        n = img.shape[axis]
        img = sum(k[t] * np.take(p, np.arange(t, t + n), axis=axis) for t in range(2 * r + 1))
    return img


def scene(seed, size=520):
    """the sum of two Gaussian-blurred white-noise fields (sigma 1.5 px weight 1, sigma 4 px weight 0.7), scaled to 0..255; float64"""
    rng = np.random.default_rng(seed)
    a, b = blur(rng.standard_normal((size, size)), 1.5), blur(rng.standard_normal((size, size)), 4.0)
    s = a / a.std() + 0.7 * b / b.std()
    return (s - s.min()) * (255.0 / (s.max() - s.min()))


def project(G, x, y):
    """double: (x, y) through the 3 x 3 map G"""
    d = G[2, 0] * x + G[2, 1] * y + G[2, 2]
    return (G[0, 0] * x + G[0, 1] * y + G[0, 2]) / d, (G[1, 0] * x + G[1, 1] * y + G[1, 2]) / d


def render(sc, G, w, h, rng, sigma):
    """a w x h BGR frame: pixel p shows the scene at G(p), bilinear in double, plus N(0, sigma^2) levels, rounded"""
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X, Y = project(G, xs, ys)
    xi, yi = np.floor(X).astype(int), np.floor(Y).astype(int)
    assert xi.min() >= 0 and yi.min() >= 0 and xi.max() < sc.shape[1] - 1 and yi.max() < sc.shape[0] - 1
    q, p = X - xi, Y - yi
    v = sc[yi, xi] * (1 - p) * (1 - q) + sc[yi, xi + 1] * (1 - p) * q + sc[yi + 1, xi] * p * (1 - q) + sc[yi + 1, xi + 1] * p * q
    v = np.clip(np.rint(v + rng.normal(0.0, sigma, v.shape)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[..., None], 3, axis=2))


def similarity(deg, s, tx, ty, px=0.0, py=0.0):
    c, n = s * np.cos(np.radians(deg)), s * np.sin(np.radians(deg))
    return np.array([[c, -n, tx], [n, c, ty], [px, py, 1.0]])


def record(i, j, a_xy, b_xy, H, accepted=1, ids=None):
    """one PAIR_RESULT: inliers a_xy in image i, b_xy in image j (float arrays [n, 2]), H float[9]"""
    r = np.zeros(1, tr.PAIR_RESULT)[0]
    n = len(a_xy)
    r["i"], r["j"], r["n_in"], r["n_selected"], r["ok"], r["accepted"], r["_pad"] = i, j, n, min(n + 3, 396), 1, accepted, 7
    r["H"] = np.asarray(H, f32).reshape(9)
    m = min(n, 400)
    r["a"]["x"][:m], r["a"]["y"][:m] = np.asarray(a_xy, f32)[:m, 0], np.asarray(a_xy, f32)[:m, 1]
    r["b"]["x"][:m], r["b"]["y"][:m] = np.asarray(b_xy, f32)[:m, 0], np.asarray(b_xy, f32)[:m, 1]
    idv = np.arange(m, dtype=np.int32) * 3 + 11 if ids is None else np.asarray(ids, np.int32)
    r["a"]["id"][:m], r["b"]["id"][:m] = idv, idv + 1000
    return r


def records(*recs):
    out = np.zeros(len(recs), tr.PAIR_RESULT)
    for k, r in enumerate(recs):
        out[k] = r
    return out


@functools.lru_cache(maxsize=None)
def quality(tie_sigma=0.5, img_sigma=2.0):
    """The quality case of the issue: two 240 x 240 frames of one 520 x 520 scene, frame j (image 1) the scene shifted by (130, 140), frame i
    (image 0) a rotation of 12 degrees with scale 1.06, shift (150, 90) and perspective terms 4e-5, -3e-5; H the exact j -> i map in float32;
    400 points b uniform in [40, 200)^2 kept where H(b) lies in [30, 210)^2; a = H(b) + N(0, tie_sigma^2).  Returns a dict with the frames
    (also an unrelated frame i for the false pair), H, truth (H(b), double) and the one record."""
    sc = scene(1)
    rng = np.random.default_rng(2)
    Gj = similarity(0.0, 1.0, 130.0, 140.0)
    Gi = similarity(12.0, 1.06, 150.0, 90.0, 4e-5, -3e-5)
    fj = render(sc, Gj, 240, 240, rng, img_sigma)
    fi = render(sc, Gi, 240, 240, rng, img_sigma)
    other = render(scene(3), Gi, 240, 240, rng, img_sigma)
    Hd = np.linalg.inv(Gi) @ Gj
    Hd = Hd / Hd[2, 2]
    H = Hd.astype(f32).reshape(9)
    b = rng.uniform(40.0, 200.0, (400, 2)).astype(f32)
    tx, ty = project(H.astype(np.float64).reshape(3, 3), b[:, 0].astype(np.float64), b[:, 1].astype(np.float64))
    ok = (tx >= 30) & (tx < 210) & (ty >= 30) & (ty < 210)
    b, truth = b[ok], np.stack([tx[ok], ty[ok]], 1)
    a = (truth + rng.normal(0.0, tie_sigma, truth.shape)).astype(f32) if tie_sigma > 0 else truth.astype(f32)
    Hres = H.copy()
    Hres[8] = f32(1.7)                                     # Ransac2D's residual sits in H[8]; the refinement must read it as 1
    return dict(imgs=[fi, fj], other=other, H=H, truth=truth, rec=records(record(0, 1, a, b, Hres)))


def rms(rec, truth):
    n = len(truth)
    d = np.stack([rec["a"]["x"][:n], rec["a"]["y"][:n]], 1).astype(np.float64) - truth
    return float(np.sqrt((d ** 2).sum(1).mean()))


def random_frame(w, h, seed, smooth=1.2):
    """a textured BGR frame with three different channels (the gray weights matter)"""
    rng = np.random.default_rng(seed)
    chans = []
    for _ in range(3):
        v = blur(rng.standard_normal((h + 8, w + 8)), smooth)[4:-4, 4:-4]
        chans.append((v - v.min()) * (255.0 / (v.max() - v.min())))
    return np.ascontiguousarray(np.rint(np.stack(chans, 2)).astype(np.uint8))


def warp_frame(src, H, w, h):
    """frame i such that src (frame j) maps into it by H (j -> i): nearest-in-double bilinear resampling, for tests that only need a
    plausible partner frame, not ground truth"""
    Hi = np.linalg.inv(np.asarray(H, np.float64).reshape(3, 3))
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X, Y = project(Hi, xs, ys)
    X, Y = np.clip(X, 0, src.shape[1] - 1.001), np.clip(Y, 0, src.shape[0] - 1.001)
    xi, yi = np.floor(X).astype(int), np.floor(Y).astype(int)
    q, p = (X - xi)[..., None], (Y - yi)[..., None]
    s = src.astype(np.float64)
    v = s[yi, xi] * (1 - p) * (1 - q) + s[yi, xi + 1] * (1 - p) * q + s[yi + 1, xi] * p * (1 - q) + s[yi + 1, xi + 1] * p * q
    return np.ascontiguousarray(np.rint(v).astype(np.uint8))


def checker(w, h, period):
    """0 / 255 checker of the given period, all channels alike"""
    y, x = np.mgrid[0:h, 0:w]
    assert period in (2, 3)
    v = ((x + y) & 1) * 255 if period == 2 else ((x % 3 == 0) ^ (y % 3 == 0)) * 255
    return np.ascontiguousarray(np.repeat(v.astype(np.uint8)[..., None], 3, axis=2))


@functools.lru_cache(maxsize=None)
def status_case():
    """Two 96 x 80 frames, frame i (image 0) = frame j (image 1) moved by (+2, +1) whole pixels, so a true tie correlates to exactly 1; a
    block of frame j is flat (FLAT templates) and another block of frame i alone is flat (windows without variance: LOW with peak 0).  One
    record whose ties meet every status at radius 7, search 3.  Returns (imgs, records, expected statuses)."""
    fj = random_frame(96, 80, 5)
    fj[50:75, 5:30] = 77
    fi = np.roll(fj, (1, 2), axis=(0, 1))
    fi[5:40, 55:95] = 200
    H = [1, 0, 2, 0, 1, 1, 0, 0, 1]
    b = np.array([[40.25, 30.5], [33.0, 44.0], [40.0, 52.0], [6.5, 30.0], [7.5, 30.0], [17.0, 62.0], [73.0, 21.0], [45.5, 60.25]], np.float64)
    err = np.array([[0.3, -0.4], [1.0, -2.0], [3.0, 0.0], [0, 0], [0, 0], [0, 0], [0, 0], [-0.45, 0.2]])
    a = b + [2, 1] + err
    want = [tr.REFINED, tr.REFINED, tr.BORDER, tr.EDGE, tr.EDGE, tr.FLAT, tr.LOW, tr.REFINED]
    return [fi, fj], records(record(0, 1, a, b, H)), np.array(want, np.uint8)

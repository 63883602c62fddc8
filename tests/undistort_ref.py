"""numpy restatement of the lens undistortion (include/mi355_mosaic.h, "lens undistortion"; csrc/undistort.hip, csrc/lens.h), written from
the contract: every operation of the map is a separate float32 operation in the header's order, the sample is the renders' pixel expression.

    cam    : dict with fx, fy, cx, cy, k1, k2, p1, p2, k3 (Python floats = the C doubles)
    out    : None (the camera's own intrinsics) or (out_fx, out_fy, out_cx, out_cy)
"""
import numpy as np

F = np.float32
NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")


def camera(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    return dict(zip(NAMES, (float(fx), float(fy), float(cx), float(cy), float(k1), float(k2), float(p1), float(p2), float(k3))))


def consts(cam, out=None):
    """the constants formed once on the host: the camera and the output principal point cast to float, the reciprocal focal lengths from
    quotients taken in double"""
    ofx, ofy, ocx, ocy = (cam["fx"], cam["fy"], cam["cx"], cam["cy"]) if out is None or all(v == 0 for v in out) else out
    with np.errstate(over="ignore"):
        c = {k: F(cam[k]) for k in NAMES}
    c["ocx"], c["ocy"] = F(ocx), F(ocy)
    c["ifx"], c["ify"] = F(1.0 / float(ofx)), F(1.0 / float(ofy))
    return c


def distort(c, x, y):
    """(xs, ys) of normalised output coordinates x, y (float32 arrays of one shape)"""
    with np.errstate(over="ignore", invalid="ignore"):
        xx = x * x; yy = y * y; xy = x * y; r2 = xx + yy; a1 = xy + xy
        t = r2 * c["k3"]; t = c["k2"] + t; t = r2 * t; t = c["k1"] + t; t = r2 * t; rad = F(1.0) + t
        tx = (c["p1"] * a1) + (c["p2"] * (r2 + (xx + xx)))
        ty = (c["p1"] * (r2 + (yy + yy))) + (c["p2"] * a1)
        xd = (x * rad) + tx; yd = (y * rad) + ty
        xs = (c["fx"] * xd) + c["cx"]; ys = (c["fy"] * yd) + c["cy"]
    assert xs.dtype == F and ys.dtype == F
    return xs, ys


def source_map_at(c, u, v):
    """(xs, ys) of the output pixels (u, v): integer arrays of one shape"""
    x = (u.astype(F) - c["ocx"]) * c["ifx"]
    y = (v.astype(F) - c["ocy"]) * c["ify"]
    return distort(c, x, y)


def source_map(cam, w, h, out=None):
    """the two source-coordinate planes, float32 [h, w]"""
    v, u = np.mgrid[0:h, 0:w]
    return source_map_at(consts(cam, out), u, v)


def inside(xs, ys, w, h):
    with np.errstate(invalid="ignore"):
        return (xs >= F(0)) & (xs <= F(w - 1)) & (ys >= F(0)) & (ys <= F(h - 1))


def bilin(s00, s01, s10, s11, p, q):
    """hm::bilin: (uchar)(int)(((s00 (1-p)) (1-q) + (s01 (1-p)) q) + (s10 p) (1-q)) + (s11 p) q), float32 throughout"""
    omp, omq = F(1.0) - p, F(1.0) - q
    v = (((s00 * omp) * omq + (s01 * omp) * q) + (s10 * p) * omq) + (s11 * p) * q
    assert v.dtype == F
    return v.astype(np.int32).astype(np.uint8)


def undistort(img, cam, out=None, fill=0):
    """(the undistorted [h, w, 3] uint8 image, n_outside)"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    xs, ys = source_map(cam, w, h, out)
    has = inside(xs, ys, w, h)
    res = np.full((h, w, 3), fill, np.uint8)
    xv, yv = xs[has], ys[has]
    xi = np.minimum(xv.astype(np.int32), w - 2)
    yi = np.minimum(yv.astype(np.int32), h - 2)
    q = xv - xi.astype(F)
    p = yv - yi.astype(F)
    f = img.astype(F)
    vals = np.stack([bilin(f[yi, xi, c], f[yi, xi + 1, c], f[yi + 1, xi, c], f[yi + 1, xi + 1, c], p, q) for c in range(3)], -1)
    res[has] = vals
    return res, int((~has).sum())


def border(w, h):
    """(u, v) of the 2 (w + h) - 4 border pixels"""
    u = np.concatenate([np.arange(w), np.arange(w), np.zeros(h - 2, np.int64), np.full(h - 2, w - 1)])
    v = np.concatenate([np.zeros(w, np.int64), np.full(w, h - 1), np.arange(1, h - 1), np.arange(1, h - 1)])
    return u, v


def fit(cam, w, h):
    """(j, (out_fx, out_fy, out_cx, out_cy)) of mi355_undistort_fit; j = None where no scale fits"""
    u, v = border(w, h)
    for j in range(128, 1025):
        s = j / 256.0
        out = (s * float(F(cam["fx"])), s * float(F(cam["fy"])), cam["cx"], cam["cy"])
        xs, ys = source_map_at(consts(cam, out), u, v)
        if inside(xs, ys, w, h).all():
            return j, out
    return None, None


# ---- the test cameras and the direction check's scene ----------------------------------------------------------------------------------
def cameras_for(w, h):
    """barrel, pincushion, tangential: f = 0.8 w, c = ((w-1)/2, (h-1)/2)"""
    f, cx, cy = 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0
    return {"barrel": camera(f, f, cx, cy, -0.25, 0.07),
            "pincushion": camera(f, f, cx, cy, 0.2, 0.05),
            "tangential": camera(f, 1.01 * f, cx + 1.3, cy - 0.7, -0.2, 0.05, 1e-3, -2e-3, 0.01)}


def scene(X, Y):
    return 127.5 + 127.5 * np.sin(40.0 * X) * np.sin(40.0 * Y + 1.0)


def to_bgr(a):
    g = np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)
    return np.repeat(g[..., None], 3, -1)


def render_pinhole(w, h, fx, fy, cx, cy):
    """the scene seen by an ideal pinhole camera (double)"""
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    return to_bgr(scene((u - cx) / fx, (v - cy) / fy))


def render_distorted(w, h, cam, iters=50):
    """the scene seen by the distorted camera: pixel (u, v) sees the normalised point whose distorted image it is; the model is inverted by
    `iters` fixed-point iterations in double"""
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    xd, yd = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
    x, y = xd.copy(), yd.copy()
    k1, k2, p1, p2, k3 = (cam[k] for k in ("k1", "k2", "p1", "p2", "k3"))
    for _ in range(iters):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        tx = p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
        ty = p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
        x, y = (xd - tx) / rad, (yd - ty) / rad
    return to_bgr(scene(x, y))

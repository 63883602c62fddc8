"""CPU: the lens undistortion's restatement (tests/undistort_ref.py) and the host-only calls of the built library.

  * identity: a camera without distortion, power-of-two focal lengths and an integer centre gives back its frame, last row and column included;
  * the three test cameras (barrel, pincushion, tangential): the pixels outside with the camera's own intrinsics, the scale mi355_undistort_fit
    finds, nothing outside after the fit -- the figures come from an independent prototype of the restatement: a transcription that gives
    others is wrong;
  * the direction of the model, which no byte comparison can see: a scene rendered through each distorted camera and then undistorted is the
    scene seen by the fitted pinhole camera (mean absolute difference below a quarter of what not undistorting leaves);
  * mi355_undistort_map and mi355_undistort_fit of the built library equal the restatement bit for bit; every refusal of both;
  * NaN and infinite coordinates count as outside;
  * the new symbols are exported and declared, the structs have their sizes in C, the adaptor's UndistortImage compiles, and the binding
    fails loudly without a context.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import undistort_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 48), (37, 29), (200, 150)]
NAMES = ["barrel", "pincushion", "tangential"]
OUTSIDE_OWN = {"barrel": [0, 0, 0], "pincushion": [508, 202, 4340], "tangential": [0, 0, 0]}
FIT_J = {"barrel": [242, 241, 242], "pincushion": [284, 284, 285], "tangential": [246, 246, 246]}
NEW = ["mi355_default_undistort_params", "mi355_undistort_fit", "mi355_undistort_map", "mi355_undistort_frames_dev", "mi355_undistort_image"]


def frame(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def identity_camera(w, h):
    return ur.camera(64.0, 64.0, w // 2, h // 2)


@pytest.fixture(scope="module")
def im():
    from imagemosaicing_amd import build
    build.build()
    import imagemosaicing_amd
    return imagemosaicing_amd


def c_camera(im, cam):
    return im.Camera(**cam)


def j_of(params, cam):
    """the j of a fitted parameter set: out_fx = (j / 256) * (double)(float)fx is exact in double"""
    j = params.out_fx * 256.0 / float(np.float32(cam["fx"]))
    assert j == int(j)
    return int(j)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_identity_gives_back_the_frame(w, h):
    img = frame(w, h, 1)
    cam = identity_camera(w, h)
    out, n_out = ur.undistort(img, cam)
    assert np.array_equal(out, img) and n_out == 0
    xs, ys = ur.source_map(cam, w, h)
    v, u = np.mgrid[0:h, 0:w]
    assert np.array_equal(xs, u.astype(np.float32)) and np.array_equal(ys, v.astype(np.float32))
    assert ur.fit(cam, w, h)[0] == 256


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("i", range(3))
def test_counts_and_fit_of_the_test_cameras(name, i):
    w, h = SIZES[i]
    cam = ur.cameras_for(w, h)[name]
    img = frame(w, h, 2 + i)
    _, n_own = ur.undistort(img, cam)
    assert n_own == OUTSIDE_OWN[name][i]
    j, out = ur.fit(cam, w, h)
    assert j == FIT_J[name][i]
    res, n_fit = ur.undistort(img, cam, out)
    assert n_fit == 0
    # fill is what a pixel without a sample gets, and nothing else changes with it
    a, na = ur.undistort(img, cam, None, fill=0)
    b, nb = ur.undistort(img, cam, None, fill=255)
    has = ur.inside(*ur.source_map(cam, w, h), w, h)
    assert na == nb == int((~has).sum()) and np.array_equal(a[has], b[has]) and (a[~has] == 0).all() and (b[~has] == 255).all()


@pytest.mark.parametrize("name", NAMES)
def test_direction_of_the_model(name):
    w, h = 96, 72
    cam = ur.cameras_for(w, h)[name]
    seen = ur.render_distorted(w, h, cam)
    j, out = ur.fit(cam, w, h)
    und, n_out = ur.undistort(seen, cam, out)
    assert n_out == 0
    fitted = ur.render_pinhole(w, h, *out)
    own = ur.render_pinhole(w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    err = np.abs(und.astype(np.float64) - fitted).mean()
    base = np.abs(seen.astype(np.float64) - own).mean()
    print(name, "undistorted vs fitted pinhole %.3f, distorted vs own pinhole %.3f" % (err, base))
    assert err < base / 4.0, (err, base)


def test_nan_and_infinite_coordinates_are_outside():
    w, h = 64, 48
    cam = ur.camera(8.0, 8.0, 32, 24, k1=3e38)
    c = ur.consts(cam)
    v, u = np.mgrid[0:h, 0:w]
    x = (u.astype(np.float32) - c["ocx"]) * c["ifx"]
    y = (v.astype(np.float32) - c["ocy"]) * c["ify"]
    r2 = x * x + y * y
    xs, ys = ur.source_map(cam, w, h)
    assert np.isnan(xs).any() and np.isinf(xs).any()
    has = ur.inside(xs, ys, w, h)
    assert np.array_equal(has, r2 == 0) and has.sum() == 1
    img = frame(w, h, 9)
    out, n_out = ur.undistort(img, cam, fill=7)
    assert n_out == w * h - 1 and np.array_equal(out[24, 32], img[24, 32]) and (out[~has] == 7).all()


# ---- the library's host-only calls ------------------------------------------------------------------------------------------------------
def all_cases():
    for w, h in SIZES:
        yield "identity", w, h, identity_camera(w, h)
        for name in NAMES:
            yield name, w, h, ur.cameras_for(w, h)[name]
    yield "k1=3e38", 64, 48, ur.camera(8.0, 8.0, 32, 24, k1=3e38)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_library_map_and_fit_equal_the_restatement(im):
    for name, w, h, cam in all_cases():
        cc = c_camera(im, cam)
        xs, ys = im.undistort_map(cc, w, h)
        rx, ry = ur.source_map(cam, w, h)
        assert same_bits(xs, rx) and same_bits(ys, ry), (name, w, h)
        j, out = ur.fit(cam, w, h)
        if j is None:
            with pytest.raises(im.Mi355Error) as e:
                im.undistort_fit(cc, w, h)
            assert e.value.code == -2 and "128..1024" in str(e.value)
            continue
        p = im.undistort_fit(cc, w, h)
        assert j_of(p, cam) == j and (p.out_fx, p.out_fy, p.out_cx, p.out_cy) == out and p.fill == 0 and list(p.reserved) == [0, 0, 0], (name, w, h)
        xs, ys = im.undistort_map(cc, w, h, p)
        rx, ry = ur.source_map(cam, w, h, out)
        assert same_bits(xs, rx) and same_bits(ys, ry), (name, w, h)
        # explicit output intrinsics equal to the camera's are the defaults
        xs, ys = im.undistort_map(cc, w, h, out_fx=cam["fx"], out_fy=cam["fy"], out_cx=cam["cx"], out_cy=cam["cy"])
        rx, ry = ur.source_map(cam, w, h)
        assert same_bits(xs, rx) and same_bits(ys, ry), (name, w, h)


def test_fit_finds_no_scale_for_an_extreme_lens(im):
    """so much pincushion that even the longest focal length of the scan (j = 1024) leaves border pixels outside: no j, in the restatement and
    in the library"""
    w, h = 64, 48
    cam = ur.camera(20.0, 20.0, 31.5, 23.5, k1=50.0)
    assert ur.fit(cam, w, h)[0] is None
    with pytest.raises(im.Mi355Error) as e:
        im.undistort_fit(c_camera(im, cam), w, h)
    assert e.value.code == -2


def test_refusals_of_fit_and_map(im):
    L = im.load_library()
    good = ur.cameras_for(64, 48)["barrel"]
    out = im.UndistortParams()
    xs = np.zeros((48, 64), np.float32)
    ys = np.zeros((48, 64), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, word):
        msg = (L.mi355_last_error(None) or b"").decode()
        assert rc == -1 and word in msg, (rc, word, msg)

    cases = [(dict(fx=float("nan")), "camera.fx"), (dict(fy=float("inf")), "camera.fy"), (dict(cx=float("nan")), "camera.cx"),
             (dict(cy=float("-inf")), "camera.cy"), (dict(k1=float("nan")), "camera.k1"), (dict(k2=float("inf")), "camera.k2"),
             (dict(p1=float("nan")), "camera.p1"), (dict(p2=float("nan")), "camera.p2"), (dict(k3=float("inf")), "camera.k3"),
             (dict(fx=0.0), "camera.fx"), (dict(fy=-3.0), "camera.fy")]
    for change, word in cases:
        cc = c_camera(im, dict(good, **change))
        refused(L.mi355_undistort_fit(C.byref(cc), 64, 48, C.byref(out)), word)
        refused(L.mi355_undistort_map(C.byref(cc), None, 64, 48, ptr(xs), ptr(ys)), word)
    cc = c_camera(im, good)
    for w, h, word in [(1, 48, "w="), (64, 1, "h="), ((1 << 20) + 1, 48, "w="), (64, (1 << 20) + 1, "h="), (0, 0, "w="), (-5, 48, "w=")]:
        refused(L.mi355_undistort_fit(C.byref(cc), w, h, C.byref(out)), word)
        refused(L.mi355_undistort_map(C.byref(cc), None, w, h, ptr(xs), ptr(ys)), word)
    refused(L.mi355_undistort_fit(None, 64, 48, C.byref(out)), "camera")
    refused(L.mi355_undistort_fit(C.byref(cc), 64, 48, None), "out")
    refused(L.mi355_undistort_map(None, None, 64, 48, ptr(xs), ptr(ys)), "camera")
    refused(L.mi355_undistort_map(C.byref(cc), None, 64, 48, None, ptr(ys)), "xs")
    refused(L.mi355_undistort_map(C.byref(cc), None, 64, 48, ptr(xs), None), "ys")
    for change, word in [(dict(out_fx=float("nan")), "out_fx"), (dict(out_fy=float("inf")), "out_fy"), (dict(out_cx=float("nan")), "out_cx"),
                         (dict(out_cy=float("inf")), "out_cy"), (dict(out_fx=-1.0, out_fy=50.0), "out_fx"), (dict(out_fx=50.0), "out_fy"),
                         (dict(fill=256), "fill"), (dict(fill=-1), "fill")]:
        p = im.undistort_params(**change)
        refused(L.mi355_undistort_map(C.byref(cc), C.byref(p), 64, 48, ptr(xs), ptr(ys)), word)
    # and a good call after them
    assert L.mi355_undistort_fit(C.byref(cc), 64, 48, C.byref(out)) == 0 and j_of(out, good) == 242
    assert L.mi355_undistort_map(C.byref(cc), C.byref(out), 64, 48, ptr(xs), ptr(ys)) == 0


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared(im):
    L = im.load_library()
    hdr = open(os.path.join(ROOT, "include", "mi355_mosaic.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    assert "mi355_camera" in hdr and "mi355_undistort_params" in hdr
    for name in ("Camera", "UndistortParams", "undistort_params", "undistort_fit", "undistort_map"):
        assert hasattr(im, name), name
    for name in ("UndistortFramesDev", "UndistortImage"):
        assert hasattr(im.Context, name), name
    p = im.undistort_params()
    assert C.sizeof(p) == 48 and (p.out_fx, p.out_fy, p.out_cx, p.out_cy, p.fill) == (0.0, 0.0, 0.0, 0.0, 0) and list(p.reserved) == [0, 0, 0]
    p = im.undistort_params(out_fx=3.0, out_fy=4.0, out_cx=5.0, out_cy=6.0, fill=9)
    assert (p.out_fx, p.out_fy, p.out_cx, p.out_cy, p.fill) == (3.0, 4.0, 5.0, 6.0, 9)
    assert C.sizeof(im.Camera) == 72


def test_structs_have_their_sizes_in_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mi355_mosaic.h"\n'
                   'typedef char camera_is_72[sizeof(mi355_camera) == 72 ? 1 : -1];\n'
                   'typedef char params_are_48[sizeof(mi355_undistort_params) == 48 ? 1 : -1];\n'
                   'int main(void) { mi355_undistort_params p; mi355_camera c; c.k3 = 0; p.fill = 0; p.reserved[2] = 0; p.out_cy = c.k3; return p.fill; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_adaptor_undistort_compiles_as_cxx(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "mi355_adaptor.h"\nusing namespace mi355ref;\n'
                   'int f(const IplImage* a, IplImage* b, const mi355_camera& c, const mi355_undistort_params* p) {\n'
                   '  return mi355::UndistortImage(a, b, c) + mi355::UndistortImage(a, b, c, p); }\n'
                   'int main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    syms = subprocess.run(["nm", "-C", str(tmp_path / "t.o")], capture_output=True, text=True).stdout
    assert "mi355_undistort_image" in syms


def test_binding_raises_without_a_context(im):
    """a context that does not exist: both new methods reach the C ABI and fail there, loudly (no CPU path answers instead)"""
    ctx = im.Context.__new__(im.Context)
    ctx.L, ctx._h, ctx.device = im.load_library(), C.c_void_p(), 0
    cam = c_camera(im, ur.cameras_for(32, 32)["barrel"])
    img = np.zeros((32, 32, 3), np.uint8)
    for call in (lambda: ctx.UndistortFramesDev([4096], [8192], [32], [32], [96], [96], cam),
                 lambda: ctx.UndistortImage(img, cam),
                 lambda: ctx.UndistortImage(img, cam, out=img, fill=3)):
        with pytest.raises(im.Mi355Error) as e:
            call()
        assert e.value.code == -1

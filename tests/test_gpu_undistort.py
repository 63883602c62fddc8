"""GPU: lens undistortion (mi355_undistort_frames_dev / mi355_undistort_image, csrc/undistort.hip), byte for byte against the numpy
restatement of tests/undistort_ref.py.

  * widths on both sides of a lane's 4 pixels and a workgroup's 1024 columns, heights of 2, 3 and 9 rows, a 16 x 4000 frame;
  * content on the truncating cast's boundary (0 / 255 checkers, all-255 frames), random frames;
  * pitches and base alignments of source and destination (tests/pitched.py), every byte that is not a pixel untouched;
  * 70 frames of mixed sizes in one call against 70 calls, n = 1 and n = 0;
  * in place equals out of place, mixed calls, and an in-place group larger than one scratch fill;
  * samples at exactly w - 1 / h - 1, half-pixel shifts, NaN / infinite coordinates, fill;
  * the host form, every refusal (the ctx stays usable), and the output as ordinary frames of the gain stage and a render.
"""
import ctypes as C

import numpy as np
import pytest

from tests import undistort_ref as ur

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import imagemosaicing_amd as im
    ctx = im.Context(0)
    yield torch, im, ctx
    ctx.close()


def rand_frame(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def up(torch, img, pad=0, fill=0):
    """a device copy [h, 3w + pad] of a host image"""
    h, w = img.shape[:2]
    a = np.full((h, 3 * w + pad), fill, np.uint8)
    a[:, :3 * w] = img.reshape(h, 3 * w)
    return torch.from_numpy(a).cuda()


def down(t, w):
    a = t.cpu().numpy()
    return a[:, :3 * w].reshape(a.shape[0], w, 3)


def c_cam(im, cam):
    return im.Camera(**cam)


def params_of(im, out=None, fill=0):
    return im.undistort_params(fill=fill) if out is None else im.undistort_params(out_fx=out[0], out_fy=out[1], out_cx=out[2], out_cy=out[3], fill=fill)


def run_dev(env, imgs, cam, out=None, fill=0, in_place=False):
    """the frames through one mi355_undistort_frames_dev call on tight pitches: ([h, w, 3] outputs, n_outside)"""
    torch, im, ctx = env
    src = [up(torch, i) for i in imgs]
    dst = src if in_place else [torch.full_like(s, 99) for s in src]
    torch.cuda.synchronize()
    w = [i.shape[1] for i in imgs]; h = [i.shape[0] for i in imgs]; ws = [3 * x for x in w]
    cnt = ctx.UndistortFramesDev([s.data_ptr() for s in src], [d.data_ptr() for d in dst], w, h, ws, ws, c_cam(im, cam), params_of(im, out, fill))
    if not in_place:
        for s, i in zip(src, imgs):
            assert np.array_equal(down(s, i.shape[1]), i)                     # sources unchanged
    return [down(d, x) for d, x in zip(dst, w)], cnt


def check(env, imgs, cam, out=None, fill=0, in_place=False):
    got, cnt = run_dev(env, imgs, cam, out, fill, in_place)
    for k, i in enumerate(imgs):
        want, n_out = ur.undistort(i, cam, out, fill)
        assert np.array_equal(got[k], want), (k, i.shape, int((got[k] != want).sum()))
        assert cnt[k] == n_out, (k, i.shape, cnt[k], n_out)
    return got, cnt


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4100])
def test_widths_around_the_lane_and_the_workgroup_row(env, w):
    for h in (2, 3, 9):
        check(env, [rand_frame(w, h, 10 * w + h)], ur.cameras_for(w, h)["pincushion"])


def test_a_narrow_tall_frame(env):
    w, h = 16, 4000
    _, cnt = check(env, [rand_frame(w, h, 5)], ur.cameras_for(w, h)["pincushion"])
    assert cnt[0] > 0


# ---- content ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["barrel", "pincushion", "tangential"])
def test_content_on_the_truncating_casts_boundary(env, name):
    w, h = 67, 45
    v, u = np.mgrid[0:h, 0:w]
    checker = np.repeat((((u + v) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    checker[..., 1] = 255 - checker[..., 1]
    imgs = [checker, 255 - checker, np.full((h, w, 3), 255, np.uint8), rand_frame(w, h, 3)]
    cam = ur.cameras_for(w, h)[name]
    check(env, imgs, cam)
    j, out = ur.fit(cam, w, h)
    _, cnt = check(env, imgs, cam, out)
    assert not cnt.any()


# ---- pitches and alignment --------------------------------------------------------------------------------------------------------------
def test_pitches_and_alignment(env):
    torch, im, ctx = env
    from tests import pitched as pf
    sizes = [(37, 29), (64, 48), (5, 7), (130, 9)]
    n = 16
    shapes = [sizes[k % 4] for k in range(n)]
    imgs = [rand_frame(w, h, 40 + k) for k, (w, h) in enumerate(shapes)]
    src_pitch = [[3 * w, pf.ipl_pitch(w), pf.pitch_256(w)][k % 3] for k, (w, h) in enumerate(shapes)]
    dst_pitch = [[3 * w + 1, 3 * w + 2, pf.ipl_pitch(w), pf.pitch_256(w)][(k + k // 4) % 4] for k, (w, h) in enumerate(shapes)]
    fs = pf.PitchedFrames(imgs, src_pitch, offsets=[(k + 2) % 4 for k in range(n)], seed=11)
    fd = pf.PitchedFrames([np.zeros_like(i) for i in imgs], dst_pitch, offsets=[k // 4 for k in range(n)], seed=12)
    # every base offset meets every destination pitch kind
    assert len({(k // 4, (k + k // 4) % 4) for k in range(n)}) == 16
    ts, sp = fs.to_device(torch)
    td, dp = fd.to_device(torch)
    w, h, _ = fs.geom()
    cam = ur.camera(40.0, 41.0, 30.2, 20.7, 0.2, 0.05, 1e-3, -2e-3, 0.01)
    cnt = ctx.UndistortFramesDev(sp, dp, w, h, fs.ws, fd.ws, c_cam(im, cam), fill=200)
    got_s, got_d = fs.device_bytes(ts), fd.device_bytes(td)
    pix = np.zeros(fd.nbytes, bool)
    for k in range(n):
        want, n_out = ur.undistort(imgs[k], cam, None, 200)
        assert np.array_equal(fd.pixels(k, got_d), want), (k, shapes[k], src_pitch[k], dst_pitch[k])
        assert cnt[k] == n_out
        fd.view(k, pix)[:, :fd.row_bytes(k)] = True
    assert np.array_equal(got_d[~pix], fd.buf[~pix])                          # row padding and the gaps between frames
    assert np.array_equal(got_s, fs.buf)
    # the same frames in place on the source's pitches
    cnt2 = ctx.UndistortFramesDev(sp, sp, w, h, fs.ws, fs.ws, c_cam(im, cam), fill=200)
    got_s = fs.device_bytes(ts)
    pix = np.zeros(fs.nbytes, bool)
    for k in range(n):
        assert np.array_equal(fs.pixels(k, got_s), fd.pixels(k, got_d)), k
        fs.view(k, pix)[:, :fs.row_bytes(k)] = True
    assert np.array_equal(cnt2, cnt) and np.array_equal(got_s[~pix], fs.buf[~pix])


# ---- many frames ------------------------------------------------------------------------------------------------------------------------
def test_mixed_sizes_in_one_call_equal_single_calls(env):
    torch, im, ctx = env
    rng = np.random.default_rng(8)
    sizes = [(2, 2), (300, 200), (2, 200), (300, 2), (3, 3), (5, 4)] + [(int(rng.integers(2, 301)), int(rng.integers(2, 201))) for _ in range(64)]
    assert len(sizes) == 70
    imgs = [rand_frame(w, h, 100 + k) for k, (w, h) in enumerate(sizes)]
    cam = ur.camera(150.0, 148.0, 20.5, 14.0, 0.2, 0.05, 1e-3, -2e-3, 0.01)    # one camera for all sizes
    got, cnt = check(env, imgs, cam, fill=33)
    assert cnt.any() and (cnt < np.array([w * h for w, h in sizes])).all()          # pixels without a sample, and samples in every frame
    for k, i in enumerate(imgs):
        one, c1 = run_dev(env, [i], cam, fill=33)                              # n = 1
        assert np.array_equal(one[0], got[k]) and c1[0] == cnt[k], k
    # n = 0: success, nothing done -- also with no arrays at all
    assert len(ctx.UndistortFramesDev([], [], [], [], [], [], c_cam(im, cam))) == 0
    assert ctx.L.mi355_undistort_frames_dev(ctx._h, None, None, None, None, None, None, 0, C.byref(c_cam(im, cam)), None, None) == 0


# ---- in place ---------------------------------------------------------------------------------------------------------------------------
def test_in_place_equals_out_of_place_and_mixes_with_it(env):
    torch, im, ctx = env
    sizes = [(200, 150), (37, 29), (64, 48), (1025, 9), (5, 300)]
    imgs = [rand_frame(w, h, 60 + k) for k, (w, h) in enumerate(sizes)]
    cam = ur.cameras_for(200, 150)["tangential"]
    a, ca = check(env, imgs, cam)
    b, cb = check(env, imgs, cam, in_place=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ca, cb)
    # frames 0, 2, 4 in place (with a pitch of their own), 1 and 3 out of place
    src = [up(torch, i, pad=5, fill=77) for i in imgs]
    dst = [s if k % 2 == 0 else torch.full((s.shape[0], s.shape[1] + 3), 88, dtype=torch.uint8, device="cuda") for k, s in enumerate(src)]
    torch.cuda.synchronize()
    w = [x for x, _ in sizes]; h = [y for _, y in sizes]
    cc = ctx.UndistortFramesDev([s.data_ptr() for s in src], [d.data_ptr() for d in dst], w, h, [s.shape[1] for s in src], [d.shape[1] for d in dst], c_cam(im, cam))
    assert np.array_equal(cc, ca)
    for k in range(len(imgs)):
        assert np.array_equal(down(dst[k], w[k]), a[k]), k
        full = dst[k].cpu().numpy()
        assert (full[:, 3 * w[k]:] == (77 if k % 2 == 0 else 88)).all(), k       # the copy back writes 3w bytes per row
        if k % 2:
            assert np.array_equal(down(src[k], w[k]), imgs[k])


def test_an_in_place_group_larger_than_one_scratch_fill(env):
    """3 frames of 8000 x 7500 are 180 MB each: the 512 MB scratch holds two, so the call runs two groups (two launches; the profile hook
    counts them) -- the real sizes, not a stand-in: the frames are made and compared on the device, which keeps the test within a second."""
    torch, im, ctx = env
    w, h, n = 8000, 7500, 3
    g = torch.Generator(device="cuda").manual_seed(4)
    src = [torch.randint(0, 256, (h, 3 * w), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    dst = [torch.empty_like(s) for s in src]
    cam = c_cam(im, ur.cameras_for(w, h)["pincushion"])
    geom = ([w] * n, [h] * n, [3 * w] * n, [3 * w] * n)
    band0 = h // 2 - 40
    band = src[n - 1][band0:band0 + 80].cpu().numpy().reshape(80, w, 3)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        c_out = ctx.UndistortFramesDev([s.data_ptr() for s in src], [d.data_ptr() for d in dst], *geom, cam)
        assert ctx.profile_get("undistort")[1] == 1
        ctx.profile_reset()
        c_in = ctx.UndistortFramesDev([s.data_ptr() for s in src], [s.data_ptr() for s in src], *geom, cam)
        assert ctx.profile_get("undistort")[1] == 2
    finally:
        ctx.profile_enable(False)
    assert np.array_equal(c_in, c_out) and (c_out > 0).all()
    for s, d in zip(src, dst):
        assert torch.equal(s, d)
    # a band of rows round the centre of the last frame against the restatement (byte offsets near 90 MB)
    v0, v1 = h // 2 - 4, h // 2 + 4
    want = band_ref(band, band0, ur.cameras_for(w, h)["pincushion"], w, h, v0, v1)
    assert np.array_equal(dst[n - 1][v0:v1].cpu().numpy().reshape(v1 - v0, w, 3), want)
    del src, dst
    torch.cuda.empty_cache()


def band_ref(band, band0, cam, w, h, v0, v1):
    """output rows [v0, v1) of a w x h frame of which the source rows from band0 on are at hand in `band` (the samples must lie in them)"""
    v, u = np.mgrid[v0:v1, 0:w]
    xs, ys = ur.source_map_at(ur.consts(cam), u, v)
    has = ur.inside(xs, ys, w, h)
    res = np.zeros((v1 - v0, w, 3), np.uint8)
    xv, yv = xs[has], ys[has]
    xi = np.minimum(xv.astype(np.int32), w - 2); yi = np.minimum(yv.astype(np.int32), h - 2) - band0
    assert yi.min() >= 0 and yi.max() + 1 < band.shape[0]
    q = xv - xi.astype(np.float32); p = yv - (yi + band0).astype(np.float32)
    f = band.astype(np.float32)
    res[has] = np.stack([ur.bilin(f[yi, xi, c], f[yi, xi + 1, c], f[yi + 1, xi, c], f[yi + 1, xi + 1, c], p, q) for c in range(3)], -1)
    return res


# ---- the closed interval, degenerate arithmetic -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 48), (37, 29), (1025, 3)])
def test_identity_and_half_pixel_shifts(env, w, h):
    img = rand_frame(w, h, 21)
    cam = ur.camera(64.0, 64.0, w // 2, h // 2)
    got, cnt = check(env, [img], cam)
    assert np.array_equal(got[0], img) and cnt[0] == 0                         # samples at exactly w - 1 and h - 1: q = 1, p = 1
    for dx, dy in [(-0.5, 0.0), (0.0, -0.5), (-0.5, -0.5), (0.5, 0.5)]:
        out = (64.0, 64.0, w // 2 - dx, h // 2 - dy)                           # xs = u + dx, ys = v + dy
        xs, ys = ur.source_map(cam, w, h, out)
        assert xs[0, w - 1] == np.float32(w - 1 + dx) and ys[h - 1, 0] == np.float32(h - 1 + dy)
        got, cnt = check(env, [img], cam, out, fill=9)
        assert cnt[0] == h * (dx != 0) + w * (dy != 0) - (dx != 0 and dy != 0)  # a column and / or a row fall outside


def test_nan_and_infinite_coordinates_get_fill(env):
    w, h = 64, 48
    img = rand_frame(w, h, 22)
    cam = ur.camera(8.0, 8.0, 32, 24, k1=3e38)
    xs, ys = ur.source_map(cam, w, h)
    assert np.isnan(xs).any() and np.isinf(xs).any()
    got, cnt = check(env, [img], cam, fill=255)
    assert cnt[0] == w * h - 1 and np.array_equal(got[0][24, 32], img[24, 32])
    assert (np.delete(got[0].reshape(-1, 3), 24 * w + 32, 0) == 255).all()
    check(env, [img, rand_frame(300, 7, 23)], cam, fill=0)


# ---- the host form ------------------------------------------------------------------------------------------------------------------------
def test_host_form_equals_the_device_form(env):
    torch, im, ctx = env
    for k, (w, h) in enumerate([(200, 150), (37, 29), (2, 2), (1025, 5)]):
        img = rand_frame(w, h, 30 + k)
        cam = ur.cameras_for(w, h)["tangential" if k % 2 else "pincushion"]
        dev, cnt = run_dev(env, [img], cam, fill=17)
        out, n_out = ctx.UndistortImage(img, c_cam(im, cam), fill=17)
        assert np.array_equal(out, dev[0]) and n_out == cnt[0]
        want, n_ref = ur.undistort(img, cam, None, 17)
        assert np.array_equal(out, want) and n_out == n_ref
        # a padded destination keeps its padding; dst == src
        wide = np.full((h, 3 * w + 7), 55, np.uint8)
        view = wide[:, :3 * w].reshape(h, w, 3)
        ctx.UndistortImage(img, c_cam(im, cam), out=view, fill=17)
        assert np.array_equal(view, want) and (wide[:, 3 * w:] == 55).all()
        same = img.copy()
        res, n_same = ctx.UndistortImage(same, c_cam(im, cam), out=same, fill=17)
        assert res is same and np.array_equal(same, want) and n_same == n_ref


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable(env):
    torch, im, ctx = env
    w, h = 40, 30
    img = rand_frame(w, h, 50)
    cam = ur.cameras_for(w, h)["barrel"]
    buf = torch.zeros(8 * 4096, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    ws = 3 * w
    fb = ws * (h - 1) + 3 * w                                                  # the bytes of a frame's range

    def refused(word, d_src, d_dst, ww, hh, ws_s, ws_d, camera=cam, **kw):
        with pytest.raises(im.Mi355Error) as e:
            ctx.UndistortFramesDev(d_src, d_dst, ww, hh, ws_s, ws_d, c_cam(im, camera), **kw)
        assert e.value.code == -1 and word in str(e.value), (word, str(e.value))

    A, B, Cc = base, base + 4096, base + 8192
    refused("d_src", [0], [B], [w], [h], [ws], [ws])
    refused("d_dst", [A], [0], [w], [h], [ws], [ws])
    refused("ws_src", [A], [B], [w], [h], [ws - 1], [ws])
    refused("ws_dst", [A], [B], [w], [h], [ws], [ws - 1])
    for bad in (1, 0, -4, (1 << 20) + 1):
        refused("w=", [A], [B], [bad], [h], [4 << 20], [4 << 20])
        refused("h=", [A], [B], [w], [bad], [ws], [ws])
    for name in ur.NAMES:
        refused("camera." + name, [A], [B], [w], [h], [ws], [ws], camera=dict(cam, **{name: float("nan")}))
        refused("camera." + name, [A], [B], [w], [h], [ws], [ws], camera=dict(cam, **{name: float("inf")}))
    refused("camera.fx", [A], [B], [w], [h], [ws], [ws], camera=dict(cam, fx=0.0))
    refused("camera.fy", [A], [B], [w], [h], [ws], [ws], camera=dict(cam, fy=-1.0))
    for name in ("out_fx", "out_fy", "out_cx", "out_cy"):
        good = dict(out_fx=30.0, out_fy=30.0, out_cx=20.0, out_cy=15.0)
        refused(name, [A], [B], [w], [h], [ws], [ws], **dict(good, **{name: float("nan")}))
    refused("out_fx", [A], [B], [w], [h], [ws], [ws], out_fx=-2.0, out_fy=30.0)
    refused("out_fy", [A], [B], [w], [h], [ws], [ws], out_fx=30.0, out_fy=0.0, out_cx=1.0)
    refused("fill", [A], [B], [w], [h], [ws], [ws], fill=256)
    refused("fill", [A], [B], [w], [h], [ws], [ws], fill=-1)
    # overlaps: dst into the next frame's src, dst into another dst, dst shifted against its own src, in place with another pitch, one source
    # behind another frame's in-place range
    refused("overlaps", [A, B], [Cc, A + fb - 1], [w] * 2, [h] * 2, [ws] * 2, [ws] * 2)
    refused("overlaps", [A, B], [Cc, Cc + fb - 1], [w] * 2, [h] * 2, [ws] * 2, [ws] * 2)
    refused("overlaps", [A], [A + 3], [w], [h], [ws], [ws])
    refused("overlaps", [A], [A], [w], [h], [ws], [ws + 4])
    refused("overlaps", [A, A + 1], [A, B], [w] * 2, [h] * 2, [ws] * 2, [ws] * 2)
    refused("n=", [A] * 65536, [B] * 65536, [w] * 65536, [h] * 65536, [ws] * 65536, [ws] * 65536)
    L = ctx.L
    cc = c_cam(im, cam)
    assert L.mi355_undistort_frames_dev(ctx._h, None, None, None, None, None, None, -1, C.byref(cc), None, None) == -1
    assert "n=" in (L.mi355_last_error(ctx._h) or b"").decode()
    assert L.mi355_undistort_frames_dev(ctx._h, None, None, None, None, None, None, 1, C.byref(cc), None, None) == -1
    assert "d_src" in (L.mi355_last_error(ctx._h) or b"").decode()
    assert L.mi355_undistort_frames_dev(ctx._h, None, None, None, None, None, None, 0, None, None, None) == -1
    assert "camera" in (L.mi355_last_error(ctx._h) or b"").decode()
    # two sources may share bytes, and ranges may touch
    ctx.UndistortFramesDev([A, A], [B, Cc], [w] * 2, [h] * 2, [ws] * 2, [ws] * 2, c_cam(im, cam))
    ctx.UndistortFramesDev([A, A + fb], [base + 16384, base + 16384 + fb], [w] * 2, [h] * 2, [ws] * 2, [ws] * 2, c_cam(im, cam))
    # the host form's own arguments
    for call, word in [(lambda: L.mi355_undistort_image(ctx._h, None, w, h, ws, C.c_void_p(img.ctypes.data), ws, C.byref(cc), None, None), "src"),
                       (lambda: L.mi355_undistort_image(ctx._h, C.c_void_p(img.ctypes.data), w, h, ws, None, ws, C.byref(cc), None, None), "dst"),
                       (lambda: L.mi355_undistort_image(ctx._h, C.c_void_p(img.ctypes.data), w, h, ws - 1, C.c_void_p(img.ctypes.data), ws, C.byref(cc), None, None), "ws="),
                       (lambda: L.mi355_undistort_image(ctx._h, C.c_void_p(img.ctypes.data), w, h, ws, C.c_void_p(img.ctypes.data), ws - 1, C.byref(cc), None, None), "dst_ws="),
                       (lambda: L.mi355_undistort_image(ctx._h, C.c_void_p(img.ctypes.data), 1, h, ws, C.c_void_p(img.ctypes.data), ws, C.byref(cc), None, None), "w="),
                       (lambda: L.mi355_undistort_image(ctx._h, C.c_void_p(img.ctypes.data), w, h, ws, C.c_void_p(img.ctypes.data), ws, None, None, None), "camera")]:
        assert call() == -1
        assert word in (L.mi355_last_error(ctx._h) or b"").decode(), word
    # and the same ctx runs a good call
    check(env, [img], cam)


# ---- downstream ---------------------------------------------------------------------------------------------------------------------------
def test_undistorted_frames_are_ordinary_frames(env):
    torch, im, ctx = env
    from tests.synth import texture
    w, h, n = 160, 120, 3
    imgs = [texture(w, h, 70 + k) for k in range(n)]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))
    for k, (dx, dy) in enumerate([(0, 0), (70, 5), (30, 60)]):
        h9s[k, 2], h9s[k, 5] = dx, dy
    pairs = [(0, 1), (0, 2), (1, 2)]
    cam = ur.cameras_for(w, h)["barrel"]
    j, out = ur.fit(cam, w, h)
    ws = 3 * w + 4
    dev = [up(torch, i, pad=4) for i in imgs]
    host = [up(torch, ur.undistort(i, cam, out)[0], pad=4) for i in imgs]
    torch.cuda.synchronize()
    geom = ([w] * n, [h] * n, [ws] * n)
    cnt = ctx.UndistortFramesDev([t.data_ptr() for t in dev], [t.data_ptr() for t in dev], *geom, [ws] * n, c_cam(im, cam), params_of(im, out))
    assert not cnt.any()
    g_dev = ctx.GainCompensateDev([t.data_ptr() for t in dev], *geom, h9s, pairs)
    g_host = ctx.GainCompensateDev([t.data_ptr() for t in host], *geom, h9s, pairs)
    assert np.array_equal(g_dev, g_host)
    cw, ch, cws, _ = im.mosaic_layout([w] * n, [h] * n, h9s)
    canvases = []
    for frames in (dev, host):
        canvas = torch.zeros((ch, cws), dtype=torch.uint8, device="cuda")
        ctx.MosaicMedianDev([t.data_ptr() for t in frames], *geom, h9s, canvas.data_ptr(), cw, ch, cws)
        ctx.synchronize()
        canvases.append(canvas.cpu().numpy())
    assert np.array_equal(canvases[0], canvases[1]) and canvases[0].any()
    for a, b in zip(dev, host):
        assert torch.equal(a, b)

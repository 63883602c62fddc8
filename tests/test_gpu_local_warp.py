"""GPU: the local registration (csrc/local_warp.hip) against the numpy restatement of tests/local_warp_ref.py.

  * local_warp_kernel (mi355_apply_local_warps_dev) byte for byte: the smallest frames, widths on both sides of a lane's FP_PX = 4 pixels and a
    workgroup's FP_BW = 1024 columns by FP_ROWS + 1 = 9 rows, grids from 1 x 1 to 16 x 16 and one with a node per column, displacements that
    are zero, clamp at all four borders, half and quarter pixels, random; every pitch kind at every base offset with every byte that is not
    a pixel untouched; out of place and in place; mixed sizes in one call, each frame the same alone and among others;
  * tie_residual_kernel (mi355_tie_residual_stats_dev) every sum bit for bit on records built for every branch (tests/local_warp_cases.py:
    edge_case), on a survey at four grids, with no records, and against the host twin;
  * mi355_local_register_dev end to end, and every refusal with the ctx usable afterwards.
"""
import numpy as np
import pytest

from tests import local_warp_cases as lc
from tests import local_warp_ref as lr
from tests import pitched as pf

pytestmark = pytest.mark.gpu

BW, PX, ROWS = 1024, 4, 8          # frame_pass.h: FP_BW, FP_PX, FP_ROWS


@pytest.fixture(scope="module")
def env():
    import torch
    import imagemosaicing_amd as im
    ctx = im.Context(0)
    yield torch, im, ctx
    ctx.close()


def rand_frame(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def rand_grid(gx, gy, amp, seed):
    return np.random.default_rng(seed).uniform(-amp, amp, (gy + 1, gx + 1, 2)).astype(np.float32)


def const_grid(gx, gy, dx, dy):
    g = np.zeros((gy + 1, gx + 1, 2), np.float32)
    g[..., 0], g[..., 1] = dx, dy
    return g


def run_apply(env, imgs, grids, in_place=False):
    """the frames through one mi355_apply_local_warps_dev call on tight pitches, a guard row behind every buffer: ([h, w, 3] outputs,
    n_clamped)"""
    torch, im, ctx = env
    src = [torch.from_numpy(np.concatenate([i.reshape(i.shape[0], -1), np.full((1, 3 * i.shape[1]), 171, np.uint8)])).cuda() for i in imgs]
    dst = src if in_place else [torch.full_like(s, 99) for s in src]
    torch.cuda.synchronize()
    w = [i.shape[1] for i in imgs]; h = [i.shape[0] for i in imgs]; ws = [3 * x for x in w]
    cnt = ctx.ApplyLocalWarpsDev([s.data_ptr() for s in src], [d.data_ptr() for d in dst], w, h, ws, ws, np.stack(grids))
    out = []
    for k, i in enumerate(imgs):
        d, s = dst[k].cpu().numpy(), src[k].cpu().numpy()
        assert (d[-1] == (171 if in_place else 99)).all() and (s[-1] == 171).all(), k      # the guard rows
        if not in_place:
            assert np.array_equal(s[:-1].reshape(i.shape), i), k                           # sources unchanged
        out.append(d[:-1].reshape(i.shape))
    return out, cnt


def check_apply(env, imgs, grids, in_place=False):
    got, cnt = run_apply(env, imgs, grids, in_place)
    for k, (i, g) in enumerate(zip(imgs, grids)):
        want, n = lr.apply(i, g)
        assert np.array_equal(got[k], want), (k, i.shape, g.shape, int((got[k] != want).sum()))
        assert cnt[k] == n, (k, i.shape, cnt[k], n)
    return got, cnt


def groups(env, imgs, grids):
    """frames of one grid shape per call (a call has one grid), out of place and in place"""
    a, ca = check_apply(env, imgs, grids)
    b, cb = check_apply(env, imgs, grids, in_place=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ca, cb)
    return a, ca


# ---- local_warp_kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(2, 2), (3, 2), (33, 29), (96, 80), (BW - 1, ROWS + 1), (BW, ROWS + 1), (BW + 1, ROWS + 1), (BW + PX, ROWS + 1)])
def test_sizes_around_the_lane_the_workgroup_and_the_row_step(env, w, h):
    img = rand_frame(w, h, 7 * w + h)
    for gx, gy in ((1, 1), (3, 2), (8, 6), (16, 16), (w - 1, 1)):
        gx, gy = min(gx, w - 1, 16), min(gy, h - 1, 16)
        imgs = [img, rand_frame(w, h, 1), img, img, img]
        grids = [rand_grid(gx, gy, 3.0, gx + 31 * gy), const_grid(gx, gy, 0, 0), const_grid(gx, gy, 0.5, -0.5), const_grid(gx, gy, -0.25, 0.25),
                 rand_grid(gx, gy, 0.01, 5)]
        got, cnt = groups(env, imgs, grids)
        assert np.array_equal(got[1], imgs[1]) and cnt[1] == 0                 # the zero grid: the source, last row and column included


def test_a_node_per_column(env):
    w, h = 17, 13
    img = rand_frame(w, h, 3)
    groups(env, [img, img], [rand_grid(w - 1, h - 1, 2.0, 1), const_grid(w - 1, h - 1, 0, 0)])


@pytest.mark.parametrize("shift", [8.0, 64.0])
def test_clamping_at_all_four_borders(env, shift):
    w, h = 150, 130
    img = rand_frame(w, h, 9)
    grids = [const_grid(8, 6, sx * shift, sy * shift) for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1))]
    _, cnt = groups(env, [img] * 6, grids)
    s = int(shift)
    assert cnt.tolist() == [s * h, s * h, s * w, s * w, s * h + s * w - s * s, s * h + s * w - s * s]
    # a grid that pushes outwards at every border node only
    g = np.zeros((7, 9, 2), np.float32)
    g[:, 0, 0], g[:, -1, 0], g[0, :, 1], g[-1, :, 1] = -shift, shift, -shift, shift
    _, cnt = groups(env, [img], [g])
    assert cnt[0] > 0


def test_pitches_and_alignment(env):
    torch, im, ctx = env
    sizes = [(37, 29), (64, 48), (5, 7), (130, 9), (33, 29)]
    n = 20
    shapes = [sizes[k % 5] for k in range(n)]
    imgs = [rand_frame(w, h, 40 + k) for k, (w, h) in enumerate(shapes)]
    grids = np.stack([rand_grid(3, 2, 2.5, k) for k in range(n)])
    src_pitch = [pf.pitch_kinds(w)[(k // 4 + 2) % 5] for k, (w, h) in enumerate(shapes)]
    dst_pitch = [pf.pitch_kinds(w)[(k // 4) % 5] for k, (w, h) in enumerate(shapes)]
    fs = pf.PitchedFrames(imgs, src_pitch, offsets=[(k + 1) % 4 for k in range(n)], seed=11)
    fd = pf.PitchedFrames([np.zeros_like(i) for i in imgs], dst_pitch, offsets=[k % 4 for k in range(n)], seed=12)
    assert len({(k % 4, (k // 4) % 5) for k in range(n)}) == 20           # every base offset meets every destination pitch kind
    ts, sp = fs.to_device(torch)
    td, dp = fd.to_device(torch)
    w, h, _ = fs.geom()
    cnt = ctx.ApplyLocalWarpsDev(sp, dp, w, h, fs.ws, fd.ws, grids)
    got_s, got_d = fs.device_bytes(ts), fd.device_bytes(td)
    pix = np.zeros(fd.nbytes, bool)
    for k in range(n):
        want, nc = lr.apply(imgs[k], grids[k])
        assert np.array_equal(fd.pixels(k, got_d), want), (k, shapes[k], src_pitch[k], dst_pitch[k])
        assert cnt[k] == nc
        fd.view(k, pix)[:, :fd.row_bytes(k)] = True
    assert np.array_equal(got_d[~pix], fd.buf[~pix])                          # row padding and the gaps between frames
    assert np.array_equal(got_s, fs.buf)
    # the same frames in place on the source's pitches
    cnt2 = ctx.ApplyLocalWarpsDev(sp, sp, w, h, fs.ws, fs.ws, grids)
    got_s = fs.device_bytes(ts)
    pix = np.zeros(fs.nbytes, bool)
    for k in range(n):
        assert np.array_equal(fs.pixels(k, got_s), fd.pixels(k, got_d)), k
        fs.view(k, pix)[:, :fs.row_bytes(k)] = True
    assert np.array_equal(cnt2, cnt) and np.array_equal(got_s[~pix], fs.buf[~pix])


def test_mixed_sizes_in_one_call_equal_single_calls(env):
    torch, im, ctx = env
    rng = np.random.default_rng(8)
    sizes = [(9, 7), (300, 200), (9, 200), (300, 7), (BW + 1, 9), (10, 8)] + [(int(rng.integers(9, 301)), int(rng.integers(7, 201))) for _ in range(24)]
    imgs = [rand_frame(w, h, 100 + k) for k, (w, h) in enumerate(sizes)]
    grids = [rand_grid(8, 6, 4.0, 200 + k) for k in range(len(sizes))]
    got, cnt = check_apply(env, imgs, grids)
    assert cnt.any()
    for k in (0, 1, 4, 17, 29):
        one, c1 = run_apply(env, [imgs[k]], [grids[k]])
        assert np.array_equal(one[0], got[k]) and c1[0] == cnt[k], k
    # frames 0, 2, 4 .. in place (a pitch of their own), the others out of place
    src = [torch.from_numpy(np.pad(i.reshape(i.shape[0], -1), ((0, 0), (0, 5)), constant_values=77)).cuda() for i in imgs]
    dst = [s if k % 2 == 0 else torch.full((s.shape[0], s.shape[1] + 3), 88, dtype=torch.uint8, device="cuda") for k, s in enumerate(src)]
    torch.cuda.synchronize()
    w = [x for x, _ in sizes]; h = [y for _, y in sizes]
    cc = ctx.ApplyLocalWarpsDev([s.data_ptr() for s in src], [d.data_ptr() for d in dst], w, h, [s.shape[1] for s in src], [d.shape[1] for d in dst], np.stack(grids))
    assert np.array_equal(cc, cnt)
    for k in range(len(imgs)):
        full = dst[k].cpu().numpy()
        assert np.array_equal(full[:, :3 * w[k]].reshape(imgs[k].shape), got[k]), k
        assert (full[:, 3 * w[k]:] == (77 if k % 2 == 0 else 88)).all(), k
    assert len(ctx.ApplyLocalWarpsDev([], [], [], [], [], [], np.zeros((0, 7, 9, 2), np.float32))) == 0


# ---- tie_residual_kernel -------------------------------------------------------------------------------------------------------------------
def stats_dev(env, rec, w, h, h9s, **p):
    torch, im, ctx = env
    q = dict(lr.DEFAULTS, **p)
    n_vals = im.local_warp_stats_len(len(w), q["grid_x"], q["grid_y"])
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).cuda() if len(rec) else None
    out = torch.full((n_vals + 4,), 0x5a5a5a5a, dtype=torch.int64, device="cuda")       # garbage the call must clear, and a guard behind it
    torch.cuda.synchronize()
    ctx.TieResidualStatsDev(d_rec.data_ptr() if d_rec is not None else 0, len(rec), w, h, h9s, out.data_ptr(), **p)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[n_vals:] == 0x5a5a5a5a).all()
    return got[:n_vals]


def test_statistics_on_records_for_every_branch(env):
    torch, im, ctx = env
    e = lc.edge_case()
    want = lr.stats(e["rec"], e["w"], e["h"], e["h9s"], **e["params"])
    got = stats_dev(env, e["rec"], e["w"], e["h"], e["h9s"], **e["params"])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert got[-8] == e["n_skipped"]
    NN, sd = 63, lr.stride(8, 6)
    tails = got[:-8].reshape(e["n"], sd)[:, 7 * NN:]
    assert (tails[:, 2:5] > 0).any(0).all() and (e["rec"]["n_in"] == 400).any() and (e["rec"]["n_in"] == 1).any()
    assert tails[5, 0] == 4 and tails[5, 2:5].tolist() == [0, 2, 6]           # the ties one float32 step on either side of both thresholds
    assert np.array_equal(got, im.tie_residual_stats_host(e["rec"], e["w"], e["h"], e["h9s"], **e["params"]))
    # the same records in another order, and each alone: the sums add
    rec = e["rec"][::-1].copy()
    assert np.array_equal(stats_dev(env, rec, e["w"], e["h"], e["h9s"], **e["params"]), want)
    # no records: zeros, nothing launched; no frames
    assert not stats_dev(env, e["rec"][:0], e["w"], e["h"], e["h9s"], **e["params"]).any()
    assert not stats_dev(env, e["rec"][:0], [], [], np.zeros((0, 9), np.float32)).any()


@pytest.mark.parametrize("grid", [(8, 6), (1, 1), (16, 16), (3, 2)])
def test_statistics_of_a_survey(env, grid):
    torch, im, ctx = env
    s = lc.survey(seed=2)
    p = dict(grid_x=grid[0], grid_y=grid[1])
    got = stats_dev(env, s["rec"], s["w"], s["h"], s["h9s"], **p)
    assert np.array_equal(got, lr.stats(s["rec"], s["w"], s["h"], s["h9s"], **p))
    assert np.array_equal(got, im.tie_residual_stats_host(s["rec"], s["w"], s["h"], s["h9s"], **p))


# ---- the whole step -----------------------------------------------------------------------------------------------------------------------
def frames_to_device(torch, imgs, pad=4):
    t = [torch.from_numpy(np.pad(i.reshape(i.shape[0], -1), ((0, 0), (0, pad)), constant_values=66)).cuda() for i in imgs]
    torch.cuda.synchronize()
    return t


def test_local_register_end_to_end(env):
    torch, im, ctx = env
    s = lc.survey(seed=4)
    h9s = s["h9s"].copy()
    w, h = list(s["w"]), list(s["h"])
    imgs = [rand_frame(w[k], h[k], 300 + k) for k in range(s["n"])]
    st = lr.stats(s["rec"], w, h, h9s)
    grids, _, reps = lr.solve(st, s["n"])
    dev = frames_to_device(torch, imgs)
    d_rec = torch.from_numpy(s["rec"].view(np.uint8).copy()).cuda()
    g, rep = ctx.LocalRegisterDev(d_rec.data_ptr(), len(s["rec"]), [t.data_ptr() for t in dev], w, h, [3 * x + 4 for x in w], h9s)
    assert np.array_equal(lr.node_q8(g), lr.node_q8(grids)) and lr.node_q8(g).any()
    for k in range(s["n"]):
        full = dev[k].cpu().numpy()
        assert np.array_equal(full[:, :3 * w[k]].reshape(imgs[k].shape), lr.apply(imgs[k], grids[k])[0]), k
        assert (full[:, 3 * w[k]:] == 66).all()
        assert rep["n_ties"][k] == reps[k]["n_ties"] and rep["solved"][k] == 1 and abs(rep["rms_after"][k] - reps[k]["rms_after"]) < 1e-6
    # a frame that takes no part is not touched and may be missing; one below min_ties keeps its bytes
    h9s[5, 8] = 0.0
    st = lr.stats(s["rec"], w, h, h9s)
    cut = sorted(int(st[k * lr.stride(8, 6) + 7 * 63]) for k in range(5))[2]      # the median of the five frames' kept sides
    grids, _, reps = lr.solve(st, s["n"], **dict(lr.DEFAULTS, min_ties=cut))
    assert 1 <= sum(r["solved"] for r in reps) < 5 and reps[5]["n_ties"] == 0
    dev = frames_to_device(torch, imgs)
    ptrs = [t.data_ptr() for t in dev]
    ptrs[5] = 0
    g, rep = ctx.LocalRegisterDev(d_rec.data_ptr(), len(s["rec"]), ptrs, w, h, [3 * x + 4 for x in w], h9s, min_ties=cut)
    assert np.array_equal(lr.node_q8(g), lr.node_q8(grids)) and not g[5].any()
    for k in range(s["n"]):
        want = lr.apply(imgs[k], grids[k])[0] if reps[k]["solved"] else imgs[k]
        assert np.array_equal(dev[k].cpu().numpy()[:, :3 * w[k]].reshape(imgs[k].shape), want), k
    # no records: nothing moves
    g, rep = ctx.LocalRegisterDev(0, 0, [t.data_ptr() for t in dev[:2]], w[:2], h[:2], [3 * x + 4 for x in w[:2]], h9s[:2])
    assert not g.any() and not rep["solved"].any()


def test_refusals_leave_the_ctx_usable(env):
    torch, im, ctx = env
    w, h = 40, 30
    img = rand_frame(w, h, 50)
    buf = torch.zeros(8 * 4096, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    ws = 3 * w
    fb = ws * (h - 1) + 3 * w
    A, B, Cc = base, base + 4096, base + 8192
    zero = np.zeros((1, 3, 4, 2), np.float32)

    def refused(word, call):
        with pytest.raises(im.Mi355Error) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), (word, str(e.value))

    ap = ctx.ApplyLocalWarpsDev
    refused("d_src", lambda: ap([0], [B], [w], [h], [ws], [ws], zero))
    refused("d_dst", lambda: ap([A], [0], [w], [h], [ws], [ws], zero))
    refused("ws_src", lambda: ap([A], [B], [w], [h], [ws - 1], [ws], zero))
    refused("ws_dst", lambda: ap([A], [B], [w], [h], [ws], [ws - 1], zero))
    for bad in (1, 0, -4, (1 << 20) + 1):
        refused("w=", lambda: ap([A], [B], [bad], [h], [4 << 20], [4 << 20], zero))
        refused("h=", lambda: ap([A], [B], [w], [bad], [ws], [ws], zero))
    refused("grid_x", lambda: ap([A], [B], [w], [h], [ws], [ws], np.zeros((1, 3, 18, 2), np.float32)))
    refused("grid_y", lambda: ap([A], [B], [w], [h], [ws], [ws], np.zeros((1, 18, 3, 2), np.float32)))
    refused("grid_x", lambda: ap([A], [B], [w], [h], [ws], [ws], np.zeros((1, 3, 1, 2), np.float32)))
    refused("grid_x=3 > w-1", lambda: ap([A], [B], [3], [h], [ws], [ws], zero))
    refused("grid_y=2 > h-1", lambda: ap([A], [B], [w], [2], [ws], [ws], zero))
    for v in (float("nan"), float("inf"), 64.5, -65.0):
        g = zero.copy()
        g[0, 1, 2, 1] = v
        refused("grid value", lambda: ap([A], [B], [w], [h], [ws], [ws], g))
    refused("overlaps", lambda: ap([A, B], [Cc, A + fb - 1], [w] * 2, [h] * 2, [ws] * 2, [ws] * 2, np.repeat(zero, 2, 0)))
    refused("overlaps", lambda: ap([A], [A + 3], [w], [h], [ws], [ws], zero))
    refused("overlaps", lambda: ap([A], [A], [w], [h], [ws], [ws + 4], zero))
    refused("n=", lambda: ap([A] * 65536, [B] * 65536, [w] * 65536, [h] * 65536, [ws] * 65536, [ws] * 65536, np.zeros((65536, 2, 2, 2), np.float32)))
    L = ctx.L
    assert L.mi355_apply_local_warps_dev(ctx._h, None, None, None, None, None, None, 1, 3, 2, zero.ctypes.data_as(im.capi.C.c_void_p), None) == -1
    assert "d_src" in (L.mi355_last_error(ctx._h) or b"").decode()
    # the statistics and the whole step
    s = lc.survey(seed=1, n=2)
    d_rec = torch.from_numpy(s["rec"].view(np.uint8).copy()).cuda()
    out = torch.zeros(im.local_warp_stats_len(2, 8, 6), dtype=torch.int64, device="cuda")
    sd, rg = ctx.TieResidualStatsDev, ctx.LocalRegisterDev
    frames = frames_to_device(torch, [rand_frame(160, 120, k) for k in range(2)], pad=0)
    fp = [t.data_ptr() for t in frames]
    for word, kw in (("grid_x", dict(grid_x=0)), ("grid_y", dict(grid_y=17)), ("max_residual", dict(max_residual=float("nan"))), ("max_residual", dict(max_residual=-1.0)),
                     ("max_shift", dict(max_shift=0.0)), ("max_shift", dict(max_shift=65.0)), ("smooth", dict(smooth=-0.5)), ("smooth", dict(smooth=float("inf"))),
                     ("prior", dict(prior=0.0)), ("prior", dict(prior=float("nan"))), ("min_ties", dict(min_ties=-1))):
        refused(word, lambda: sd(d_rec.data_ptr(), 1, s["w"], s["h"], s["h9s"], out.data_ptr(), **kw))
        refused(word, lambda: rg(d_rec.data_ptr(), 1, fp, s["w"], s["h"], [480] * 2, s["h9s"], **kw))
    p = im.local_warp_params()
    p.reserved = 7
    refused("reserved", lambda: sd(d_rec.data_ptr(), 1, s["w"], s["h"], s["h9s"], out.data_ptr(), params=p))
    refused("results", lambda: sd(0, 1, s["w"], s["h"], s["h9s"], out.data_ptr()))
    refused("stats", lambda: sd(d_rec.data_ptr(), 1, s["w"], s["h"], s["h9s"], 0))
    refused("n_pairs", lambda: sd(d_rec.data_ptr(), -1, s["w"], s["h"], s["h9s"], out.data_ptr()))
    refused("grid_x=8 > w-1", lambda: sd(d_rec.data_ptr(), 1, [8, 160], s["h"], s["h9s"], out.data_ptr()))
    refused("h=", lambda: sd(d_rec.data_ptr(), 1, s["w"], [120, 1], s["h9s"], out.data_ptr()))
    refused("d_imgs", lambda: rg(d_rec.data_ptr(), 1, [fp[0], 0], s["w"], s["h"], [480] * 2, s["h9s"]))
    refused("ws=", lambda: rg(d_rec.data_ptr(), 1, fp, s["w"], s["h"], [480, 479], s["h9s"]))
    refused("d_results", lambda: rg(0, 1, fp, s["w"], s["h"], [480] * 2, s["h9s"]))
    for t, k in zip(frames, range(2)):
        assert np.array_equal(t.cpu().numpy().reshape(120, 160, 3), rand_frame(160, 120, k))         # no refusal touched a frame
    # and the same ctx runs good calls
    check_apply(env, [img], [rand_grid(3, 2, 2.0, 1)])
    assert np.array_equal(stats_dev(env, s["rec"], s["w"], s["h"], s["h9s"]), lr.stats(s["rec"], s["w"], s["h"], s["h9s"]))

"""GPU: the lens self-calibration's device half (csrc/calib.hip) against its host twin -- the blocks of tie_blocks_kernel<CalibFormer> and the whole
loop on device records give the same BITS as mi355_pair_calib_blocks_host and mi355_calibrate_lens_results -- and the stage end to end from
pixels."""
import numpy as np
import pytest

from tests import calib_cases as cc
from tests import calib_ref as cr

pytestmark = pytest.mark.gpu


def _to_dev(torch, recs):
    return torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1).copy()).cuda()


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


def _dev_blocks(ctx, torch, im, d_r, count, h8, cam):
    d_b = torch.full((count + 1, im.PAIR_CALIB_BLOCK.itemsize), 0xCD, dtype=torch.uint8, device="cuda")        # one record of guard
    torch.cuda.synchronize()
    ctx.PairCalibBlocksDev(d_r.data_ptr(), count, h8, cam, d_b.data_ptr())
    ctx.synchronize()
    got = d_b.cpu().numpy()
    assert (got[count] == 0xCD).all(), count
    return got[:count].reshape(-1).view(im.PAIR_CALIB_BLOCK)


@pytest.mark.parametrize("theta", [cc.CAM_START[4:], cc.THETA_TRUE, cc.THETA_BAD, (-0.1, 0.02, 0.001, -0.002, 0.01)])
def test_device_blocks_equal_host_blocks_on_edge_records(ctx, theta):
    import torch
    import imagemosaicing_amd as im
    recs, h8 = cc.edge_records()
    cam = im.Camera(*(cc.CAM_TRUE[:4] + tuple(theta)))
    d_r = _to_dev(torch, recs)
    want = im.pair_calib_blocks_host(recs, h8, cam)
    assert (want["n_in"] > 0).sum() == 16 and ((want["n_bad"] > 0).any() == (theta == cc.THETA_BAD))
    for count in cc.EDGE_COUNTS + (len(recs),):
        got = _dev_blocks(ctx, torch, im, d_r, count, h8, cam)
        assert got.tobytes() == want[:count].tobytes(), count


@pytest.mark.parametrize("theta", [cc.CAM_START[4:], cc.THETA_TRUE])
def test_device_blocks_equal_host_blocks_on_grid16(ctx, theta):
    import torch
    import imagemosaicing_amd as im
    recs = cc.survey("grid16", 0.5).copy()
    recs = np.concatenate([recs, recs[:5]])                     # records that are not accepted, in between after the shuffle
    recs["accepted"][-5:] = 0
    recs = recs[np.random.default_rng(3).permutation(len(recs))]
    h8 = np.array([cr.start_state(r["H"], cc.CAM_START) for r in recs])
    cam = im.Camera(*(cc.CAM_TRUE[:4] + tuple(theta)))
    want = im.pair_calib_blocks_host(recs, h8, cam)
    got = _dev_blocks(ctx, torch, im, _to_dev(torch, recs), len(recs), h8, cam)
    assert got.tobytes() == want.tobytes() and (want["n_in"] > 0).sum() == len(recs) - 5 and not want["n_bad"].any()


@pytest.mark.parametrize("name", ["grid16", "strip12"])
def test_device_calibration_equals_host_calibration_bit_for_bit(ctx, name):
    import torch
    import imagemosaicing_amd as im
    start = im.Camera(*cc.CAM_START)
    for noise in (0.0, 0.5):
        recs = cc.survey(name, noise).copy()
        recs = np.concatenate([recs, recs[:3]])                 # three records that are not accepted, for the compaction to drop
        recs["accepted"][-3:] = 0
        recs = recs[np.random.default_rng(4).permutation(len(recs))]
        d_r = _to_dev(torch, recs)
        for mask in (3, 15):
            want, wrep = im.calibrate_lens_results(recs, start, mask=mask)
            torch.cuda.synchronize()
            got, grep_ = ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), start, mask=mask)
            assert bytes(got) == bytes(want) and grep_ == wrep, (noise, mask, grep_, wrep)
            assert wrep["accepted"] >= 3 and wrep["n_pairs_used"] == len(recs) - 3 and wrep["n_unused_records"] == 0
    # ... and on a caller's stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        try:
            got, grep_ = ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), start, mask=mask)
        finally:
            ctx.set_stream(None)
    assert bytes(got) == bytes(want) and grep_ == wrep


def test_empty_input_unused_sets_and_refusals(ctx):
    import torch
    import imagemosaicing_amd as im
    start = im.Camera(520.0, 520.0, 256.0, 240.0, 0.01, -0.02, 0.001, 0.002, 0.003)
    edge, h8 = cc.edge_records()
    unused = np.concatenate([edge[[5, 15, 16, 17, 18, 21]], cc.bad_scale_records()])
    d_u = _to_dev(torch, unused)
    recs = cc.survey("strip12", 0.5)
    d_r = _to_dev(torch, recs)
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    zero = dict(trials=0, accepted=0, n_pairs_used=0, n_unused_records=0, n_points=0, cost0=0.0, cost=0.0) | {"lambda": 0.0}
    for ptr, n in ((0, 0), (d_u.data_ptr(), len(unused))):
        out, rep = ctx.CalibrateLensDev(ptr, n, start)
        assert bytes(out) == bytes(start) and rep == zero
    ctx.PairCalibBlocksDev(0, 0, None, start, 0)
    assert ctx.profile_get("calibrate")[1] == 0                 # nothing launched
    # refusals come before any launch and leave the ctx usable
    good = im.Camera(*cc.CAM_START)
    for text, kw in (("mask = 0", dict(mask=0)), ("mask = 32", dict(mask=32)), ("min_ties = 7", dict(min_ties=7)), ("min_ties = 401", dict(min_ties=401)),
                     ("max_iters = -1", dict(max_iters=-1)), ("lambda0 = ", dict(lambda0=-1.0)), ("lambda_up = ", dict(lambda_up=1.0)),
                     ("lambda_down = ", dict(lambda_down=float("nan"))), ("min_rel_decrease = ", dict(min_rel_decrease=-1e-3))):
        with pytest.raises(im.Mi355Error, match=text) as e:
            ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), good, **kw)
        assert e.value.code == -1
    for k, name in enumerate(cr.CAM_FIELDS):
        cam = list(cc.CAM_START)
        cam[k] = float("inf") if k & 1 else float("nan")
        with pytest.raises(im.Mi355Error, match="camera %s = " % name):
            ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), im.Camera(*cam))
        with pytest.raises(im.Mi355Error, match="camera %s = " % name):
            ctx.PairCalibBlocksDev(d_r.data_ptr(), len(recs), h8[:len(recs)], im.Camera(*cam), d_u.data_ptr())
    with pytest.raises(im.Mi355Error, match="camera fx = 0"):
        ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), im.Camera(0.0, *cc.CAM_START[1:]))
    with pytest.raises(im.Mi355Error, match="camera fy = -1"):
        ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), im.Camera(520.0, -1.0, *cc.CAM_START[2:]))
    for text, args in (("n_pairs = -1", (d_r.data_ptr(), -1, good)), ("n_pairs = 4 with NULL records", (0, 4, good)), ("NULL camera", (d_r.data_ptr(), 4, None))):
        with pytest.raises(im.Mi355Error, match=text):
            ctx.CalibrateLensDev(*args)
    for text, args in (("n = -2", (d_r.data_ptr(), -2, h8, good, d_u.data_ptr())), ("NULL records", (0, 3, h8, good, d_u.data_ptr())),
                       ("NULL h8", (d_r.data_ptr(), 3, None, good, d_u.data_ptr())), ("NULL out", (d_r.data_ptr(), 3, h8, good, 0)),
                       ("NULL camera", (d_r.data_ptr(), 3, h8, None, d_u.data_ptr())), ("min_ties = 3", (d_r.data_ptr(), 3, h8, good, d_u.data_ptr(), 3))):
        with pytest.raises(im.Mi355Error, match=text):
            ctx.PairCalibBlocksDev(*args)
    assert ctx.profile_get("calibrate")[1] == 0
    # bad ties at the start camera: MI355_ERR_FAILED naming record and tie, from the records in HBM
    with pytest.raises(im.Mi355Error, match=r"record 0 \(0, 1\).*the first is tie \d+ ") as e:
        ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), im.Camera(*(cc.CAM_TRUE[:4] + cc.THETA_BAD)))
    assert e.value.code == -2
    with pytest.raises(im.Mi355Error) as e2:
        im.calibrate_lens_results(recs, im.Camera(*(cc.CAM_TRUE[:4] + cc.THETA_BAD)))
    assert str(e2.value) == str(e.value) and ctx.profile_get("calibrate")[1] == 1
    # the following good call
    ctx.profile_reset()
    want, wrep = im.calibrate_lens_results(recs, good)
    got, rep = ctx.CalibrateLensDev(d_r.data_ptr(), len(recs), good)
    launches = ctx.profile_get("calibrate")[1]
    ctx.profile_enable(False)
    assert bytes(got) == bytes(want) and rep == wrep and rep["accepted"] >= 3
    assert launches == rep["trials"] + 1                         # one launch for the start and one per trial


def test_survey_end_to_end(ctx):
    """six rendered frames of one strip, resampled through a camera with k1 = +0.08 as a stand-in for a lens (the truth is then outside the
    model family: no truth comparison): extract, match, calibrate on the records in HBM.  The device result is the host form's on the records
    copied back; the rms falls; and after undistorting the frames with the estimate, a second calibration finds less left to correct.
    Measured on an MI355X (DESIGN, "Lens self-calibration"): first k1 = -0.0779, k2 = 0.0128, rms 0.976 -> 0.253 px, largest map displacement
    16.56 px; second rms 0.2524 -> 0.2522 px, largest map displacement 0.064 px."""
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    w, h, F = 640, 480, 6
    frames, A, gains, ws = render_frames(ctx, torch, F, w, h, per_row=F)
    lens = im.Camera(520.0, 520.0, 319.5, 239.5, 0.08, 0.0, 0.0, 0.0, 0.0)
    start = im.Camera(520.0, 520.0, 319.5, 239.5, 0.0, 0.0, 0.0, 0.0, 0.0)
    ptrs, ww, hh, wss = [frames[k].data_ptr() for k in range(F)], [w] * F, [h] * F, [ws] * F
    shot = torch.empty_like(frames)
    sptrs = [shot[k].data_ptr() for k in range(F)]
    ctx.UndistortFramesDev(ptrs, sptrs, ww, hh, wss, wss, lens)
    pairs = im.pair_schedule(F, F)

    def calibrate(fptrs):
        for k in range(F):
            ctx.SiftExtractDev(k, fptrs[k], w, h, ws)
        res = torch.zeros((len(pairs), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 3)
        ctx.synchronize()
        got, rep = ctx.CalibrateLensDev(res.data_ptr(), len(pairs), start)
        r = res.cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
        want, wrep = im.calibrate_lens_results(r, start)
        assert bytes(got) == bytes(want) and rep == wrep
        return got, rep

    est1, rep1 = calibrate(sptrs)
    rms = lambda rep: (np.sqrt(rep["cost0"] / rep["n_points"]), np.sqrt(rep["cost"] / rep["n_points"]))
    move1 = cc.map_error(cr.cam_tuple(est1), cr.cam_tuple(start))
    print("first:", cr.cam_tuple(est1)[4:6], rep1, "rms %.4f -> %.4f px, largest map displacement %.3f px" % (rms(rep1) + (move1,)))
    assert rep1["n_pairs_used"] >= 4 and rep1["accepted"] >= 1 and rms(rep1)[1] < rms(rep1)[0]
    fixed = torch.empty_like(frames)
    fptrs = [fixed[k].data_ptr() for k in range(F)]
    ctx.UndistortFramesDev(sptrs, fptrs, ww, hh, wss, wss, est1)
    est2, rep2 = calibrate(fptrs)
    move2 = cc.map_error(cr.cam_tuple(est2), cr.cam_tuple(start))
    print("second:", cr.cam_tuple(est2)[4:6], rep2, "rms %.4f -> %.4f px, largest map displacement %.3f px" % (rms(rep2) + (move2,)))
    assert move2 < move1

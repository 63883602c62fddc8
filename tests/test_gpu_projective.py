"""GPU: the projective refinement's device half (csrc/projective.hip) against its host twin -- the blocks of tie_blocks_kernel<NormalFormer> and
the whole loop on device records give the same BITS as mi355_pair_normal_blocks_host and mi355_global_projective_refine_results."""
import numpy as np
import pytest

from tests import projective_cases as pc
from tests import projective_ref as pr

pytestmark = pytest.mark.gpu


def _to_dev(torch, recs):
    return torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1).copy()).cuda()


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


def test_device_blocks_equal_host_blocks_bit_for_bit(ctx):
    import torch
    import imagemosaicing_amd as im
    recs, h8, part = pc.edge_records()
    d_r = _to_dev(torch, recs)
    want = im.pair_normal_blocks_host(recs, h8, part)
    assert (want["n_in"] > 0).sum() > 150 and int(want["n_in"][9]) == 401
    for count in pc.EDGE_COUNTS:
        d_b = torch.full((count + 1, im.PAIR_NORMAL_BLOCK.itemsize), 0xCD, dtype=torch.uint8, device="cuda")        # one record of guard
        torch.cuda.synchronize()
        ctx.PairNormalBlocksDev(d_r.data_ptr(), count, h8, part, d_b.data_ptr())
        ctx.synchronize()
        got = d_b.cpu().numpy()
        assert (got[count] == 0xCD).all(), count
        assert got[:count].reshape(-1).view(im.PAIR_NORMAL_BLOCK).tobytes() == want[:count].tobytes(), count


@pytest.mark.parametrize("name", ["grid16", "strip12"])
def test_device_refinement_equals_host_refinement_bit_for_bit(ctx, name):
    import torch
    import imagemosaicing_amd as im
    for noise in (0.0, 0.5):
        s = pc.survey(name, noise)
        recs = s["recs"].copy()
        recs = np.concatenate([recs, recs[:3]])                 # three records that are not accepted, for the compaction to drop
        recs["accepted"][-3:] = 0
        recs = recs[np.random.default_rng(4).permutation(len(recs))]
        d_r = _to_dev(torch, recs)
        for prior in (0.0, 0.01):
            p = im.projective_params(prior=prior)
            want, wrep = im.global_projective_refine_results(recs, s["w"], s["h"], s["start"], params=p)
            torch.cuda.synchronize()
            got, grep_ = ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(recs), s["w"], s["h"], s["start"], params=p)
            assert got.tobytes() == want.tobytes() and grep_ == wrep, (noise, prior, grep_, wrep)
            assert wrep["accepted"] >= 1 and wrep["n_pairs_used"] == len(s["recs"])
    # ... and on a caller's stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        try:
            got, grep_ = ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(recs), s["w"], s["h"], s["start"], params=p)
        finally:
            ctx.set_stream(None)
    assert got.tobytes() == want.tobytes() and grep_ == wrep


def test_device_refinement_errors_and_empty_input(ctx):
    import torch
    import imagemosaicing_amd as im
    s = pc.survey("strip12", 0.5)
    bad = s["recs"].copy()
    bad["n_in"][2] = 401
    d_r = _to_dev(torch, bad)
    torch.cuda.synchronize()
    with pytest.raises(im.Mi355Error, match="n_in = 401"):
        ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(bad), s["w"], s["h"], s["start"])
    with pytest.raises(im.Mi355Error, match="lambda_up"):
        ctx.GlobalProjectiveRefineDev(d_r.data_ptr(), len(bad), s["w"], s["h"], s["start"], params=im.projective_params(lambda_up=1.0))
    out, rep = ctx.GlobalProjectiveRefineDev(0, 0, s["w"], s["h"], s["start"])
    assert out.tobytes() == s["start"].tobytes() and all(v == 0 for v in rep.values())


def test_survey_end_to_end(ctx):
    """six rendered frames of 640 x 480 (tests/synth_survey.py: yaw, scale, sensor noise): extract, match, align affinely, refine on the
    records in HBM; the data cost falls, and the output is the host form's on the records copied back"""
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import render_frames
    w, h, F = 640, 480, 6
    frames, A, gains, ws = render_frames(ctx, torch, F, w, h, per_row=3)
    for k in range(F):
        ctx.SiftExtractDev(k, frames[k].data_ptr(), w, h, ws)
    pairs = im.pair_schedule(F, F)
    res = torch.zeros((len(pairs), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.MatchPairsDev(pairs, res.data_ptr(), 2.5, 3)
    ctx.synchronize()
    r = res.cpu().numpy().reshape(-1).view(im.PAIR_RESULT)
    label = im.select_connected_results(r, F)
    assert label.sum() >= 4
    fixed = [1 if (k == 0 or label[k] == 0) else 0 for k in range(F)]
    start = im.global_affine_align_results(r, F, fixed=fixed, label=label)
    ww, hh = np.full(F, w, np.int32), np.full(F, h, np.int32)
    got, rep = ctx.GlobalProjectiveRefineDev(res.data_ptr(), len(pairs), ww, hh, start, fixed=fixed, label=label)
    print("end to end:", rep, "rms %.4g -> %.4g px" % (np.sqrt(rep["cost0"] / rep["n_points"]), np.sqrt(rep["cost_data"] / rep["n_points"])))
    assert rep["n_free"] >= 3 and rep["cost_data"] < rep["cost0"]
    want, wrep = im.global_projective_refine_results(r, ww, hh, start, fixed=fixed, label=label)
    assert got.tobytes() == want.tobytes() and rep == wrep
    move = np.abs(pr.corners(pr.transforms_h8(got), ww, hh) - pr.corners(pr.transforms_h8(start), ww, hh)).max()
    print("largest corner move from the affine start %.3g px" % move)

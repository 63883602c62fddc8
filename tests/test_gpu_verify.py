"""GPU: pair verification (include/mi355_mosaic.h, "pair verification").  The kernels against their host twins and the numpy restatement
(tests/verify_ref.py) byte for byte; the loop's device form against its host form and the reference; its output against the existing
select-connected and alignment functions on the kept records alone; the demotion convention; the refusals; and the effect on the corners
of surveys with 10 % wrong pairs (tests/verify_cases.py)."""
import numpy as np
import pytest

from tests import verify_cases as vc
from tests import verify_ref as vr

pytestmark = pytest.mark.gpu

SURVEYS = [("grid36", 2, 0), ("grid36", 2, 10), ("strip40d", 2, 0), ("strip40d", 2, 10), ("strip_adjacent", 2, 0), ("strip_adjacent", 2, 10)]
_cache = {}


def survey(name, seed, pct):
    """a survey with the reference's result and the host form's, formed once"""
    import imagemosaicing_amd as im
    key = (name, seed, pct)
    if key not in _cache:
        s = vc.survey(name, seed, pct)
        s["ref"] = vr.verify(s["recs"], s["n"])
        s["host"] = im.verify_pairs_results(s["recs"], s["n"])
        _cache[key] = s
    return _cache[key]


def _to_dev(torch, recs):
    return torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1).copy()).cuda()


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


def test_edges_device_host_reference_byte_for_byte(ctx):
    import torch
    import imagemosaicing_amd as im
    recs = vc.edge_records()
    want = vr.edges(recs, vc.EDGE_IMAGES)
    host = im.pair_edges_host(recs, vc.EDGE_IMAGES)
    assert host.tobytes() == want.tobytes()
    f = want["flags"]
    assert (f == 3).sum() > 150 and (f == 0).sum() > 40 and f[14] == 1 and f[15] == 1 and f[16] == 3 and f[17] == 1 and f[18] == 1
    assert not f[[9, 10, 11, 12, 13]].any() and int(want["n_in"][9]) == 401
    d_r = _to_dev(torch, recs)
    for count in vc.EDGE_COUNTS:
        d_e = torch.full((count + 1, im.PAIR_EDGE.itemsize), 0xCD, dtype=torch.uint8, device="cuda")        # one record of guard
        torch.cuda.synchronize()
        ctx.PairEdgesDev(d_r.data_ptr(), count, vc.EDGE_IMAGES, d_e.data_ptr())
        ctx.synchronize()
        got = d_e.cpu().numpy()
        assert (got[count] == 0xCD).all(), count
        assert got[:count].tobytes() == want[:count].tobytes(), count


def _cycles_three_ways(ctx, edg, n, tol=6.0):
    import imagemosaicing_amd as im
    want = vr.cycles(edg, n, tol)
    host = im.pair_cycles_host(edg, n, tol)
    dev = ctx.PairCyclesDev(edg, n, tol)
    assert host.tobytes() == want.tobytes()
    assert dev.tobytes() == want.tobytes()
    return want


@pytest.mark.parametrize("n_common", [0, 1, 63, 64, 65, 300])
def test_cycles_common_neighbour_counts(ctx, n_common):
    edg, n = vc.translation_graph(n_common, err=(3.0, 4.0), seed=n_common)
    c = _cycles_three_ways(ctx, edg, n, 6.0)
    assert (int(c["n_ok"][0]), int(c["n_bad"][0])) == (n_common, 0)
    assert c["min_e2"][0] == (25.0 if n_common else np.inf)
    if n_common:                                  # every other edge is in exactly one triangle (with the edge (0, 1))
        assert (c["n_ok"][1:] + c["n_bad"][1:] == 1).all()


def test_cycles_tolerance_is_inclusive(ctx):
    edg, n = vc.translation_graph(5, err=(6.0, 0.0), seed=3)
    c = _cycles_three_ways(ctx, edg, n, 6.0)
    assert (int(c["n_ok"][0]), int(c["n_bad"][0]), float(c["min_e2"][0])) == (5, 0, 36.0)
    # one step to the other side: integer translations cannot give E = nextafter(36), so the tolerance moves instead -- the largest
    # tolerance whose square is below E = 36 makes the same triangles BAD
    below = float(np.nextafter(6.0, 0.0))
    assert below * below < 36.0 and float(np.nextafter(below * below, np.inf)) <= 36.0
    c = _cycles_three_ways(ctx, edg, n, below)
    assert (int(c["n_ok"][0]), int(c["n_bad"][0]), float(c["min_e2"][0])) == (0, 5, 36.0)


def test_cycles_star_and_special_graphs(ctx):
    edg, n = vc.star_graph(400, 2)
    c = _cycles_three_ways(ctx, edg, n)
    assert (int(c["n_ok"][0]), int(c["n_bad"][0])) == (1, 0) and c["min_e2"][0] == 0.0
    edg, n = vc.star_graph(400, 70)                     # the shorter list is longer than a wave
    c = _cycles_three_ways(ctx, edg, n)
    assert (int(c["n_ok"][0]), int(c["n_bad"][0])) == (69, 0)
    edg, n = vc.special_graph()
    c = _cycles_three_ways(ctx, edg, n)
    assert [int(v) for v in c["n_ok"][:3]] == [1, 1, 1] and c["min_e2"][1] == 0.0          # the triangle 0-1-2 from each of its edges
    assert int(c["n_bad"][0]) == 1                     # ... and the edge (0, 1) has the horizon triangle over frame 3: BAD, no E
    assert c["min_e2"][0] == 0.0
    assert (int(c["n_ok"][5]), int(c["n_bad"][5])) == (1, 0)          # the zero-area box
    assert (int(c["n_ok"][8]), int(c["n_bad"][8]), float(c["min_e2"][8])) == (0, 0, np.inf)          # not testable
    assert (int(c["n_ok"][9]), int(c["n_bad"][9])) == (0, 0)          # no common neighbour


def test_cycles_both_orientations_of_a_triangle(ctx):
    base, n = vc.special_graph()
    tri = base[:3].copy()
    for mask in range(8):                               # every edge of the triangle stored either way round
        e = tri.copy()
        for q in range(3):
            if mask >> q & 1:
                e["i"][q], e["j"][q] = tri["j"][q], tri["i"][q]
                e["F"][q], e["B"][q] = tri["B"][q], tri["F"][q]
        c = _cycles_three_ways(ctx, e, 3)
        assert [int(v) for v in c["n_ok"]] == [1, 1, 1] and not c["n_bad"].any(), mask
        assert c["min_e2"].tolist() == [0.0, 0.0, 0.0], mask


def test_cycles_duplicate_pair_is_refused(ctx):
    import imagemosaicing_amd as im
    edg, n = vc.translation_graph(3)
    dup = np.concatenate([edg, edg[2:3]])
    dup["i"][-1], dup["j"][-1] = edg["j"][2], edg["i"][2]          # the same unordered pair, the other way round
    with pytest.raises(im.Mi355Error, match="records 2 and %d" % (len(dup) - 1)):
        ctx.PairCyclesDev(dup, n)
    with pytest.raises(im.Mi355Error, match="records 2 and %d" % (len(dup) - 1)):
        im.pair_cycles_host(dup, n)
    bad = edg.copy()
    bad["j"][1] = n                                      # a testable edge that names a frame outside the table never reaches a kernel
    with pytest.raises(im.Mi355Error, match="edge 1"):
        ctx.PairCyclesDev(bad, n)
    assert ctx.PairCyclesDev(edg, n).tobytes() == im.pair_cycles_host(edg, n).tobytes()          # the ctx works afterwards


def test_residuals_device_host_reference_byte_for_byte(ctx):
    import torch
    import imagemosaicing_amd as im
    recs = vc.edge_records()
    h9, label = vc.edge_transforms()
    d_r = _to_dev(torch, recs)
    for lb in (label, None):
        want = vr.residuals(recs, h9, lb)
        host = im.pair_residuals_host(recs, h9, lb)
        assert host.tobytes() == want.tobytes()
        assert (want["n_used"] > 0).sum() > 120 and want["n_used"][19] == 0 and want["n_den"][23] > 0 and want["n_used"][23] > 0
        for count in vc.EDGE_COUNTS:
            d_o = torch.full((count + 1, im.PAIR_RESIDUAL.itemsize), 0xCD, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.PairResidualsDev(d_r.data_ptr(), count, h9, lb, d_o.data_ptr())
            ctx.synchronize()
            got = d_o.cpu().numpy()
            assert (got[count] == 0xCD).all(), count
            assert got[:count].tobytes() == want[:count].tobytes(), count


@pytest.mark.parametrize("name,seed,pct", SURVEYS)
def test_loop_device_equals_host_equals_reference(ctx, name, seed, pct):
    import torch
    import imagemosaicing_amd as im
    s = survey(name, seed, pct)
    recs, n, ref = s["recs"], s["n"], s["ref"]
    h_out, h_label, h_tr, h_rep, h_sum = s["host"]
    d_r = _to_dev(torch, recs)
    d_o = torch.full((len(recs) + 1, im.PAIR_RESULT.itemsize), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    label, tr, rep, summ = ctx.VerifyPairsDev(d_r.data_ptr(), len(recs), n, d_o.data_ptr())
    got = d_o.cpu().numpy()
    assert (got[len(recs)] == 0xCD).all()
    out = got[:len(recs)].reshape(-1).view(im.PAIR_RESULT)
    # the device form == the host form, byte for byte
    assert out.tobytes() == h_out.tobytes() and label.tobytes() == h_label.tobytes() and tr.tobytes() == h_tr.tobytes()
    assert rep.tobytes() == h_rep.tobytes() and summ.tobytes() == h_sum.tobytes()
    # ... == the reference's decisions
    assert np.array_equal(rep["verdict"], ref["verdict"]) and np.array_equal(label, ref["label"]) and np.array_equal(rep["round"], ref["round"])
    assert np.array_equal(rep["n_ok"], ref["n_ok"]) and np.array_equal(rep["n_bad"], ref["n_bad"]) and int(summ["rounds"]) == ref["rounds"]
    assert rep["min_e2"].tobytes() == ref["min_e2"].tobytes()
    assert [int(v) for v in summ["count"][:6]] == [int((ref["verdict"] == v).sum()) for v in range(6)]
    # the output is what the existing functions give for the kept records alone
    kept = np.isin(rep["verdict"], vr.KEPT_VERDICTS)
    want_label = im.select_connected_results(recs[kept], n)
    assert label.tobytes() == want_label.tobytes()
    assert tr.tobytes() == im.global_affine_align_results(recs[kept], n, label=want_label).tobytes()
    assert tr.tobytes() == im.global_affine_align_results(out, n, label=im.select_connected_results(out, n)).tobytes()
    # demoted records follow tie refinement's convention, the others are byte-identical
    assert out[kept].tobytes() == recs[kept].tobytes()
    dem = out[~kept]
    assert not dem["ok"].any() and not dem["accepted"].any() and not dem["H"].any()
    back = dem.copy()
    back["ok"], back["accepted"], back["H"] = recs["ok"][~kept], recs["accepted"][~kept], recs["H"][~kept]
    assert back.tobytes() == recs[~kept].tobytes()
    # in place == out of place
    label2, tr2, rep2, summ2 = ctx.VerifyPairsDev(d_r.data_ptr(), len(recs), n, d_r.data_ptr())
    assert d_r.cpu().numpy().tobytes() == out.tobytes() and rep2.tobytes() == rep.tobytes() and tr2.tobytes() == tr.tobytes()
    if name == "strip_adjacent" and pct == 0:
        assert (rep["verdict"] == im.VERDICT_BRIDGE).all() and int(summ["count"][im.VERDICT_VERIFIED]) == 0 and label.all()
    if pct == 0:                                        # nothing to find: the plain alignment's bits
        assert kept.all()
        assert tr.tobytes() == im.global_affine_align_results(recs, n, label=im.select_connected_results(recs, n)).tobytes()


@pytest.mark.parametrize("name", ["grid36", "strip40d"])
def test_effect_on_the_corners(ctx, name):
    import imagemosaicing_amd as im
    s = survey(name, 2, 10)
    recs, n = s["recs"], s["n"]
    _, label, tr, rep, _ = s["host"]
    kept = np.isin(rep["verdict"], vr.KEPT_VERDICTS)
    assert np.array_equal(kept, ~s["wrong"]) and label.all()
    right = recs[~s["wrong"]]
    clean = im.global_affine_align_results(right, n, label=im.select_connected_results(right, n))
    assert tr.tobytes() == clean.tobytes()
    plain = im.global_affine_align_results(recs, n, label=im.select_connected_results(recs, n))
    e_plain, e_ver = vc.corner_error(plain, s["G"]), vc.corner_error(tr, s["G"])
    print("%s: corner error %.1f px plain, %.1f px verified" % (name, e_plain, e_ver))
    assert e_plain > 10 * e_ver


def test_refusals_leave_the_ctx_usable(ctx):
    import torch
    import imagemosaicing_amd as im
    s = survey("grid36", 2, 10)
    recs, n = s["recs"], s["n"]
    d_r = _to_dev(torch, recs)
    d_o = torch.zeros((len(recs), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def both(match, recs_=None, d=None, n_pairs=None, n_images=n, out=True, **kw):
        r = recs if recs_ is None else recs_
        with pytest.raises(im.Mi355Error, match=match) as e:
            ctx.VerifyPairsDev((d_r if d is None else d).data_ptr(), len(r) if n_pairs is None else n_pairs, n_images, d_o.data_ptr() if out else 0, **kw)
        assert e.value.code == -1
        if out and n_pairs is None:
            with pytest.raises(im.Mi355Error, match=match):
                im.verify_pairs_results(r, n_images, **kw)
    for field in ("cycle_tol", "gate_abs", "gate_k"):
        for v in (0.0, -1.0, np.nan, np.inf):
            both(field, **{field: v})
    both("max_rounds", max_rounds=0)
    both("n_images", n_images=0)
    both("n_images", n_images=65536)
    both("n_pairs", n_pairs=-1)
    both("NULL", out=False)
    bad = recs.copy()
    bad["n_in"][3] = 401
    both("record 3", bad, _to_dev(torch, bad))
    bad = recs.copy()
    bad["j"][5] = n
    both("record 5", bad, _to_dev(torch, bad))
    dup = np.concatenate([recs, recs[7:8]])
    d_dup = _to_dev(torch, dup)
    d_o = torch.zeros((len(dup), im.PAIR_RESULT.itemsize), dtype=torch.uint8, device="cuda")
    both("records 7 and %d" % (len(dup) - 1), dup, d_dup)
    # nothing usable at all: MI355_ERR_FAILED, and the ctx still works
    none = recs.copy()
    none["accepted"] = 0
    with pytest.raises(im.Mi355Error, match="no pair could be verified") as e:
        ctx.VerifyPairsDev(_to_dev(torch, none).data_ptr(), len(none), n, d_o.data_ptr())
    assert e.value.code == -2
    label, tr, rep, summ = ctx.VerifyPairsDev(d_r.data_ptr(), len(recs), n, d_o.data_ptr())
    assert rep.tobytes() == s["host"][3].tobytes()

"""CPU: pair verification's host twins (mi355_pair_edges_host, mi355_pair_cycles_host, mi355_pair_residuals_host,
mi355_verify_pairs_results) against the numpy restatement (tests/verify_ref.py), byte for byte, on the records and graphs the GPU tests use
(tests/verify_cases.py); the loop's output against the existing select-connected and alignment functions; the refusals."""
import numpy as np
import pytest

import imagemosaicing_amd as im
from tests import verify_cases as vc
from tests import verify_ref as vr


def test_edges_host_equals_reference():
    recs = vc.edge_records()
    want = vr.edges(recs, vc.EDGE_IMAGES)
    for count in vc.EDGE_COUNTS:
        assert im.pair_edges_host(recs[:count], vc.EDGE_IMAGES).tobytes() == want[:count].tobytes()
    ok = want["flags"] == 3
    assert ok.sum() > 150 and np.isfinite(want["F"][ok]).all() and np.isfinite(want["B"][ok]).all()
    for q in np.flatnonzero(ok)[:20]:                   # B is F's inverse
        P = want["F"][q].reshape(3, 3) @ want["B"][q].reshape(3, 3)
        assert np.allclose(P / P[2, 2], np.eye(3), atol=1e-6)
    n1 = np.flatnonzero(ok & (want["n_in"] == 1))[0]    # one tie: a zero-area box at that tie
    assert want["box"][n1].tolist() == [recs["b"]["x"][n1, 0], recs["b"]["y"][n1, 0]] * 2
    q = np.flatnonzero(ok & (want["n_in"] >= 31))[0]    # the box orders -0 below +0
    assert np.signbit(want["box"][q][1]) and want["box"][q][1] == 0 and want["box"][q][2] == np.float32(3999.5)


@pytest.mark.parametrize("graph", ["t0", "t1", "t65", "star", "special"])
def test_cycles_host_equals_reference(graph):
    edg, n = {"t0": lambda: vc.translation_graph(0), "t1": lambda: vc.translation_graph(1, (3.0, 4.0)), "t65": lambda: vc.translation_graph(65, (6.0, 0.0)),
              "star": lambda: vc.star_graph(400, 2), "special": vc.special_graph}[graph]()
    want = vr.cycles(edg, n, 6.0)
    assert im.pair_cycles_host(edg, n, 6.0).tobytes() == want.tobytes()
    if graph == "t65":
        assert (int(want["n_ok"][0]), int(want["n_bad"][0]), float(want["min_e2"][0])) == (65, 0, 36.0)
        below = float(np.nextafter(6.0, 0.0))
        c = im.pair_cycles_host(edg, n, below)
        assert c.tobytes() == vr.cycles(edg, n, below).tobytes() and (int(c["n_ok"][0]), int(c["n_bad"][0])) == (0, 65)


def test_residuals_host_equals_reference():
    recs = vc.edge_records()
    h9, label = vc.edge_transforms()
    for lb in (label, None):
        want = vr.residuals(recs, h9, lb)
        assert im.pair_residuals_host(recs, h9, lb).tobytes() == want.tobytes()
    assert want["n_den"][23] > 0 and want["n_used"][23] > 0 and want["n_used"][19] == 0


@pytest.mark.parametrize("name,pct", [("grid36", 10), ("strip40d", 10), ("strip_adjacent", 0)])
def test_loop_host_equals_reference_and_the_existing_alignment(name, pct):
    s = vc.survey(name, 2, pct)
    recs, n = s["recs"], s["n"]
    ref = vr.verify(recs, n)
    out, label, tr, rep, summ = im.verify_pairs_results(recs, n)
    assert np.array_equal(rep["verdict"], ref["verdict"]) and np.array_equal(rep["round"], ref["round"]) and np.array_equal(label, ref["label"])
    assert np.array_equal(rep["n_ok"], ref["n_ok"]) and np.array_equal(rep["n_bad"], ref["n_bad"]) and int(summ["rounds"]) == ref["rounds"]
    assert rep["min_e2"].tobytes() == ref["min_e2"].tobytes()
    assert np.allclose(rep["rms"], ref["rms"], rtol=1e-3) and abs(float(summ["gate"]) - ref["gate"]) < 1e-3 * ref["gate"]
    kept = np.isin(rep["verdict"], vr.KEPT_VERDICTS)
    assert np.array_equal(kept, ~s["wrong"]) and int(summ["n_labelled"]) == n
    want_label = im.select_connected_results(recs[kept], n)
    assert label.tobytes() == want_label.tobytes()
    assert tr.tobytes() == im.global_affine_align_results(recs[kept], n, label=want_label).tobytes()
    assert out[kept].tobytes() == recs[kept].tobytes()
    dem = out[~kept]
    assert not dem["ok"].any() and not dem["accepted"].any() and not dem["H"].any()
    assert np.array_equal(dem["n_in"], recs["n_in"][~kept]) and dem["a"].tobytes() == recs["a"][~kept].tobytes() and dem["b"].tobytes() == recs["b"][~kept].tobytes()
    # a second pass over its own output changes nothing
    out2 = im.verify_pairs_results(out, n)
    assert out2[0].tobytes() == out.tobytes() and out2[2].tobytes() == tr.tobytes()


def test_host_refusals():
    s = vc.survey("strip_adjacent", 2, 0)
    recs, n = s["recs"], s["n"]
    for kw, match in ((dict(cycle_tol=0.0), "cycle_tol"), (dict(gate_abs=np.nan), "gate_abs"), (dict(gate_k=np.inf), "gate_k"), (dict(max_rounds=0), "max_rounds")):
        with pytest.raises(im.Mi355Error, match=match) as e:
            im.verify_pairs_results(recs, n, **kw)
        assert e.value.code == -1
    with pytest.raises(im.Mi355Error, match="n_images"):
        im.verify_pairs_results(recs, 65536)
    bad = recs.copy()
    bad["n_in"][3] = 401
    with pytest.raises(im.Mi355Error, match="record 3"):
        im.verify_pairs_results(bad, n)
    dup = np.concatenate([recs, recs[3:4]])
    with pytest.raises(im.Mi355Error, match="records 3 and 11"):
        im.verify_pairs_results(dup, n)
    none = recs.copy()
    none["accepted"] = 0
    with pytest.raises(im.Mi355Error, match="no pair could be verified") as e:
        im.verify_pairs_results(none, n)
    assert e.value.code == -2

"""CPU: the crafted cases of tests/guided_cases.py hold what they claim under the numpy restatement tests/guided_ref.py, five single-line mutations
of the restatement each change at least one of them, and the restatement rescues weak pairs on the reference's own 20 frames (oracle SIFT,
orc_match_pair and orc_ransac2d at 2.5 px, 1000 samples, seed 12345; guides chained from the accepted consecutive pairs in float64)."""
import os

import numpy as np
import pytest

from tests import guided_cases as gc
from tests import guided_ref as gr
from tests import oracle_lib as ol
from tests.golden_util import GOLD

SEED = 12345
MUTATIONS = ("radius_lt", "no_k_tie", "no_q_tie", "ratio_le", "cut_d1")


def _ids(a, b):
    return [(int(q), int(k)) for q, k in zip(b["id"], a["id"])]


def test_crafted_cases_hold_their_facts():
    seen = set()
    for c in gc.crafted_cases() + gc.guide_cases():
        a, b, dd = gc.ref_select(c)
        f = c["facts"]
        seen |= set(f)
        if "ids" in f:
            assert sorted(_ids(a, b)) == sorted(f["ids"]), c["tag"]
        if "ids_in_order" in f:
            assert _ids(a, b) == f["ids_in_order"], c["tag"]
            assert f["n_survivors"] == len(gc.ref_select(c, max_selected=10 ** 6)[0]), c["tag"]
            assert list(dd) == sorted(dd) and (f["n_survivors"] <= 400 or dd[399] == dd[398]), (c["tag"], "equal d1 across the cut")
        if "d1" in f:
            assert list(dd) == f["d1"], c["tag"]
        if "n_sel" in f:
            assert len(a) == f["n_sel"], c["tag"]
        assert np.array_equal(a["x"], c["xy_i"][a["id"], 0]) and np.array_equal(b["y"], c["xy_j"][b["id"], 1]), c["tag"]
    assert seen >= {"ids", "ids_in_order", "d1", "n_sel"}


def test_sizes_and_guides_find_ties_where_they_can():
    for c in gc.size_cases():
        a, b, dd = gc.ref_select(c)
        m = min(len(c["xy_i"]), len(c["xy_j"]))
        assert len(a) <= min(m, 400) and (m < 10 or len(a) >= min(400, int(0.4 * m))), (c["tag"], len(a))
        assert len(set(a["id"])) == len(a) == len(set(b["id"])), (c["tag"], "one to one")
    for c in gc.guide_cases():
        n = len(gc.ref_select(c)[0])
        if c["tag"].split()[1] in ("identity", "shift", "similarity", "projective", "zero"):
            assert n >= 150, (c["tag"], n)
            assert 7 not in gc.ref_select(c)[1]["id"] or "zero" not in c["tag"]
        else:
            assert n == 0, (c["tag"], n)


def test_max_selected_cuts_the_same_order():
    c = gc.survivor_case(500)
    full = gc.ref_select(c)
    cut = gc.ref_select(c, max_selected=100)
    assert len(cut[0]) == 100 and all(np.array_equal(x[:100], y) for x, y in zip(full, cut))


@pytest.mark.parametrize("mut", MUTATIONS)
def test_each_mutation_changes_a_crafted_case(mut):
    changed = []
    for c in gc.crafted_cases():
        want, got = gc.ref_select(c), gc.ref_select(c, mut=mut)
        if any(not np.array_equal(x, y) for x, y in zip(want, got)):
            changed.append(c["tag"])
    assert changed, mut


def test_planted_pair_is_recovered(oracle):
    c = gc.planted_case()
    a, b, dd = gc.ref_select(c)
    assert len(a) == 400                                    # 300 true and 100 wrong ties survive; the cut keeps the best 400
    r = gr.record(oracle, 0, 1, c["xy_i"], c["d_i"], c["xy_j"], c["d_j"], c["G"], seed=SEED)
    assert int(r["accepted"]) == 1 and int(r["n_selected"]) == 400 and 280 <= int(r["n_in"]) <= 310, (int(r["n_in"]),)


# ---- the reference's 20 frames ------------------------------------------------------------------------------------------------------------------
def _frame(k):
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(os.path.join(GOLD, "DSC%05d.JPG" % (4 + k))).convert("RGB"))[:, :, ::-1])


def golden_survey(orc, spans=(2, 3, 4)):
    """features of the 20 frames, the pair stage's verdict on the consecutive pairs and on every pair of the given spans, and the guided record of
    every span pair whose chain of consecutive pairs is accepted -- all on the oracle"""
    frames = [_frame(k) for k in range(20)]
    h, w = frames[0].shape[:2]
    feats = ol.parallel_map(lambda f: orc.sift(f, 2000), frames)
    xy = [np.stack([kp["x"], kp["y"]], 1).astype(np.float32) for kp, _ in feats]
    ds = [d for _, d in feats]

    def stage(ij):
        i, j = ij
        nin, i1, i2, H, ns = orc.match_pair(xy[i], ds[i], xy[j], ds[j], w, h, 2.5, SEED)
        return dict(i=i, j=j, n_in=nin, accepted=int(nin > 30), H=H)

    cons = ol.parallel_map(stage, [(k, k + 1) for k in range(19)])
    chains = gr.chain_guides(cons, 20)
    out = {}
    for s in spans:
        pairs = [(i, i + s) for i in range(20 - s) if (i, i + s) in chains]
        base = ol.parallel_map(stage, pairs)
        guided = ol.parallel_map(lambda ij: gr.record(orc, ij[0], ij[1], xy[ij[0]], ds[ij[0]], xy[ij[1]], ds[ij[1]], chains[ij], 2.5, SEED), pairs)
        out[s] = dict(pairs=pairs, base=base, guided=guided)
    return out


def test_guided_matching_rescues_weak_pairs_on_the_reference_frames():
    orc = ol.load_oracle_fast()
    sv = golden_survey(orc, spans=(2, 3))
    for s in (2, 3):
        g = sv[s]
        print("span %d: chained %d, pair stage accepts %d, guided accepts %d; n_in %s -> %s" % (
            s, len(g["pairs"]), sum(b["accepted"] for b in g["base"]), sum(int(r["accepted"]) for r in g["guided"]),
            [b["n_in"] for b in g["base"]], [int(r["n_in"]) for r in g["guided"]]))
    assert len(sv[2]["pairs"]) == 18 and len(sv[3]["pairs"]) == 17
    assert sum(b["accepted"] for b in sv[2]["base"]) == 15
    assert all(int(r["accepted"]) for r in sv[2]["guided"])
    assert sum(int(r["accepted"]) for r in sv[3]["guided"]) >= 8
    for s in (2, 3):
        assert not any(int(r["accepted"]) and int(r["n_selected"]) < 7 for r in sv[s]["guided"])

"""GPU: the frame-table family on ONE used context -- the median, seamline, optimised-seamline, feathered and refined renders, their covers,
host and _into forms, the gain and block-gain stages, the overview levels and the striped preview (tests/used_context.py: render_steps).

Every step is held, byte for byte, to its stage's own reference (tests/median_ref.py, seamline_ref.py, seamcut_ref.py, feather_ref.py,
gain_ref.py, block_gain_ref.py, overview_ref.py; the refined render to the oracle) and to the same call on a fresh context.  The surveys:

  L  twelve 128 x 96 frames, canvas 337 x 310: four list blocks, 43 x 39 cells at level 3
  W  130 frames of 12 .. 16 px on a 24 x 24 canvas: 130 table entries, ramps and frame ids; 6 x 6 cells
  S  two 64 x 96 frames, canvas 88 x 96: 22 x 24 cells at level 2
  B  two 32 x 24 frames 100 rows apart, canvas 32 x 124: the rows between them meet no frame's box

Large comes before small (tests/test_used_context_plan.py asserts, per shared buffer, that more was left than is written); device outputs are
pre-filled and their rows wider than the layout's, host rows carry a tail that must stay.
"""
import numpy as np
import pytest

from tests import gain_ref as gr
from tests import used_context as uc

pytestmark = pytest.mark.gpu


def test_renders_gains_and_overviews_on_one_used_context(oracle):
    import torch
    import imagemosaicing_amd as im
    env = uc.Env(torch, im)
    uc.render_prepare(env, oracle)
    steps = uc.render_steps()
    res = uc.run_steps(env, steps, oracle)
    V = uc.render_surveys()
    L, W, S, B = V["L"], V["W"], V["S"], V["B"]
    # the gains of the one-call form are the host solve of the restatement's statistics, bit for bit
    for X, step in ((L, 2), (S, 4)):
        recs, cover = gr.stats_ref(X.maps(oracle), X.pairs, step)
        g = res["gain compensate %s, step %d" % (X.name, step)][0]
        assert g.tobytes() == im.solve_gains(gr.to_records(recs, X.pairs), cover).tobytes() and not np.all(g.view(np.float32) == 1.0), X.name
    # the surveys do what they were built for
    assert res["median W, depth 9"][2].max() > 64 and res["seamline host L"][1].max() == 12
    rep = dict(zip(sorted(S.seamcut(oracle)["report"]), res["seamcut W, three stages"][2]))
    assert set(rep) == {"changed", "energy_after", "energy_before", "fallback"}
    assert S.seamcut(oracle)["report"]["changed"] > 0 and L.seamcut(oracle)["report"]["changed"] > 0       # the cell maps name frames
    for name in ("seamline B", "feathered B, 1 stripe"):
        c = res[name][0]
        assert c[:23, :3 * B.cw].any() and c[100:, :3 * B.cw].any() and not c[24:99].any() and not c[:, 3 * B.cw:].any(), name
    own, cnt = res["seamline B, maps only"]
    assert not own[24:99].any() and not cnt[24:99].any() and set(np.unique(own)) == {0, 1, 2}
    stripe = res["refined L, rows 100 .. 249"][0]
    assert np.all(stripe[:100] == uc.FILL8) and np.all(stripe[250:] == uc.FILL8) and np.array_equal(stripe[100:250], res["refined L"][0][100:250])
    assert np.all(res["median into L, depth 5"][0][:, 3 * L.cw:] == uc.TAIL) and np.all(res["seamcut into S"][0][:, 3 * S.cw:] == uc.TAIL)

"""GPU: the chip family on ONE used context -- BlendSeamCellsDev, ChipsAndMasksSeam, MosaicBlendedSeam / Dev / Into, plain ChipsAndMasks and
MosaicBlendedDev (whole canvas and stripe), MultiBandBlend of held chips, and SeamCellsDev on the mosaic grid directly around
BlendSeamCellsDev (tests/used_context.py: chip_steps).

Every step is held, byte for byte, to tests/blend_seam_ref.py (records, cells, report, masks, chips; canvases against the oracle's blend of
the restated masks, as in tests/test_gpu_blend_seam.py), the plain forms to the oracle, SeamCellsDev to tests/seamcut_ref.py -- and to the
same call on a fresh context.  The cases, of tests/blend_seam_patterns.py, tests/warp_patterns.py and tests/blend_edges.py:

  big          twelve 128 x 96 frames, canvas 337 x 310, 22 x 20 cells at level 4: first, and again at the end
  thin_named1  4 chips, three with a 0 / 0 distance map, under a caller's map: the smallest, directly after the largest
  many130      130 chips of 16 x 16 in one ownership block (several batches), 6 x 6 cells
  crafted3     3 chips, 22 x 34 cells at level 2: the most cells, before many130's 36
  keep_drops   a dropped frame that the caller's map names in every cell
  seventy, thin, strip   the plain forms between the seam forms
"""
import numpy as np
import pytest

from tests import used_context as uc

pytestmark = pytest.mark.gpu


def test_blends_along_seams_and_plain_on_one_used_context(oracle):
    import torch
    import imagemosaicing_amd as im
    env = uc.Env(torch, im)
    uc.chip_prepare(env, oracle)
    res = uc.run_steps(env, uc.chip_steps(), oracle)
    # the large case at the end equals its first run
    assert np.array_equal(res["blended along seams big, device, again"][0], res["blended along seams big, device, first"][0])
    # SeamCellsDev on the mosaic grid gives the same map before and after BlendSeamCellsDev went through the label stage's buffers
    for name in ("crafted3", "many130"):
        assert np.array_equal(res["mosaic cells %s, before" % name][0], res["mosaic cells %s, after" % name][0]), name
    # the cases do what they were built for: maps that name frames, more than 64 chips that own something, a stripe of the whole canvas
    X = uc.chip_cases()
    assert X["G"].own(oracle)["report"]["changed"] > 0 and X["M"].own(oracle)["report"]["changed"] > 0
    assert len(X["M"].own(oracle)["masks"]) == 130 and sum(1 for m in X["M"].own(oracle)["masks"] if m.any()) > 32
    seventy = uc.plain_cases()[0].chips(oracle)
    assert sum(1 for m in seventy["masks"] if m.any()) > 64
    whole, part = res["plain blended strip"][0], res["plain blended strip, from row 49"][0]
    assert np.array_equal(part, whole[49:]) and part.shape[0] > 0
    assert np.all(res["blended along seams keep_drops, into"][0][:, -8:] == uc.TAIL)

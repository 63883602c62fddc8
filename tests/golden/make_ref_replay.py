#!/usr/bin/env python3
"""Records tests/golden/ref_replay.npz: the outputs of the reference's own code (oracle/_ref/libref_oracle.so, built by
oracle/ref/build_ref.sh from the reference tree) for every call the tests that take the `ref` fixture make.  Where
oracle/_ref cannot be built, the fixture replays these outputs (tests/oracle_lib.py RefReplay).

Run where the reference tree is at hand, after build():   python tests/golden/make_ref_replay.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import imagemosaicing_amd as im  # noqa: E402
from tests import oracle_lib as ol  # noqa: E402
from tests import test_oracle_vs_ref as t_vs  # noqa: E402
from tests import test_overlap as t_ov  # noqa: E402
from tests import test_match_patterns_oracle as t_mp  # noqa: E402
from tests import test_warp_patterns_oracle as t_wp  # noqa: E402


def run_all(orc, ref):
    for t in (t_vs.test_inverse_random, t_vs.test_ransac_random, t_vs.test_warp_random, t_vs.test_ransac_degenerate_inputs):
        t(orc, ref)
    t_ov.test_resample_by_overlap_vs_reference(im, ref)
    t_ov.test_oracle_chips_and_masks_vs_reference(orc, ref)
    t_wp.check_all_vs_reference(orc, ref)          # the warp stage's edge cases (tests/warp_patterns.py) where the reference's code is defined
    t_mp.check_select_vs_reference(orc, ref)       # the grid walk on cell-edge and cell-filling patterns (tests/match_patterns.py), inside the label array


def main():
    R = ol.load_ref()
    assert R is not None, "needs oracle/_ref (the reference tree)"
    rec = ol.RefRecorder(R)
    orc = ol.load_oracle()
    run_all(orc, rec)
    rec.save()
    run_all(orc, ol.RefReplay())          # the replay gives back what the library gave
    # ... and a digest tells a changed byte, dtype or shape from the array it was made of
    a = np.arange(4096, dtype=np.uint8)
    d = ol.ArrayDigest.of(a)
    b = a.copy(); b[1234] ^= 1
    assert np.array_equal(a, d) and np.array_equal(d, a.copy())
    assert not np.array_equal(b, d) and not np.array_equal(a.view(np.int8), d) and not np.array_equal(a.reshape(64, 64), d)
    print("%d calls -> %s (%d bytes)" % (len(rec.calls), ol.REF_REPLAY, os.path.getsize(ol.REF_REPLAY)))


if __name__ == "__main__":
    main()

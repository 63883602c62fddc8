"""GPU: the selection's hash table in memory on the pass-0 side (unique_compact_mem, csrc/sift.hip).  select_unique_kernel keeps the
listed locations in LDS up to 4096 points; beyond that the table lies in the frame's candidate list.  No frame of tests/test_gpu_sift_dedupe.py
(all at most 512x384) stores that many records, so this file has one larger frame: terrain 1100x780 with select_margin = 65536, where
every record is listed (more than 4096 of them, duplicates among them) and the 2000 strongest keypoints must be the oracle's."""
import numpy as np
import pytest

from tests import sift_patterns as sp
from tests.synth_frames import terrain
from tests.test_gpu_sift_edges import _same

pytestmark = pytest.mark.gpu


def test_everything_listed_through_the_memory_table(oracle):
    import imagemosaicing_amd as im
    w, h = 1100, 780
    img = terrain(w, h, seed=sp.shape_seed(w, h))
    want = oracle.sift(img)
    c = im.Context(0)
    base = c.SiftExtract(0, img, max_kp=4096)
    cnt0 = c.last_sift_counters()
    c.set_option("select_margin", 65536)
    kp, desc = c.SiftExtract(1, img, max_kp=4096)
    cnt = c.last_sift_counters()
    c.close()
    print(f"terrain {w}x{h}: refined records {cnt[1]}, oriented keypoints margin 256: {cnt0[2]}, margin 65536: {cnt[2]}, kept {cnt[3]}")
    assert cnt[1] > 4096, "too few records to leave the LDS table"
    assert cnt[1] <= 2000 + 65536 and cnt[5] == 0                      # everything listed in pass 0
    # every location oriented exactly once: as many keypoints as keep-all returns (duplicates left in would add theirs)
    assert cnt0[2] < cnt[2] == len(oracle.sift(img, 0, 32768)[0])
    _same((base[0], base[1].astype(np.uint8)), want, "terrain 1100x780 margin 256")
    _same((kp, desc.astype(np.uint8)), want, "terrain 1100x780 margin 65536")

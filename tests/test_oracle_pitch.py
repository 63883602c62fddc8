"""CPU: the oracle reads caller frames by their row pitch (ws) and nothing else -- the premise of tests/test_gpu_frame_geometry.py, which
holds the HIP kernels on padded, odd and mixed geometry to the oracle run on contiguous copies.  Every call here goes through oracle.L with
the frames of tests/pitched.py (padding and gaps full of non-zero garbage) and must give the bytes of the same call on contiguous rows,
down to the tiny frames the GPU tests use."""
import ctypes as C

import numpy as np

from tests import oracle_lib as ol
from tests import pitched as pf


def _warp(oracle, ptr, w, h, ws, ch, h9):
    h9 = np.ascontiguousarray(h9, np.float32)
    dst = C.c_void_p()
    dw, dh, dws = C.c_int(), C.c_int(), C.c_int()
    rc = oracle.L.orc_image_projection_transform(C.c_void_p(ptr), int(w), int(h), int(ws), int(ch), h9.ctypes.data_as(C.c_void_p),
                                                 C.byref(dst), C.byref(dw), C.byref(dh), C.byref(dws))
    assert rc == 0
    buf = np.ctypeslib.as_array(C.cast(dst, ol.u8p), shape=(dh.value, dws.value)).copy()
    oracle.L.orc_free(dst)
    return buf, dw.value, dh.value, dws.value


def test_warp_reads_rows_by_pitch(oracle):
    rng = np.random.default_rng(2)
    sizes = [(2, 2), (2, 9), (9, 2), (7, 5), (333, 257), (201, 150), (130, 97)]
    for ch in (3, 1):
        imgs = pf.mixed_images(sizes, seed=4, ch=ch)
        for shift in range(5):
            fr = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, ch, shift), offsets=[k % 4 for k in range(len(sizes))], seed=shift)
            for k in range(len(sizes)):
                H = np.eye(3) + rng.normal(0, 0.05, (3, 3))
                H[0, 2], H[1, 2] = rng.uniform(-20, 20), rng.uniform(-20, 20)
                H[2, 0], H[2, 1], H[2, 2] = rng.normal(0, 1e-4), rng.normal(0, 1e-4), 1
                h9 = H.reshape(9).astype(np.float32)
                got = _warp(oracle, fr.host_ptrs()[k], fr.w[k], fr.h[k], fr.ws[k], ch, h9)
                rc, want = oracle.image_projection_transform(imgs[k], h9)
                assert rc == 0 and got[1:] == want[1:] and np.array_equal(got[0], want[0]), (ch, shift, sizes[k], int(fr.ws[k]))


def test_mosaic_and_chips_read_rows_by_pitch(oracle):
    sizes = pf.MIXED_SIZES
    imgs = pf.mixed_images(sizes, seed=1)
    h9s = pf.mixed_h9s(sizes)
    _, want = oracle.mosaic_images_refined(imgs, h9s)
    blend_h9s = h9s.copy()
    blend_h9s[pf.MIXED_SKIP, 8] = 1.0
    chips, cw, chh, dG = oracle.chip_layout([i.shape[1] for i in imgs], [i.shape[0] for i in imgs], blend_h9s)
    assert len(chips) == len(imgs)
    for shift in range(5):
        fr = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, 3, shift), seed=10 + shift)
        w, h, ws = fr.geom()
        ptrs = fr.host_ptr_array(skip={pf.MIXED_SKIP})        # the skipped frame is never read
        cwv, chv, cws = C.c_int(), C.c_int(), C.c_int()
        args = (ptrs, w.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), ws.ctypes.data_as(C.c_void_p), len(imgs), h9s.ctypes.data_as(C.c_void_p))
        assert oracle.L.orc_mosaic_images_refined(*args, None, C.byref(cwv), C.byref(chv), C.byref(cws)) == 0
        canvas = np.zeros((chv.value, cws.value), np.uint8)
        assert oracle.L.orc_mosaic_images_refined(*args, canvas.ctypes.data_as(C.c_void_p), C.byref(cwv), C.byref(chv), C.byref(cws)) == 0
        assert (cwv.value, chv.value, cws.value) == want[1:] and np.array_equal(canvas, want[0]), shift
        for c in chips:
            k = int(c["img"])
            want_chip, want_mask = oracle.chip_warp(imgs[k], blend_h9s[k], dG, c)
            ccws, mws = (int(c["w"]) * 3 + 3) & ~3, (int(c["w"]) + 3) & ~3
            chip = np.full((int(c["h"]), ccws), 0, np.uint8)
            mask = np.full((int(c["h"]), mws), 0, np.uint8)
            ci = np.array([c], ol.CHIPINFO)
            h9 = np.ascontiguousarray(blend_h9s[k])
            rc = oracle.L.orc_chip_warp(C.c_void_p(fr.host_ptrs()[k]), int(w[k]), int(h[k]), int(ws[k]), h9.ctypes.data_as(C.c_void_p),
                                        dG.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), chip.ctypes.data_as(C.c_void_p), ccws,
                                        mask.ctypes.data_as(C.c_void_p), mws)
            assert rc == 0 and np.array_equal(chip, want_chip) and np.array_equal(mask, want_mask), (shift, k)
    # the tiny frames take part: each has a chip, and all but the 2 x 2 one (no texel with a right and a lower neighbour) own pixels of the blend
    r = oracle.chips_and_masks(imgs, blend_h9s)
    assert len(r["chips"]) == len(imgs)
    for c, m in zip(r["chips"], r["masks"]):
        assert m[:, :int(c["w"])].any() == (sizes[int(c["img"])] != (2, 2)), int(c["img"])


def test_sift_and_surf_read_rows_by_pitch(oracle):
    from tests.synth_frames import terrain
    imgs = [terrain(333, 257, seed=3), terrain(201, 150, seed=9)]
    fr = pf.PitchedFrames(imgs, [1000, pf.ipl_pitch(201)], offsets=[1, 3], seed=7)
    for k, img in enumerate(imgs):
        okp, odesc = oracle.sift(img)
        kp = np.zeros(2048, ol.KEYPOINT)
        desc = np.zeros((2048, 128), np.uint8)
        oracle.L.orc_sift.restype = C.c_int
        n = oracle.L.orc_sift(C.c_void_p(fr.host_ptrs()[k]), int(fr.w[k]), int(fr.h[k]), int(fr.ws[k]), 2000,
                              kp.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), 2048)
        assert n == len(okp) > 100 and np.array_equal(kp[:n], okp) and np.array_equal(desc[:n], odesc), k
        skp, sdesc = oracle.surf(img)
        kp = np.zeros(4096, ol.KEYPOINT)
        desc = np.zeros((4096, 128), np.float32)
        oracle.L.orc_surf.restype = C.c_int
        n = oracle.L.orc_surf(C.c_void_p(fr.host_ptrs()[k]), int(fr.w[k]), int(fr.h[k]), int(fr.ws[k]), C.c_float(50.0),
                              kp.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), 4096)
        assert n == len(skp) > 10 and np.array_equal(kp[:n], skp) and np.array_equal(desc[:n].view(np.uint32), sdesc.view(np.uint32)), k


def test_pitched_frames_helper():
    imgs = pf.mixed_images([(5, 3), (2, 2), (7, 4)], seed=0)
    fr = pf.PitchedFrames(imgs, [16, 13, 256], offsets=[1, 2, 3], seed=4)
    for k, img in enumerate(imgs):
        assert fr.base[k] % 256 == k + 1 and fr.view(k).shape == (img.shape[0], int(fr.ws[k]))
        assert np.array_equal(fr.pixels(k), img)
        pad = fr.padding(k)
        assert pad.shape[1] == fr.ws[k] - 3 * fr.w[k] and (pad != 0).all()
    assert fr.base[0] + 3 * 16 <= fr.base[1] and fr.base[1] + 2 * 13 <= fr.base[2]

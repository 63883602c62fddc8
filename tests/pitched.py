"""Frames with row pitch: the caller-owned layout of include/mi355_mosaic.h (rows of `ws` bytes, IplImage / BitmapImage), for the tests
of tests/test_gpu_frame_geometry.py and tests/test_oracle_pitch.py.

A PitchedFrames holds every frame in ONE host buffer: frame k starts at a 256-byte boundary plus offsets[k] (so a device copy of the
buffer gives base pointers at +1, +2, +3 ...), its rows are `ws[k]` bytes apart, and every byte that is not a pixel (row padding, the gaps
between frames) is non-zero garbage of the frame's own seed.  `imgs` keeps the contiguous h x w x ch copies the references are run on.
"""
import ctypes as C

import numpy as np


def ipl_pitch(w, ch=3):
    """IplImage / CreateBitmap8U widthStep: rows padded to 4 bytes"""
    return (ch * w + 3) & ~3


def pitch_256(w, ch=3):
    return (ch * w + 255) & ~255


class PitchedFrames:
    def __init__(self, imgs, pitches, offsets=None, seed=0):
        self.imgs = [np.ascontiguousarray(i, np.uint8) for i in imgs]
        n = len(self.imgs)
        self.n = n
        self.ch = [1 if i.ndim == 2 else i.shape[2] for i in self.imgs]
        self.w = np.array([i.shape[1] for i in self.imgs], np.int32)
        self.h = np.array([i.shape[0] for i in self.imgs], np.int32)
        self.ws = np.array(pitches, np.int32)
        offsets = [0] * n if offsets is None else list(offsets)
        assert len(self.ws) == n and len(offsets) == n
        assert all(self.ws[k] >= self.ch[k] * self.w[k] for k in range(n))
        self.base, end = [], 0
        for k in range(n):
            b = ((end + 255) & ~255) + int(offsets[k])
            self.base.append(b)
            end = b + int(self.h[k]) * int(self.ws[k])
        self.nbytes = ((end + 255) & ~255) + 256
        self.buf = np.empty(self.nbytes, np.uint8)
        rng = np.random.default_rng(seed)
        self.buf[:] = rng.integers(1, 256, self.nbytes, dtype=np.uint8)
        for k in range(n):
            # each frame's padding: its own non-zero garbage
            b, e = self.base[k], self.base[k] + int(self.h[k]) * int(self.ws[k])
            self.buf[b:e] = np.random.default_rng(seed * 1000 + k + 1).integers(1, 256, e - b, dtype=np.uint8)
            self.view(k)[:, :self.row_bytes(k)] = self.imgs[k].reshape(int(self.h[k]), -1)

    def row_bytes(self, k):
        return self.ch[k] * int(self.w[k])

    def view(self, k, buf=None):
        """frame k as an [h, ws] view of the host buffer (or of `buf`, a copy of it)"""
        buf = self.buf if buf is None else buf
        b = self.base[k]
        return buf[b:b + int(self.h[k]) * int(self.ws[k])].reshape(int(self.h[k]), int(self.ws[k]))

    def pixels(self, k, buf=None):
        """the h x w x ch pixels of frame k in `buf` (default: the host buffer)"""
        v = self.view(k, buf)[:, :self.row_bytes(k)]
        return np.ascontiguousarray(v).reshape(self.imgs[k].shape)

    def padding(self, k, buf=None):
        return np.ascontiguousarray(self.view(k, buf)[:, self.row_bytes(k):])

    def host_ptrs(self):
        return [self.buf.ctypes.data + b for b in self.base]

    def host_ptr_array(self, skip=()):
        return (C.c_void_p * self.n)(*[None if k in skip else p for k, p in enumerate(self.host_ptrs())])

    def geom(self):
        """(w, h, ws) int32 arrays"""
        return self.w.copy(), self.h.copy(), self.ws.copy()

    def to_device(self, torch, device="cuda"):
        """(tensor, device pointers): one device copy of the whole buffer, frame k at data_ptr() + base[k]"""
        t = torch.from_numpy(self.buf.copy()).to(device)
        torch.cuda.synchronize()
        return t, [t.data_ptr() + b for b in self.base]

    def device_bytes(self, t):
        return t.cpu().numpy()



# ---- one mixed-geometry frame set ---------------------------------------------------------------------------------------------------------
# widths with w % 4 of 1, 2, 3 (and 0), heights off multiples of 8 / 16 / 32, the smallest frames the renders accept (2 x 2, 2 x N, N x 2)
MIXED_SIZES = [(333, 257), (201, 150), (130, 97), (2, 2), (2, 9), (9, 2), (241, 7), (161, 121), (50, 50), (77, 61)]
MIXED_SKIP = 8                     # h9[8] == 0: the refined render skips it


def pitch_kinds(w, ch=3):
    """3w (unpadded: odd w makes it odd), IplImage, 3w + 1, 3w + 13, rounded to 256 bytes"""
    return [ch * w, ipl_pitch(w, ch), ch * w + 1, ch * w + 13, pitch_256(w, ch)]


def mixed_pitches(sizes, ch=3, shift=0):
    return [pitch_kinds(w, ch)[(k + shift) % 5] for k, (w, h) in enumerate(sizes)]


def mixed_h9s(sizes, seed=5, skip=MIXED_SKIP):
    """frame 0 fixed at the origin, the others scattered over it (heavy overlap), odd ones with a projective row"""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    h9s = np.zeros((n, 9), np.float32)
    for k in range(n):
        H = np.eye(3)
        if k:
            a = rng.uniform(-0.25, 0.25)
            s = rng.uniform(0.8, 1.25)
            H[:2, :2] = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) + rng.normal(0, 0.03, (2, 2))
            H[0, 2], H[1, 2] = rng.uniform(-40, 260), rng.uniform(-30, 170)
            if k % 2:
                H[2, 0], H[2, 1] = rng.normal(0, 4e-4), rng.normal(0, 4e-4)
        h9s[k] = H.reshape(9)
    if skip is not None:
        h9s[skip, 8] = 0.0
    return h9s


def mixed_images(sizes, seed=0, ch=3):
    from tests.synth import texture
    out = [texture(w, h, seed=seed + 17 * k) for k, (w, h) in enumerate(sizes)]
    return out if ch == 3 else [np.ascontiguousarray(i[..., 1]) for i in out]

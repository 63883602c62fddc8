"""GPU: the three one-pass renders (refined, feathered, seamline) share one host path -- the entry check, the frame table with its upload and
candidate lists, the used-flag pass, the staging of host images -- and one set of context buffers.  The suites of each render pin it alone;
this one runs them interleaved on ONE context, over two surveys of very different size, and holds every result to the bytes of the same
call on a fresh context: nothing a call leaves in the shared table, lists, flags or staging buffers may reach the next one.

  A  four 160 x 120 frames with overlapping translations and one mild projective; two of them on a padded pitch (canvas about 300 x 250)
  B  two 32 x 24 frames 100 rows apart (canvas 32 x 124): the canvas rows between them meet no frame's box

The device canvases are pre-filled and wider than the layout's rows, so that an unwritten row and uncleared padding show.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL8, FILL16, TAIL = 7, 0x5555, 201


def _frame(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(3 * x + y) % 256, (x + 5 * y + 40 * seed) % 256, (2 * x + 2 * y + 90) % 256], axis=2)
    return ((base + rng.integers(0, 64, (h, w, 3))) % 256).astype(np.uint8)


def _survey_a():
    imgs = [_frame(160, 120, 1 + k) for k in range(5)]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (5, 1))
    for k, (dx, dy) in enumerate([(0, 0), (100, 20), (30, 110), (120, 125)]):
        h9s[k, 2], h9s[k, 5] = dx, dy
    h9s[4] = [1.02, 0.03, 60, -0.02, 0.98, 55, 1e-4, 5e-5, 1]
    return imgs, h9s, [0, 5, 0, 36, 0]


def _survey_b():
    imgs = [_frame(32, 24, 11), _frame(32, 24, 12)]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    h9s[1, 5] = 100
    return imgs, h9s, [0, 0]


class Survey:
    def __init__(self, torch, im, imgs, h9s, pads):
        self.imgs, self.h9s = imgs, h9s
        self.t = []
        for a, pad in zip(imgs, pads):
            h, w = a.shape[:2]
            buf = np.full((h, 3 * w + pad), 0xEE, np.uint8)
            buf[:, :3 * w] = a.reshape(h, 3 * w)
            self.t.append(torch.from_numpy(buf).cuda())
        torch.cuda.synchronize()
        self.ptrs = [t.data_ptr() for t in self.t]
        self.w = [a.shape[1] for a in imgs]; self.h = [a.shape[0] for a in imgs]; self.ws = [t.shape[1] for t in self.t]
        self.cw, self.ch, lws, _ = im.mosaic_layout(self.w, self.h, h9s)
        self.cws = lws + 8                                                   # a caller's wider row: [3 cw, cws) is padding to clear
        self.geom = (self.ptrs, self.w, self.h, self.ws, h9s)

    def canvas(self, torch):
        c = torch.full((self.ch, self.cws), FILL8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                                            # the fill runs on torch's stream, the library on the ctx's own
        return c

    def maps(self, torch):
        m = [torch.full((self.ch, self.cw), FILL16, dtype=torch.int16, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        return m


def _steps(torch, A, B):
    """(name, call): call(ctx) -> tuple of numpy arrays"""
    u16 = lambda t: t.cpu().numpy().view(np.uint16)

    def refined(S):
        def f(ctx):
            c = S.canvas(torch)
            ctx.MosaicImagesRefinedDev(*S.geom, c.data_ptr(), S.cw, S.ch, S.cws)
            return (c.cpu().numpy(),)
        return f

    def feathered(S, cuts):
        def f(ctx):
            c = S.canvas(torch)
            for row0, row1 in zip(cuts[:-1], cuts[1:]):
                ctx.MosaicFeatheredDev(*S.geom, c.data_ptr(), S.cw, S.ch, S.cws, row0, row1 - row0, ramp=9)
            return (c.cpu().numpy(),)
        return f

    def seamline(S, canvas=True):
        def f(ctx):
            c = S.canvas(torch) if canvas else None
            own, cnt = S.maps(torch)
            if canvas:
                ctx.MosaicSeamlineDev(*S.geom, c.data_ptr(), S.cw, S.ch, S.cws, d_owner=own.data_ptr(), d_count=cnt.data_ptr())
            else:
                ctx.MosaicSeamlineDev(None, S.w, S.h, None, S.h9s, 0, S.cw, S.ch, S.cws, d_owner=own.data_ptr(), d_count=cnt.data_ptr())
            return ((c.cpu().numpy(),) if canvas else ()) + (u16(own), u16(cnt))
        return f

    def into(S, name, **kw):
        def f(ctx):
            out = np.full((S.ch, 3 * S.cw + 13), TAIL, np.uint8)
            getattr(ctx, name)(S.imgs, None, S.h9s, out=out, **kw)
            return (out,)
        return f

    return [
        ("refined A", refined(A)),
        ("feathered B", feathered(B, [0, B.ch])),
        ("seamline A", seamline(A)),
        ("seamline cover B", lambda ctx: (ctx.SeamlineCover(B.w, B.h, B.h9s),)),
        ("exact stripe cover A", lambda ctx: (ctx.StripeCover(A.w, A.h, A.h9s, 0, A.ch, exact=True),)),
        ("feathered A, two stripes", feathered(A, [0, 131, A.ch])),
        ("refined B", refined(B)),
        ("seamline B, maps only", seamline(B, canvas=False)),
        ("refined_into A", into(A, "MosaicImagesRefinedInto")),
        ("feathered_into A", into(A, "MosaicFeatheredInto", ramp=9)),
        ("seamline_into A", into(A, "MosaicSeamlineInto")),
        # beyond the listed sequence: the seamline canvas of B (its frame-free rows), and the host forms, whose staging buffer the three share
        ("seamline B", seamline(B)),
        ("refined host B", lambda ctx: (ctx.MosaicImagesRefined(B.imgs, B.h9s)[0],)),
        ("feathered host A", lambda ctx: (ctx.MosaicFeathered(A.imgs, A.h9s, ramp=9)[0],)),
        ("seamline host B", lambda ctx: ctx.MosaicSeamline(B.imgs, B.h9s, want_owner=True)[::4]),
    ]


def test_interleaved_renders_equal_fresh_contexts():
    import torch
    import imagemosaicing_amd as im
    A, B = Survey(torch, im, *_survey_a()), Survey(torch, im, *_survey_b())
    assert 280 <= A.cw <= 320 and 230 <= A.ch <= 270 and (B.cw, B.ch) == (32, 124)
    steps = _steps(torch, A, B)
    ctx = im.Context(0)
    shared = [call(ctx) for _, call in steps]
    ctx.close()
    for (name, call), got in zip(steps, shared):
        fresh = im.Context(0)
        want = call(fresh)
        fresh.close()
        assert len(got) == len(want) > 0
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a, b), "%s: %d values differ from a fresh context's" % (name, int((a != b).sum()))
    res = dict(zip([n for n, _ in steps], shared))
    # the surveys do what they were built for
    assert res["seamline A"][2].max() >= 3 and res["seamline cover B"][0].all() and res["exact stripe cover A"][0].any()
    assert not np.array_equal(res["refined A"][0], res["seamline A"][0]) and not np.array_equal(res["refined A"][0], res["feathered A, two stripes"][0])
    # B: the rows that meet no frame's box are written as zeros, and so is the padding of every row, in all three renders
    box1 = int(100 - 0.5)                                                    # frame 1's box begins at (int)(100 - 0.5f); frame 0's ends at row 23
    for name in ("refined B", "feathered B", "seamline B"):
        c = res[name][0]
        assert c.shape == (B.ch, B.cws) and c[:23, :3 * B.cw].any() and c[100:, :3 * B.cw].any(), name
        assert not c[24:box1].any(), name + ": frame-free rows"
        assert not c[:, 3 * B.cw:].any(), name + ": row padding"
    for name in ("seamline B", "seamline B, maps only"):
        own, cnt = res[name][-2:]
        assert not own[24:box1].any() and not cnt[24:box1].any() and set(np.unique(own)) == {0, 1, 2}, name
    # A: padding cleared on every row of the device canvases; the bytes past 3 cw of an _into destination stay the caller's
    for name in ("refined A", "seamline A", "feathered A, two stripes"):
        assert not res[name][0][:, 3 * A.cw:].any(), name + ": row padding"
    for name in ("refined_into A", "feathered_into A", "seamline_into A"):
        assert np.all(res[name][0][:, 3 * A.cw:] == TAIL), name
    assert np.array_equal(res["refined_into A"][0][:, :3 * A.cw], res["refined A"][0][:, :3 * A.cw])
    assert np.array_equal(res["seamline_into A"][0][:, :3 * A.cw], res["seamline A"][0][:, :3 * A.cw])
    assert np.array_equal(res["feathered_into A"][0][:, :3 * A.cw], res["feathered A, two stripes"][0][:, :3 * A.cw])
